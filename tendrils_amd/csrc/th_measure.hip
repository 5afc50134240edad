// th_measure.hip - measure programs: a caller's reduction over the state ring.  The other five kinds of program write - the
// ring, a view image, a vertex record, a varying -; what a caller could learn of its particles was th_stats' seven fixed fields
// or the whole ring through the host.  A measure program is the caller's per-particle sample function (th_measure_prelude.inc:
// th_measure_main) run under the reduction th_stats is built on (th_kernels.hip: stats_kernel / stats_fold_kernel): per-lane
// accumulation over a grid-stride loop, a __shfl_xor butterfly per wave, four waves folded through LDS, one plain-stored partial
// per workgroup, then ONE workgroup that folds the partials in a fixed assignment - no atomics anywhere, so the same ring order
// gives the same bits on every run.  It reads the ring buffer where it lies - tile-sorted slots through their perm table, a
// packed ring's 8-byte texels in place - and disturbs nothing: no slot order, no draw geometry, no counter.
//
// The caller's kernels leave the partials; the fold does not depend on the caller's source and lives here.  The same fold
// kernel folds the ranks' result blocks of a row-band job (th_measure_global), in rank order.
#include "th_ring.hpp"           // RingView, TH_RING_BUFFER_OK: what the passes that read the ring where it lies share

using namespace thi;

namespace {

#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#undef TH_TAPS
#define TH_PACKED(...) #__VA_ARGS__
const char kPacked[] =
#include "th_packed.inc"
    ;
#undef TH_PACKED
const char kPrelude[] =
#include "th_measure_prelude.inc"
    ;

constexpr int kMeasureChannels = 8;
using Partial = th_measure_result;          // a workgroup's partial, a result block: one layout (th_measure_prelude.inc: th_measure_partial)
static_assert(sizeof(Partial) == 144 && offsetof(Partial, sum) == 16 && offsetof(Partial, min) == 80 && offsetof(Partial, max) == 112,
              "th_measure_result: layout shared with th_measure_prelude.inc");

// the launch record (th_measure_prelude.inc: th_measure_args, th_program_uniform_block - the same layout)
struct MeasureArgs {
    const float4 *in, *flow;
    const uint32_t *perm;
    Partial *part;
    uint32_t count, width, rows, row0, global_height;
    int32_t fw, fh;
    uint32_t reserved;
};
using KernArgs = ProgramKernArgs<MeasureArgs>;
static_assert(sizeof(MeasureArgs) == 64 && offsetof(KernArgs, u) == 64 && sizeof(KernArgs) == 64 + kUniformBytes,
              "launch record: layout shared with th_measure_prelude.inc");

constexpr size_t kMaxParts = 2048;          // program_launch's grid: th::grid_for(count, 8)

// what a lane of the fold carries: the prelude's th_measure_acc at eight channels
struct Acc {
    unsigned long long taken, particles;
    double sum[kMeasureChannels];
    float mn[kMeasureChannels], mx[kMeasureChannels];
};
__device__ __forceinline__ void acc_add(Acc &r, const Partial &p)
{
    r.taken += p.taken; r.particles += p.particles;
#pragma unroll
    for (int c = 0; c < kMeasureChannels; ++c) {
        r.sum[c] += p.sum[c];
        r.mn[c] = p.min[c] < r.mn[c] ? p.min[c] : r.mn[c];
        r.mx[c] = p.max[c] > r.mx[c] ? p.max[c] : r.mx[c];
    }
}

// `nparts` blocks -> 1, by ONE workgroup of 256 threads: thread k mod 256 takes block k, in increasing k; then the butterfly and
// the wave fold of the caller's kernels.  The assignment is fixed: the same blocks give the same bits.  particles: what the
// result says of it - 0: the sum of the blocks' own (the ranks' blocks of th_measure_global).
__global__ __launch_bounds__(256) void measure_fold_kernel(const Partial *part, uint32_t nparts, unsigned long long particles, Partial *out)
{
    __shared__ Partial sh[4];
    Acc r;
    r.taken = 0ull; r.particles = 0ull;
#pragma unroll
    for (int c = 0; c < kMeasureChannels; ++c) { r.sum[c] = 0.0; r.mn[c] = __builtin_huge_valf(); r.mx[c] = -__builtin_huge_valf(); }
    // (one block's nine loads in flight at a time.  All eight blocks of a thread loaded up front, at clamped indices - 72 loads,
    // 332 VGPRs - measured SLOWER: the fold and its launch 0.0147 ms instead of 0.0120; profiles/measure_program.txt)
    for (uint32_t k = threadIdx.x; k < nparts; k += 256u) acc_add(r, part[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        r.taken += __shfl_xor(r.taken, o); r.particles += __shfl_xor(r.particles, o);
#pragma unroll
        for (int c = 0; c < kMeasureChannels; ++c) {
            r.sum[c] += __shfl_xor(r.sum[c], o);
            const float on = __shfl_xor(r.mn[c], o), ox = __shfl_xor(r.mx[c], o);
            r.mn[c] = on < r.mn[c] ? on : r.mn[c];
            r.mx[c] = ox > r.mx[c] ? ox : r.mx[c];
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
        Partial &p = sh[threadIdx.x >> 6];
        p.taken = r.taken; p.particles = r.particles;
#pragma unroll
        for (int c = 0; c < kMeasureChannels; ++c) { p.sum[c] = r.sum[c]; p.min[c] = r.mn[c]; p.max[c] = r.mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        Partial t = sh[0];
        for (int w = 1; w < 4; ++w) {
            t.taken += sh[w].taken; t.particles += sh[w].particles;
#pragma unroll
            for (int c = 0; c < kMeasureChannels; ++c) {
                t.sum[c] += sh[w].sum[c];
                t.min[c] = sh[w].min[c] < t.min[c] ? sh[w].min[c] : t.min[c];
                t.max[c] = sh[w].max[c] > t.max[c] ? sh[w].max[c] : t.max[c];
            }
        }
        if (particles) t.particles = particles;
        *out = t;
    }
}

// the context's result blocks: [0] this context's own | [1 .. world] the ranks', gathered | [world + 1] the job's
th_status measure_storage(th_context *c)
{
    if (!c->measure_parts) if (th_status s = c->measure_parts.alloc(kMaxParts)) return s;
    const size_t need = 2 + (size_t)std::max(c->comm_world, 1);
    if (c->measure_blocks.size() < need) {
        TH_HIP(hipStreamSynchronize(c->stream));          // (a job joined since the last measure: nothing still reads the old blocks)
        if (th_status s = c->measure_blocks.alloc(need)) return s;
    }
    return TH_OK;
}

// the checks, then the caller's kernel over ring buffer `buffer` where it lies and the fold into block 0: enqueued, nothing more
th_status measure_enqueue(th_context *c, th_program *prog, const char *entry, const void *uniforms, uint32_t uniform_bytes, int32_t buffer)
{
    if (th_status s = use(c, true)) return s;             // read-only: the last draw's geometry and a fused launch's statistics stay valid
    if (th_status s = program_run_args(prog, kMeasureProgram, entry, uniforms, uniform_bytes)) return s;
    TH_RING_BUFFER_OK(c, buffer, entry);
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    if (th_status s = measure_storage(c)) return s;
    const RingView ring = ring_read(c, buffer);
    KernArgs k{};
    MeasureArgs &a = k.a;
    a.in = static_cast<const float4 *>(ring.in); a.perm = ring.perm;
    a.flow = c->flow; a.fw = c->fw; a.fh = c->fh;
    a.part = c->measure_parts;
    a.count = ring.count; a.width = ring.width; a.rows = (uint32_t)c->cfg.height;
    a.row0 = ring.row0; a.global_height = (uint32_t)c->cfg.global_height;
    k.set_uniforms(uniforms, uniform_bytes);
    const int grid = th::grid_for(c->texels(), 8);
    LaunchTimer timer;
    if (th_status s = timer.begin(c)) return s;
    if (th_status s = program_launch(c, m->entry[c->packed ? kMeasurePacked : kMeasureF32], c->texels(), k)) return s;
    if (th_status s = timer.end(c)) return s;
    hipLaunchKernelGGL(measure_fold_kernel, dim3(1), dim3(256), 0, c->stream, c->measure_parts.get(), (uint32_t)grid,
                       (unsigned long long)c->texels(), c->measure_blocks.get());
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // namespace

extern "C" {

th_status th_measure_program_compile(const char *source, const char *name, int32_t channels, th_program **out)
{
    if (out) *out = nullptr;
    TH_REQUIRE(channels >= 1 && channels <= kMeasureChannels, "a measure program has 1 .. %d channels (%d)", kMeasureChannels, channels);
    return program_compile(kMeasureProgram, "#define TH_MEASURE_CHANNELS " + std::to_string(channels) + "\n" + kTaps + "\nnamespace th {\n" + kPacked + "\n}\n" + kPrelude,
                           source, name, out);
}

th_status th_measure_async(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t buffer, void **device_result)
{
    TH_REQUIRE(c, "null context");
    if (th_status s = measure_enqueue(c, prog, "th_measure_async", uniforms, uniform_bytes, buffer)) return s;
    if (device_result) *device_result = c->measure_blocks.get();
    return TH_OK;
}

th_status th_measure_run(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t buffer, th_measure_result *out)
{
    TH_REQUIRE(c && out, "th_measure_run: null context or output");
    if (th_status s = measure_enqueue(c, prog, "th_measure_run", uniforms, uniform_bytes, buffer)) return s;
    return read_back(c, out, c->measure_blocks.get(), sizeof *out);
}

// the local measure, ONE all-gather of the ranks' blocks (equal parts: a single ncclAllGather on RCCL), the fold over them in
// rank order on the context's stream: every rank ends with the same bits
th_status th_measure_global(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t buffer, th_measure_result *out)
{
    TH_REQUIRE(c && out, "th_measure_global: null context or output");
    if (th_status s = measure_enqueue(c, prog, "th_measure_global", uniforms, uniform_bytes, buffer)) return s;
    if (!c->comm || c->comm_world <= 1) return read_back(c, out, c->measure_blocks.get(), sizeof *out);      // a world of one is th_measure_run: no collective
    const int world = c->comm_world;
    std::vector<size_t> bytes((size_t)world, sizeof(Partial)), offset((size_t)world);
    for (int r = 0; r < world; ++r) offset[(size_t)r] = (size_t)r * sizeof(Partial);
    Partial *blocks = c->measure_blocks;
    if (c->transport->allgather_bytes(c->comm, blocks, blocks + 1, bytes.data(), offset.data(), c->comm_rank, world, c->stream))
        return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    hipLaunchKernelGGL(measure_fold_kernel, dim3(1), dim3(256), 0, c->stream, blocks + 1, (uint32_t)world, 0ull, blocks + 1 + world);
    TH_HIP(hipGetLastError());
    return read_back(c, out, blocks + 1 + world, sizeof *out);
}

}  // extern "C"
