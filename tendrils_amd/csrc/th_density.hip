// th_density.hip - the density map: the particles' count and summed velocity on a grid over the view, left in an image the
// library's own passes read (a caller texture slot, the spawner's image).  th_stats and the measure programs say numbers ABOUT
// the particles; this says where they are, without the ring leaving the device.  A built-in pass: fixed kernels, no hiprtc.
//
// Every accumulation is an INTEGER addition - a cell's count in uint32, its velocity sums in int64 of 2^-32 units - so the
// result depends on neither the slot order nor the order the adds arrive in: a tile-sorted ring, a packed ring's decoded texels
// and the same ring in texel order give the same bits, run after run.  Three kernels:
//   density_clear_kernel    the accumulators (20 B a cell) and the info block
//   density_tally_kernel    the ring where it lies (no perm: a cell does not depend on who the particle is): every workgroup takes
//                           a run of consecutive blocks of 2048 slots, eight non-temporal loads a lane in flight.  It keeps a
//                           WINDOW of 48 x 48 cells in LDS (46 KB: a 32 x 32 tile of cells and 8 cells around it) under LDS
//                           integer atomics, and the window lives on from block to block: while at least half of a block's
//                           particles fall into it, it stays; else it is flushed - its non-zero cells, one global atomic per
//                           word, neighbouring lanes neighbouring cells - and moves to the tile of the first particle a wave
//                           found, if a quarter of the block's particles are there.  Over tile-sorted slots a run of blocks is
//                           one neighbourhood of the view and most adds end in LDS; in texel order no window gathers a
//                           quarter, none opens, and every particle goes straight to global integer atomics - as do, always,
//                           the cells outside the window.  (The comparison arm - all global atomics, no window - was measured
//                           and is not in the product: profiles/density_map.txt.)
//   density_convert_kernel  accumulators -> RGBA32F texels, and the sum of the counts = `inside`
// No float atomics, no inline assembly; every index that addresses LDS or memory comes from a value compared in range first.
#include "th_ring.hpp"           // Slot, wave_sum, fold_counters, RingView: what the passes that read the ring where it lies share

using namespace thi;

namespace {

constexpr int kWinHalo = 8, kWinSide = 32 + 2 * kWinHalo, kWinCells = kWinSide * kWinSide;      // the window: a 32 x 32 tile and a halo around it
constexpr uint32_t kLaneSlots = 8, kBlockSlots = 256u * kLaneSlots;   // slots a lane / a workgroup takes at a time
constexpr int kTallyPerCu = 3;            // 46 KB of LDS a workgroup
constexpr int kInfoWords = 5;             // th_density_info
enum { kParticles, kLive, kInside, kOutside, kNonfinite };
static_assert(sizeof(th_density_info) == kInfoWords * 8 && sizeof(th_density_uniforms) == 24, "th_density_*: the header's layout");
constexpr int64_t kMaxCells = 1 << 22;

struct DensityParams {
    const void *in;                   // the ring buffer: float4 or, packed, uint2 per slot
    uint32_t count;
    float view_x, view_y;
    int32_t w, h;
    uint32_t *cnt;                    // [cells]
    unsigned long long *sum;          // [cells][2]: int64 in two's complement
    unsigned long long *info;         // [kInfoWords]
    float4 *dst;
};

// accumulators (16-byte words) and the info block: {particles, 0, 0, 0, 0}
__global__ __launch_bounds__(256) void density_clear_kernel(v4u *acc, uint32_t words, unsigned long long *info, unsigned long long particles)
{
    const v4u zero = {0u, 0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < words; i += gridDim.x * 256u) acc[i] = zero;
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)kInfoWords) info[threadIdx.x] = threadIdx.x == kParticles ? particles : 0ull;
}

// a velocity component in 2^-32 units, round-half-even; false: not finite, adds nothing
TH_D bool density_quantum(float v, long long &q)
{
    q = 0;
    if (!(__builtin_fabsf(v) < __builtin_huge_valf())) return false;
    q = __float2ll_rn(__builtin_fminf(__builtin_fmaxf(v, -4.0f), 4.0f) * 4294967296.0f);
    return true;
}

template <bool PACKED>
__global__ __launch_bounds__(256) void density_tally_kernel(const DensityParams p, uint32_t run)
{
    __shared__ uint32_t win_cnt[kWinCells];
    __shared__ unsigned long long win_sum[kWinCells * 2];
    __shared__ int cand[4][2];                  // per wave: the cell of its first inside particle of the block (x < 0: none)
    __shared__ uint32_t votes[2][3];            // by the block's parity: its inside particles | those in the window | ... in the window proposed
    __shared__ uint32_t tally[4 * 3];           // live, outside, nonfinite of the four waves (fold_counters)
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)kWinCells; i += 256u) { win_cnt[i] = 0u; win_sum[2 * i] = 0ull; win_sum[2 * i + 1] = 0ull; }
    if (tid < 3u) { votes[0][tid] = 0u; votes[1][tid] = 0u; }
    __syncthreads();
    const float wf = (float)p.w, hf = (float)p.h, wm1 = (float)(p.w - 1), hm1 = (float)(p.h - 1);
    uint32_t live = 0u, outside = 0u, nonfinite = 0u;
    const uint32_t nblocks = (p.count + kBlockSlots - 1u) / kBlockSlots;
    const uint32_t first = blockIdx.x * run, last = first + run < nblocks ? first + run : nblocks;
    int ox = 0, oy = 0;                         // the window's corner, while it is `open` (uniform over the workgroup, as is all that moves it)
    bool open = false;
    // the window's non-zero cells to memory, one global atomic a word, and the window zero again (cells past the grid's edge
    // stay zero: nothing was added there); the caller's barriers order it against the LDS atomics on both sides
    auto flush = [&]() {
        for (uint32_t i = tid; i < (uint32_t)kWinCells; i += 256u) {
            const uint32_t n = win_cnt[i];
            if (!n) continue;
            const unsigned long long sx = win_sum[2 * i], sy = win_sum[2 * i + 1];
            win_cnt[i] = 0u; win_sum[2 * i] = 0ull; win_sum[2 * i + 1] = 0ull;
            const int x = ox + (int)(i % (uint32_t)kWinSide), y = oy + (int)(i / (uint32_t)kWinSide);
            if (x < 0 || y < 0 || x >= p.w || y >= p.h) continue;
            const uint32_t cell = (uint32_t)y * (uint32_t)p.w + (uint32_t)x;
            atomicAdd(&p.cnt[cell], n);
            if (sx) atomicAdd(&p.sum[2 * (size_t)cell], sx);
            if (sy) atomicAdd(&p.sum[2 * (size_t)cell + 1], sy);
        }
    };
    for (uint32_t b = first; b < last; ++b) {
        const uint32_t base = b * kBlockSlots + tid;
        typename Slot<PACKED>::Raw raw[kLaneSlots];      // all of the lane's loads in flight before anything is decoded
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) {
            const uint32_t idx = base + k * 256u;
            raw[k] = idx < p.count ? Slot<PACKED>::load(p.in, idx) : Slot<PACKED>::none();
        }
        v4f s[kLaneSlots];
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) s[k] = Slot<PACKED>::state(raw[k]);
        int cx[kLaneSlots], cy[kLaneSlots];     // the cell; cx < 0: none (inert, outside, past the end)
        int mine_x = -1, mine_y = -1;           // the lane's first cell
        uint32_t inside = 0u, hits = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) {
            cx[k] = cy[k] = -1;
            if (!slot_live(s[k])) continue;                  // (a slot past the end was loaded as inert)
            ++live;
            const float fx = __builtin_floorf((((s[k].x * p.view_x) + 1.0f) * 0.5f) * wf);
            const float fy = __builtin_floorf((((s[k].y * p.view_y) + 1.0f) * 0.5f) * hf);
            if (fx >= 0.0f && fx <= wm1 && fy >= 0.0f && fy <= hm1) {       // (a NaN or infinite position fails)
                cx[k] = (int)fx; cy[k] = (int)fy;
                if (mine_x < 0) { mine_x = cx[k]; mine_y = cy[k]; }
                ++inside;
                hits += (open && (uint32_t)(cx[k] - ox) < (uint32_t)kWinSide && (uint32_t)(cy[k] - oy) < (uint32_t)kWinSide) ? 1u : 0u;
            } else ++outside;
        }
        bool windowed = false;
        {
            // Does the window stay?  Every lane reaches the butterflies and the barriers: all that follows is uniform.
            const uint32_t par = b & 1u;
            inside = wave_sum(inside); hits = wave_sum(hits);
            const unsigned long long have = __ballot(mine_x >= 0);
            if (have && (tid & 63u) == (uint32_t)(__ffsll((long long)have) - 1)) { cand[tid >> 6][0] = mine_x; cand[tid >> 6][1] = mine_y; }
            if (!have && (tid & 63u) == 0u) cand[tid >> 6][0] = -1;
            if ((tid & 63u) == 0u && inside) { atomicAdd(&votes[par][0], inside); atomicAdd(&votes[par][1], hits); }
            if (tid < 3u) votes[par ^ 1u][tid] = 0u;      // (the next block's: everybody has read them before the barrier that ended the last block)
            __syncthreads();
            const uint32_t all_inside = votes[par][0];
            windowed = open;
            if (all_inside && !(open && 2u * votes[par][1] >= all_inside)) {
                // fewer than half of the block's particles fall into the window (or there is none): it moves to the 32 x 32 block
                // of cells around the first particle a wave found, kWinHalo cells more on every side - if a quarter are there
                if (open) { flush(); open = false; }
                int nx = -1, ny = -1;
#pragma unroll
                for (int wv = 3; wv >= 0; --wv) if (cand[wv][0] >= 0) { nx = cand[wv][0]; ny = cand[wv][1]; }
                nx = (nx & ~31) - kWinHalo; ny = (ny & ~31) - kWinHalo;
                uint32_t there = 0u;
#pragma unroll
                for (uint32_t k = 0; k < kLaneSlots; ++k)
                    there += (cx[k] >= 0 && (uint32_t)(cx[k] - nx) < (uint32_t)kWinSide && (uint32_t)(cy[k] - ny) < (uint32_t)kWinSide) ? 1u : 0u;
                there = wave_sum(there);
                if ((tid & 63u) == 0u && there) atomicAdd(&votes[par][2], there);
                __syncthreads();                          // (and the flush's zeros are in place before anybody adds)
                open = 4u * votes[par][2] >= all_inside;
                ox = nx; oy = ny;
                windowed = open;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) {
            if (cx[k] < 0) continue;
            long long qx, qy;
            const bool okx = density_quantum(s[k].z, qx), oky = density_quantum(s[k].w, qy);
            if (!(okx && oky)) ++nonfinite;
            const uint32_t dx = (uint32_t)(cx[k] - ox), dy = (uint32_t)(cy[k] - oy);
            if (windowed && dx < (uint32_t)kWinSide && dy < (uint32_t)kWinSide) {
                const uint32_t at = dy * (uint32_t)kWinSide + dx;
                atomicAdd(&win_cnt[at], 1u);
                if (qx) atomicAdd(&win_sum[2 * at], (unsigned long long)qx);
                if (qy) atomicAdd(&win_sum[2 * at + 1], (unsigned long long)qy);
            } else {
                const uint32_t cell = (uint32_t)cy[k] * (uint32_t)p.w + (uint32_t)cx[k];      // 0 <= cx < w, 0 <= cy < h: below w * h
                atomicAdd(&p.cnt[cell], 1u);
                if (qx) atomicAdd(&p.sum[2 * (size_t)cell], (unsigned long long)qx);
                if (qy) atomicAdd(&p.sum[2 * (size_t)cell + 1], (unsigned long long)qy);
            }
        }
        __syncthreads();                                  // (the block's LDS atomics before a flush; cand and votes before the next block writes them)
    }
    if (open) flush();
    fold_counters<kLive, kOutside, kNonfinite>(tally, p.info, {live, outside, nonfinite});      // every lane of the workgroup is here
}

// one lane per cell: (count, sumx * 2^-32, sumy * 2^-32, count ? 1 : 0), every conversion to nearest; the counts' sum is `inside`
__global__ __launch_bounds__(256) void density_convert_kernel(const DensityParams p)
{
    __shared__ unsigned long long part[4];      // (fold_counters)
    const uint32_t cells = (uint32_t)p.w * (uint32_t)p.h;
    unsigned long long inside = 0ull;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cells; i += gridDim.x * 256u) {
        const uint32_t n = p.cnt[i];
        const long long sx = (long long)p.sum[2 * (size_t)i], sy = (long long)p.sum[2 * (size_t)i + 1];
        inside += n;
        p.dst[i] = make_float4((float)n, (float)((double)sx * 0x1p-32), (float)((double)sy * 0x1p-32), n ? 1.0f : 0.0f);
    }
    fold_counters<kInside>(part, p.info, {inside});      // (every lane arrives: the loop above returns nobody)
}

size_t acc_words(int64_t cells) { return (size_t)((cells * 20 + 15) / 16); }      // 16 B of sums and 4 B of count a cell, in 16-byte words

// the checks, the destination's shape, the three kernels: enqueued, nothing more
th_status density_enqueue(th_context *c, const th_density_uniforms *u, int32_t buffer, const char *entry)
{
    if (th_status s = use(c, true)) return s;             // read-only: the last draw's geometry and a fused launch's statistics stay valid
    TH_REQUIRE(u, "%s: null uniforms", entry);
    TH_REQUIRE(u->w >= 1 && u->h >= 1 && (int64_t)u->w * u->h <= kMaxCells, "%s: a grid of %dx%d (1 <= w, h and w * h <= %lld)", entry, u->w, u->h, (long long)kMaxCells);
    TH_REQUIRE(std::isfinite(u->viewSize[0]) && std::isfinite(u->viewSize[1]), "%s: viewSize is not finite", entry);
    TH_REQUIRE(u->dest == TH_VIEW_TEXTURE || u->dest == TH_VIEW_SPAWN_IMAGE, "%s: dest %d (TH_VIEW_TEXTURE or TH_VIEW_SPAWN_IMAGE)", entry, u->dest);
    TH_REQUIRE(u->dest != TH_VIEW_TEXTURE || (u->slot >= 0 && u->slot < TH_MAX_TEXTURES), "%s: texture slot %d outside 0..%d", entry, u->slot, TH_MAX_TEXTURES - 1);
    TH_RING_BUFFER_OK(c, buffer, entry);
    TH_RING_TEXELS_OK(c, entry);
    const int64_t cells = (int64_t)u->w * u->h;
    if (!c->density_info) if (th_status s = c->density_info.alloc(kInfoWords)) return s;
    if (c->density_acc.size() < acc_words(cells)) {
        TH_HIP(hipStreamSynchronize(c->stream));          // (an earlier density's kernels may still read the old accumulators)
        if (th_status s = c->density_acc.alloc(acc_words(cells))) return s;
    }
    DensityParams p{};
    if (u->dest == TH_VIEW_TEXTURE) {                      // as th_texture_upload leaves the slot: the memory stays when shape and format do
        th_context::Texture &t = c->textures[u->slot];
        if (u->w != t.w || u->h != t.h || t.format != TH_TEX_RGBA32F) {
            if (th_status s = image_reshape(c, t.texels, t.w, t.h, u->w, u->h, sizeof(float4))) return s;
            t.format = TH_TEX_RGBA32F;
        }
        p.dst = reinterpret_cast<float4 *>(t.texels.get());
    } else {                                               // as th_spawn_image_upload leaves the image
        if (u->w != c->iw || u->h != c->ih) if (th_status s = image_reshape(c, c->image, c->iw, c->ih, u->w, u->h)) return s;
        p.dst = c->image;
    }
    const RingView ring = ring_read(c, buffer);            // where it lies, in whatever slot order (a cell does not depend on who the particle is: ring.perm is not read)
    p.in = ring.in; p.count = ring.count;
    p.view_x = u->viewSize[0]; p.view_y = u->viewSize[1];
    p.w = u->w; p.h = u->h;
    p.sum = reinterpret_cast<unsigned long long *>(c->density_acc.get());
    p.cnt = reinterpret_cast<uint32_t *>(p.sum + 2 * (size_t)cells);
    p.info = c->density_info;
    const uint32_t words = (uint32_t)acc_words(cells);
    hipLaunchKernelGGL(density_clear_kernel, dim3(th::grid_for(words, 8)), dim3(256), 0, c->stream, reinterpret_cast<v4u *>(c->density_acc.get()), words,
                       p.info, (unsigned long long)c->texels());
    // every workgroup a run of consecutive blocks, so that its window lives on from one block to the next: three workgroups on a
    // CU (the LDS), twelve waves with eight loads a lane in flight
    const uint32_t nblocks = (p.count + kBlockSlots - 1u) / kBlockSlots;
    const uint32_t run = (nblocks + 256u * kTallyPerCu - 1u) / (256u * kTallyPerCu), grid = (nblocks + run - 1u) / run;
    dispatch_packed(c, [&](auto packed) { hipLaunchKernelGGL(density_tally_kernel<decltype(packed)::value>, dim3(grid), dim3(256), 0, c->stream, p, run); });
    hipLaunchKernelGGL(density_convert_kernel, dim3(th::grid_for((size_t)cells, 8)), dim3(256), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // namespace

extern "C" {

th_status th_density_async(th_context *c, const th_density_uniforms *u, int32_t buffer, void **device_info)
{
    if (th_status s = density_enqueue(c, u, buffer, "th_density_async")) return s;
    if (device_info) *device_info = c->density_info.get();
    return TH_OK;
}

th_status th_density(th_context *c, const th_density_uniforms *u, int32_t buffer, th_density_info *out)
{
    TH_REQUIRE(c && out, "th_density: null context or output");
    if (th_status s = density_enqueue(c, u, buffer, "th_density")) return s;
    return read_back(c, out, c->density_info.get(), sizeof *out);
}

}  // extern "C"
