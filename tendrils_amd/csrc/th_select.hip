// th_select.hip - select: the particles of one ring buffer that match a fixed predicate, as 32-byte records in TEXEL order, the
// ring left where it lies.  Measure programs say numbers ABOUT the particles and the density map WHERE they are; this says WHICH
// ones - a box, a band of speeds, a 1 : n thinning - without the 16 bytes a particle of th_download_state, and without the move
// back to texel order that a download of tile-sorted slots costs.  A built-in pass: fixed kernels, no hiprtc, no program kind.
//
// Stream compaction through a bit per TEXEL.  Everything that decides is an integer or a float compare, so the result depends on
// neither the slot order, nor the order of arrival, nor the run:
//   select_mark_kernel     the ring where it lies, one non-temporal load a slot, tile-sorted slots through their perm table: the
//                          predicate, and the particle's bit into the mask word of its TEXEL.  In texel order a wave's 64 slots are
//                          one word: the wave's __ballot is that word, lane 0 stores it - and its popcount - with plain stores;
//                          nothing is cleared, nothing atomic.  Over tile-sorted slots the mask is cleared first and every MATCHED
//                          lane ORs its bit in (an integer atomic); select_count_kernel then takes the words' popcounts.  The live
//                          particles: per lane, a butterfly per wave, one integer atomic per workgroup.
//   (scan)                 th_sort.hip's exclusive scan over the words' counts, as it is; select_total_kernel leaves
//                          matched = offsets[last] + popcount(mask[last]) and written = min(matched, capacity) in the info block
//   select_gather_kernel   the slots again: a particle's bit is read from the MASK - the predicate is evaluated in one place
//                          only -, its rank is offsets[word] + popcount(word below its bit), and below `capacity` the slot is
//                          loaded and two 16-byte stores leave its record.  A slot whose bit is clear is not loaded.
// Why the bits are indexed by texel and not by slot: the records come in increasing texel, and there is no inverse of perm to
// walk a slot-indexed mask in that order; with texel-indexed bits the rank of a particle is a popcount below its own bit,
// whatever slot holds it.  The price is the second walk over the slots (and, tile-sorted, the atomics).
// No lane leaves the mark kernel before its wave-wide operations: the loop's bound is the workgroup's, a lane past the last
// slot carries "no match, not live".  Every index that addresses memory comes from a value compared in range first.
#include "th_select_match.hpp"   // Slot, SelectClauses, select_match, select_checks: shared with th_histogram.hip

using namespace thi;

namespace {

constexpr int kInfoWords = 4;             // th_select_info
enum { kParticles, kLive, kMatched, kWritten };
static_assert(sizeof(th_select_uniforms) == 40 && sizeof(th_selected) == 32 && sizeof(th_select_info) == kInfoWords * 8, "th_select_*: the header's layout");
static_assert(offsetof(th_selected, index) == 16, "th_selected: the state, then index, x, y, reserved");

struct SelectParams {
    const void *in;                   // the ring buffer: float4 or, packed, uint2 per slot
    const uint32_t *perm;             // slot -> local texel (tile-sorted slots), or null: texel order
    uint32_t count, width, row0;      // this context's texels; the texture's width; the band's first row
    uint32_t nwords;                  // mask words: (count + 63) / 64
    SelectClauses q;                  // the predicate's clauses
    uint32_t capacity;                // records the gather may write
    unsigned long long *mask;         // [nwords]: bit t & 63 of word t >> 6 is local texel t
    uint32_t *counts;                 // [nwords]: the words' popcounts, then (scanned in place) the matches before each word
    unsigned long long *info;         // [kInfoWords]
    th_selected *records;
};

TH_D uint32_t wave_sum(uint32_t v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

// {0, 0, 0, 0} into the info block and, over tile-sorted slots, zero into the mask
__global__ __launch_bounds__(256) void select_clear_kernel(unsigned long long *mask, uint32_t nwords, unsigned long long *info)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nwords; i += gridDim.x * 256u) mask[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)kInfoWords) info[threadIdx.x] = 0ull;
}

template <bool PACKED>
__global__ __launch_bounds__(256) void select_mark_kernel(const SelectParams p)
{
    __shared__ uint32_t part[4];
    const uint32_t tid = threadIdx.x;
    uint32_t live_n = 0u;
    // `base` is the workgroup's, a multiple of 256: every lane of the workgroup takes the same turns, a wave covers the 64
    // consecutive slots of ONE mask word
    for (uint32_t base = blockIdx.x * 256u; base < p.count; base += gridDim.x * 256u) {
        const uint32_t idx = base + tid;
        bool live = false, match = false;
        uint32_t t = idx;
        if (idx < p.count) {
            const v4f s = Slot<PACKED>::state(Slot<PACKED>::load(p.in, idx));
            if (p.perm) t = __builtin_nontemporal_load(p.perm + idx);          // (wave-uniform test: the argument segment)
            live = slot_live(s);
            match = t < p.count && select_match(p.q, s, live, t);
        }
        live_n += live ? 1u : 0u;
        if (!p.perm) {
            const unsigned long long word = __ballot(match);                    // every lane of the wave is here
            const uint32_t w = idx >> 6;
            if ((tid & 63u) == 0u && w < p.nwords) { p.mask[w] = word; p.counts[w] = (uint32_t)__popcll(word); }
        } else if (match) {
            atomicOr(&p.mask[t >> 6], 1ull << (t & 63u));                       // t < count: word t >> 6 < nwords
        }
    }
    live_n = wave_sum(live_n);
    if ((tid & 63u) == 0u) part[tid >> 6] = live_n;
    __syncthreads();
    if (tid == 0u) {
        const uint32_t n = part[0] + part[1] + part[2] + part[3];
        if (n) atomicAdd(&p.info[kLive], (unsigned long long)n);
    }
}

__global__ __launch_bounds__(256) void select_count_kernel(const unsigned long long *mask, uint32_t *counts, uint32_t nwords)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nwords; i += gridDim.x * 256u) counts[i] = (uint32_t)__popcll(mask[i]);
}

// behind the scan: counts[] holds the matches before each word
__global__ void select_total_kernel(const SelectParams p)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long matched = (unsigned long long)p.counts[p.nwords - 1u] + (unsigned long long)__popcll(p.mask[p.nwords - 1u]);
    p.info[kParticles] = p.count;
    p.info[kMatched] = matched;
    p.info[kWritten] = matched < p.capacity ? matched : (unsigned long long)p.capacity;
}

template <bool PACKED>
__global__ __launch_bounds__(256) void select_gather_kernel(const SelectParams p)
{
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < p.count; idx += gridDim.x * 256u) {
        const uint32_t t = p.perm ? __builtin_nontemporal_load(p.perm + idx) : idx;
        if (t >= p.count) continue;
        const unsigned long long word = p.mask[t >> 6], bit = 1ull << (t & 63u);
        if (!(word & bit)) continue;
        const uint32_t rank = p.counts[t >> 6] + (uint32_t)__popcll(word & (bit - 1ull));
        if (rank >= p.capacity) continue;
        const v4f s = Slot<PACKED>::state(Slot<PACKED>::load(p.in, idx));
        const uint32_t row = t / p.width;
        const v4u who = {t + p.row0 * p.width, t - row * p.width, row + p.row0, 0u};
        v4f *rec = reinterpret_cast<v4f *>(p.records + rank);
        rec[0] = s;
        *reinterpret_cast<v4u *>(rec + 1) = who;
    }
}

// the context's scratch, reserved by its first select (the texture's shape is the context's: only the records ever grow)
th_status select_storage(th_context *c, uint32_t nwords)
{
    if (!c->select_info) if (th_status s = c->select_info.alloc(kInfoWords)) return s;
    if (c->select_mask.size() < nwords) if (th_status s = c->select_mask.alloc(nwords)) return s;
    if (c->select_counts.size() < nwords) if (th_status s = c->select_counts.alloc(nwords)) return s;
    const size_t sums = th::exclusive_scan_sum_words(nwords);
    if (c->select_sums.size() < sums) if (th_status s = c->select_sums.alloc(sums)) return s;
    return TH_OK;
}

// `capacity` records of room; an earlier select's gather may still write the old ones
th_status select_records(th_context *c, uint32_t capacity)
{
    if (c->select_records.size() >= capacity) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    return c->select_records.alloc(capacity);
}

SelectParams select_params(th_context *c, const th_select_uniforms *u, int32_t buffer, uint32_t capacity)
{
    SelectParams p{};
    const float4 *buf = c->ring[(size_t)buffer];
    const int order = order_of(c, buf);                   // (the slot order stays: slot i holds texel perm[i])
    p.in = buf;
    p.perm = order >= 0 ? c->orders[(size_t)order].perm.get() : nullptr;
    p.count = (uint32_t)c->texels(); p.width = (uint32_t)c->cfg.width; p.row0 = (uint32_t)c->cfg.row0;
    p.nwords = (p.count + 63u) / 64u;
    p.q = select_clauses(c, u);
    p.capacity = capacity;
    p.mask = c->select_mask; p.counts = c->select_counts; p.info = c->select_info;
    p.records = c->select_records;
    return p;
}

// mark, count, scan, total: enqueued, nothing more.  The info block is complete behind them (written = min(matched, capacity))
th_status select_scan(th_context *c, const SelectParams &p)
{
    const int grid = th::grid_for(p.count, 8);
    hipLaunchKernelGGL(select_clear_kernel, dim3(th::grid_for(p.perm ? p.nwords : 1u, 8)), dim3(256), 0, c->stream, p.mask, p.perm ? p.nwords : 0u, p.info);
    if (c->packed) hipLaunchKernelGGL(select_mark_kernel<true>, dim3(grid), dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(select_mark_kernel<false>, dim3(grid), dim3(256), 0, c->stream, p);
    if (p.perm) hipLaunchKernelGGL(select_count_kernel, dim3(th::grid_for(p.nwords, 8)), dim3(256), 0, c->stream, p.mask, p.counts, p.nwords);
    th::launch_exclusive_scan_u32(p.counts, c->select_sums, p.nwords, c->stream);
    hipLaunchKernelGGL(select_total_kernel, dim3(1), dim3(64), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

th_status select_gather(th_context *c, const SelectParams &p)
{
    const int grid = th::grid_for(p.count, 8);
    if (c->packed) hipLaunchKernelGGL(select_gather_kernel<true>, dim3(grid), dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(select_gather_kernel<false>, dim3(grid), dim3(256), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // namespace

extern "C" {

th_status th_select_async(th_context *c, const th_select_uniforms *u, int32_t buffer, uint64_t capacity, void **device_records, void **device_info)
{
    if (th_status s = select_checks(c, u, buffer, "th_select_async")) return s;
    if (th_status s = use(c, true)) return s;             // read-only: the last draw's geometry and a fused launch's statistics stay valid
    const uint32_t room = (uint32_t)std::min<uint64_t>(capacity, c->texels());
    if (th_status s = select_storage(c, (uint32_t)((c->texels() + 63) / 64))) return s;
    if (th_status s = select_records(c, room)) return s;
    const SelectParams p = select_params(c, u, buffer, room);
    if (th_status s = select_scan(c, p)) return s;
    if (room) if (th_status s = select_gather(c, p)) return s;
    if (device_records) *device_records = room ? c->select_records.get() : nullptr;
    if (device_info) *device_info = c->select_info.get();
    return TH_OK;
}

th_status th_select(th_context *c, const th_select_uniforms *u, int32_t buffer, th_selected *out, uint64_t capacity, th_select_info *info)
{
    if (th_status s = select_checks(c, u, buffer, "th_select")) return s;
    TH_REQUIRE(info, "th_select: null info");
    if (th_status s = use(c, true)) return s;
    const uint32_t room = out ? (uint32_t)std::min<uint64_t>(capacity, c->texels()) : 0u;
    if (th_status s = select_storage(c, (uint32_t)((c->texels() + 63) / 64))) return s;
    SelectParams p = select_params(c, u, buffer, room);
    if (th_status s = select_scan(c, p)) return s;
    if (th_status s = read_back(c, info, c->select_info.get(), sizeof *info)) return s;      // the one wait: how many records there are
    const uint32_t written = (uint32_t)info->written;
    if (!written) return TH_OK;
    if (th_status s = select_records(c, written)) return s;
    p.records = c->select_records; p.capacity = written;
    if (th_status s = select_gather(c, p)) return s;
    return image_download(c, out, c->select_records.get(), (size_t)written * sizeof(th_selected));
}

}  // extern "C"
