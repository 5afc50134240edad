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
//                          lane ORs its bit in (an integer atomic).  The live particles: per lane, th_ring.hpp's fold of a
//                          workgroup's counters - a butterfly per wave, one integer atomic per workgroup.
//   (rank)                 th_sort.hip's launch_texel_set_rank: the words' popcounts - over tile-sorted slots only - and the
//                          exclusive scan over them, as it is; select_total_kernel leaves matched = offsets[last] +
//                          popcount(mask[last]) and written = min(matched, capacity) in the info block
//   select_gather_kernel   the slots again: a particle's bit is read from the MASK - the predicate is evaluated in one place
//                          only -, its rank is th_ring.hpp's texel_rank, and below `capacity` the slot is loaded and two
//                          16-byte stores leave its record.  A slot whose bit is clear is not loaded.
// Why the bits are indexed by texel and not by slot: the records come in increasing texel, and there is no inverse of perm to
// walk a slot-indexed mask in that order; with texel-indexed bits the rank of a particle is a popcount below its own bit,
// whatever slot holds it.  The price is the second walk over the slots (and, tile-sorted, the atomics).
// No lane leaves the mark kernel before its wave-wide operations: the loop's bound is the workgroup's, a lane past the last
// slot carries "no match, not live".  Every index that addresses memory comes from a value compared in range first.
#include "th_select_match.hpp"   // SelectClauses, select_match, select_checks: shared with th_histogram.hip; th_ring.hpp behind it

using namespace thi;

namespace {

constexpr int kInfoWords = 4;             // th_select_info
enum { kParticles, kLive, kMatched, kWritten };
static_assert(sizeof(th_select_uniforms) == 40 && sizeof(th_selected) == 32 && sizeof(th_select_info) == kInfoWords * 8, "th_select_*: the header's layout");
static_assert(offsetof(th_selected, index) == 16, "th_selected: the state, then index, x, y, reserved");

struct SelectParams {
    RingView ring;                    // the buffer where it lies; ring.perm null: texel order
    uint32_t nwords;                  // mask words: (ring.count + 63) / 64
    SelectClauses q;                  // the predicate's clauses
    uint32_t capacity;                // records the gather may write
    unsigned long long *mask;         // [nwords]: bit t & 63 of word t >> 6 is local texel t
    uint32_t *counts;                 // [nwords]: the words' popcounts, then (scanned in place) the matches before each word
    unsigned long long *info;         // [kInfoWords]
    th_selected *records;
};

// {0, 0, 0, 0} into the info block and, over tile-sorted slots, zero into the mask (here, not by launch_texel_set_clear: one launch less)
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
    for (uint32_t base = blockIdx.x * 256u; base < p.ring.count; base += gridDim.x * 256u) {
        const uint32_t idx = base + tid;
        bool live = false, match = false;
        uint32_t t = idx;
        if (idx < p.ring.count) {
            const v4f s = Slot<PACKED>::state(Slot<PACKED>::load(p.ring.in, idx));
            if (p.ring.perm) t = __builtin_nontemporal_load(p.ring.perm + idx);          // (wave-uniform test: the argument segment)
            live = slot_live(s);
            match = t < p.ring.count && select_match(p.q, s, live, t);
        }
        live_n += live ? 1u : 0u;
        if (!p.ring.perm) {
            const unsigned long long word = __ballot(match);                    // every lane of the wave is here
            const uint32_t w = idx >> 6;
            if ((tid & 63u) == 0u && w < p.nwords) { p.mask[w] = word; p.counts[w] = (uint32_t)__popcll(word); }
        } else if (match) {
            atomicOr(&p.mask[t >> 6], 1ull << (t & 63u));                       // t < count: word t >> 6 < nwords
        }
    }
    fold_counters<kLive>(part, p.info, {live_n});                          // every lane of the workgroup is here
}

// behind the scan: counts[] holds the matches before each word
__global__ void select_total_kernel(const SelectParams p)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long matched = (unsigned long long)p.counts[p.nwords - 1u] + (unsigned long long)__popcll(p.mask[p.nwords - 1u]);
    p.info[kParticles] = p.ring.count;
    p.info[kMatched] = matched;
    p.info[kWritten] = matched < p.capacity ? matched : (unsigned long long)p.capacity;
}

template <bool PACKED>
__global__ __launch_bounds__(256) void select_gather_kernel(const SelectParams p)
{
    const TexelSetView set{p.mask, p.counts};
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < p.ring.count; idx += gridDim.x * 256u) {
        const uint32_t t = p.ring.perm ? __builtin_nontemporal_load(p.ring.perm + idx) : idx;
        if (t >= p.ring.count) continue;
        const uint32_t rank = texel_rank(set, t);
        if (rank >= p.capacity) continue;                 // (kNoRank: its bit is clear)
        const v4f s = Slot<PACKED>::state(Slot<PACKED>::load(p.ring.in, idx));
        const uint32_t row = t / p.ring.width;
        const v4u who = {t + p.ring.row0 * p.ring.width, t - row * p.ring.width, row + p.ring.row0, 0u};
        v4f *rec = reinterpret_cast<v4f *>(p.records + rank);
        rec[0] = s;
        *reinterpret_cast<v4u *>(rec + 1) = who;
    }
}

// `capacity` records of room; an earlier select's gather may still write the old ones
th_status select_records(th_context *c, uint32_t capacity)
{
    if (c->select_records.size() >= capacity) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    return c->select_records.alloc(capacity);
}

// the call's parameters, over the context's scratch: reserved by its first select (the texture's shape is the context's: only the records ever grow)
th_status select_params(th_context *c, const th_select_uniforms *u, int32_t buffer, uint32_t capacity, SelectParams &p)
{
    p = SelectParams{};
    p.ring = ring_read(c, buffer);
    p.nwords = (p.ring.count + 63u) / 64u;
    if (!c->select_info) if (th_status s = c->select_info.alloc(kInfoWords)) return s;
    if (th_status s = c->select_set.reserve(p.nwords)) return s;
    p.q = select_clauses(c, u);
    p.capacity = capacity;
    p.mask = c->select_set.mask; p.counts = c->select_set.counts; p.info = c->select_info;
    p.records = c->select_records;
    return TH_OK;
}

// clear, mark, rank, total: enqueued, nothing more.  The info block is complete behind them (written = min(matched, capacity))
th_status select_scan(th_context *c, const SelectParams &p)
{
    const int grid = th::grid_for(p.ring.count, 8);
    hipLaunchKernelGGL(select_clear_kernel, dim3(th::grid_for(p.ring.perm ? p.nwords : 1u, 8)), dim3(256), 0, c->stream, p.mask, p.ring.perm ? p.nwords : 0u, p.info);
    dispatch_packed(c, [&](auto packed) { hipLaunchKernelGGL(select_mark_kernel<decltype(packed)::value>, dim3(grid), dim3(256), 0, c->stream, p); });
    th::launch_texel_set_rank(p.mask, p.counts, c->select_set.sums, p.nwords, !p.ring.perm, c->stream);      // (texel order: the mark kernel left the popcounts)
    hipLaunchKernelGGL(select_total_kernel, dim3(1), dim3(64), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

th_status select_gather(th_context *c, const SelectParams &p)
{
    dispatch_packed(c, [&](auto packed) { hipLaunchKernelGGL(select_gather_kernel<decltype(packed)::value>, dim3(th::grid_for(p.ring.count, 8)), dim3(256), 0, c->stream, p); });
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
    if (th_status s = select_records(c, room)) return s;
    SelectParams p;
    if (th_status s = select_params(c, u, buffer, room, p)) return s;
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
    SelectParams p;
    if (th_status s = select_params(c, u, buffer, room, p)) return s;
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
