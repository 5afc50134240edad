// th_follow.hip - follow: the states of a chosen set of particles, sample by sample, in a history kept on the device.  Measure
// programs, the density map, select and the histogram each look at one instant; this keeps the path of the SAME particles from
// frame to frame - an inspector, a plotter export, a trail overlay of a few thousand picked particles - for a set that a
// predicate no longer describes: it is given by its texel indices.  A built-in pass: fixed kernels, no hiprtc, no program kind.
//
// Fetching by index is free in texel order: slot = texel.  The frame loop lives in tile-sorted slots, and there is no inverse
// of perm; this unit keeps the small inverse that following a set needs - the slots of the followed texels only - and
// rebuilds it when, and only when, the sampled buffer's (order, SlotOrder::stamp) is another than the table's:
//   follow_mark_kernel     once per th_follow_set, between th_sort.hip's launch_texel_set_clear and launch_texel_set_rank: the
//                          set as a bit per LOCAL TEXEL (lane r ORs the bit of indices[r] - row0 * width: an integer atomic),
//                          then the words' popcounts and the exclusive scan over them.  The set is strictly increasing, so
//                          the rank of texel t in it is th_ring.hpp's texel_rank: select's ranking, no search.  A TexelSet
//                          of the context's own, not select's - select's device addresses stay valid until the next select.
//   follow_fill_kernel     0xFFFFFFFF into the slot table, then
//   follow_locate_kernel   one walk over perm on the streaming passes' grid, one non-temporal load a slot: t = perm[i] is
//                          compared against the texel count BEFORE it addresses the mask; a set bit gives slots[rank] = i.  No
//                          state is loaded.
//   follow_gather_kernel   lane r: one 4-byte load of its slot word - the table's entry, or over a buffer in texel order the
//                          set's own index less row0 * width: no table is filled there -, compared against the texel count
//                          first; one load of the slot (16 bytes, or the 8 of a packed ring, decoded); one 16-byte store into
//                          the history's row, contiguous across the wave.  A word out of range - perm is a permutation: it
//                          cannot happen - stores four 0x7FC00000 rather than reading anywhere.
// Only integer arithmetic and copies: the history's bits depend on neither the slot order nor the run.  No wave-wide
// operation anywhere: a lane past the end leaves.  Every index that addresses memory comes from a value compared in range first.
#include "th_ring.hpp"           // Slot<PACKED>, v4f, v4u, texel_rank, RingView: what the passes that read the ring where it lies share

using namespace thi;

namespace {

static_assert(sizeof(th_follow_info) == 48 && offsetof(th_follow_info, locates) == 40, "th_follow_info: the header's layout");
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kQuietNan = 0x7FC00000u;

// indices: whole-texture texels; base = row0 * width; count: this context's texels
__global__ __launch_bounds__(256) void follow_mark_kernel(const uint32_t *indices, uint32_t n, uint32_t base, uint32_t count, unsigned long long *mask)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) {
        const uint32_t t = indices[r] - base;                                   // (an index below the band wraps far past count)
        if (t < count) atomicOr(&mask[t >> 6], 1ull << (t & 63u));              // t < count: word t >> 6 < nwords
    }
}

__global__ __launch_bounds__(256) void follow_fill_kernel(uint32_t *slots, uint32_t n)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) slots[r] = kNoSlot;
}

// behind the rank: set.counts[] holds the members of the set before each word
__global__ __launch_bounds__(256) void follow_locate_kernel(const uint32_t *perm, uint32_t count, const TexelSetView set, uint32_t *slots, uint32_t n)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
        const uint32_t t = __builtin_nontemporal_load(perm + i);
        if (t >= count) continue;
        const uint32_t rank = texel_rank(set, t);
        if (rank < n) slots[rank] = i;                    // (kNoRank: not followed)
    }
}

// table[r] - base is the slot of member r: the slot table (base 0), or the set's indices (base = row0 * width) in texel order
template <bool PACKED>
__global__ __launch_bounds__(256) void follow_gather_kernel(const void *in, const uint32_t *table, uint32_t base, uint32_t count, uint32_t n, v4f *row)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t slot = table[r] - base;
    if (slot < count) {
        row[r] = Slot<PACKED>::state(Slot<PACKED>::load(in, slot));
    } else {
        const v4u nan = {kQuietNan, kQuietNan, kQuietNan, kQuietNan};
        *reinterpret_cast<v4u *>(row + r) = nan;
    }
}

uint32_t follow_base(const th_context *c) { return (uint32_t)c->cfg.row0 * (uint32_t)c->cfg.width; }

void follow_info(const th_context *c, th_follow_info *info)
{
    const auto &f = c->follow;
    info->particles = c->texels(); info->followed = f.n; info->depth = f.depth; info->samples = f.samples;
    info->held = std::min(f.samples, f.depth); info->locates = f.locates;
}

// ends following: what the stream still does with the history ends first
th_status follow_release(th_context *c)
{
    TH_HIP(hipStreamSynchronize(c->stream));
    c->follow_texels = {}; c->follow_set.reset(); c->follow_slots.reset(); c->follow_history.reset();
    c->follow = {};
    return TH_OK;
}

// the slots of the set in tile-sorted order `order`, found again when the table was built for another (order, stamp)
th_status follow_locate(th_context *c, int order)
{
    const th_context::SlotOrder &o = c->orders[(size_t)order];
    auto &f = c->follow;
    if (f.order == order && f.stamp == o.stamp) return TH_OK;
    const uint32_t count = (uint32_t)c->texels(), n = (uint32_t)f.n;
    hipLaunchKernelGGL(follow_fill_kernel, dim3(th::grid_for(n, 8)), dim3(256), 0, c->stream, c->follow_slots.get(), n);
    hipLaunchKernelGGL(follow_locate_kernel, dim3(th::grid_for(count, 8)), dim3(256), 0, c->stream, (const uint32_t *)o.perm.get(), count,
                       c->follow_texels.view(), c->follow_slots.get(), n);
    TH_HIP(hipGetLastError());
    f.order = order; f.stamp = o.stamp;
    ++f.locates;
    return TH_OK;
}

}  // namespace

extern "C" {

th_status th_follow_set(th_context *c, const uint32_t *indices, uint64_t n, uint32_t depth)
{
    TH_REQUIRE(c, "th_follow_set: null context");
    TH_RING_TEXELS_OK(c, "th_follow_set");
    if (n == 0) {
        if (th_status s = use(c, true)) return s;
        return follow_release(c);
    }
    TH_REQUIRE(indices, "th_follow_set: null indices with n = %llu", (unsigned long long)n);
    TH_REQUIRE(n <= TH_FOLLOW_MAX_PARTICLES, "th_follow_set: n = %llu (1 .. %u)", (unsigned long long)n, TH_FOLLOW_MAX_PARTICLES);
    TH_REQUIRE(depth >= 1u && depth <= TH_FOLLOW_MAX_DEPTH, "th_follow_set: depth = %u (1 .. %u)", depth, TH_FOLLOW_MAX_DEPTH);
    TH_REQUIRE(n * depth <= TH_FOLLOW_MAX_ENTRIES, "th_follow_set: n * depth = %llu (at most %u)", (unsigned long long)(n * depth), TH_FOLLOW_MAX_ENTRIES);
    const uint64_t base = (uint64_t)c->cfg.row0 * (uint64_t)c->cfg.width, end = base + c->texels();
    for (uint64_t i = 0; i < n; ++i) {
        TH_REQUIRE(indices[i] >= base && indices[i] < end, "th_follow_set: index %u at position %llu lies outside this context's rows (texels %llu .. %llu)",
                   indices[i], (unsigned long long)i, (unsigned long long)base, (unsigned long long)end - 1ull);
        TH_REQUIRE(i == 0 || indices[i] > indices[i - 1], "th_follow_set: index %u at position %llu is not above its predecessor %u", indices[i],
                   (unsigned long long)i, indices[i - 1]);
    }
    if (th_status s = use(c, true)) return s;             // read-only: the last draw's geometry and a fused launch's statistics stay valid
    TH_HIP(hipStreamSynchronize(c->stream));              // (a sample of the old set may still write the old history)
    const uint32_t count = (uint32_t)c->texels(), nwords = (count + 63u) / 64u, members = (uint32_t)n;
    // the new set's storage first: a failure leaves the old set as it was
    if (th_status s = c->follow_texels.reserve(nwords)) return s;      // (grow-only, and the texture's shape is the context's: an old set's is left as it is)
    DevBuf<uint32_t> set, slots;
    DevBuf<float4> history;
    if (th_status s = set.alloc(members)) return s;
    if (th_status s = slots.alloc(members)) return s;
    if (th_status s = history.alloc((size_t)members * depth)) return s;
    if (th_status s = image_upload(c, set.get(), indices, (size_t)members * sizeof(uint32_t))) return s;
    c->follow_set = std::move(set); c->follow_slots = std::move(slots); c->follow_history = std::move(history);
    c->follow = {};
    c->follow.n = n; c->follow.depth = depth;
    c->follow.times.assign(depth, 0.0);
    TH_HIP(hipMemsetAsync(c->follow_history, 0, c->follow_history.bytes(), c->stream));
    th::launch_texel_set_clear(c->follow_texels.mask, nwords, c->stream);
    hipLaunchKernelGGL(follow_mark_kernel, dim3(th::grid_for(members, 8)), dim3(256), 0, c->stream, (const uint32_t *)c->follow_set.get(), members,
                       follow_base(c), count, c->follow_texels.mask.get());
    th::launch_texel_set_rank(c->follow_texels.mask, c->follow_texels.counts, c->follow_texels.sums, nwords, false, c->stream);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

th_status th_follow_sample(th_context *c, int32_t buffer, double time)
{
    TH_REQUIRE(c, "th_follow_sample: null context");
    TH_RING_BUFFER_OK(c, buffer, "th_follow_sample");
    TH_REQUIRE(c->follow.n > 0, "th_follow_sample: no set is followed (th_follow_set)");
    if (th_status s = use(c, true)) return s;
    auto &f = c->follow;
    int order;
    const RingView ring = ring_read(c, buffer, &order);   // (the slot order stays: slot i holds texel perm[i])
    if (order >= 0) if (th_status s = follow_locate(c, order)) return s;
    const uint32_t *table = order >= 0 ? c->follow_slots.get() : c->follow_set.get();
    const uint32_t base = order >= 0 ? 0u : follow_base(c);
    const uint32_t n = (uint32_t)f.n;
    const size_t at = (size_t)(f.samples % f.depth);
    v4f *row = reinterpret_cast<v4f *>(c->follow_history.get() + at * (size_t)n);
    dispatch_packed(c, [&](auto packed) {
        hipLaunchKernelGGL(follow_gather_kernel<decltype(packed)::value>, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, ring.in, table, base, ring.count, n, row);
    });
    TH_HIP(hipGetLastError());
    f.times[at] = time;
    ++f.samples;
    return TH_OK;
}

th_status th_follow_read(th_context *c, uint64_t first, uint64_t count, float *states, double *times, th_follow_info *info)
{
    TH_REQUIRE(c, "th_follow_read: null context");
    TH_REQUIRE(info, "th_follow_read: null info");
    const auto &f = c->follow;
    TH_REQUIRE(f.n > 0, "th_follow_read: no set is followed (th_follow_set)");
    TH_REQUIRE(count == 0 || states, "th_follow_read: null states with count = %llu", (unsigned long long)count);
    const uint64_t held = std::min(f.samples, f.depth), oldest = f.samples - held;
    TH_REQUIRE(count == 0 || (first >= oldest && first <= f.samples && count <= f.samples - first),
               "th_follow_read: samples [%llu, %llu) asked, [%llu, %llu) are held", (unsigned long long)first, (unsigned long long)(first + count),
               (unsigned long long)oldest, (unsigned long long)f.samples);
    if (th_status s = use(c, true)) return s;
    TH_HIP(hipStreamSynchronize(c->stream));
    const size_t row_floats = (size_t)f.n * 4u, at = (size_t)(first % f.depth);
    const size_t head = (size_t)std::min<uint64_t>(count, f.depth - at), tail = (size_t)count - head;       // (the history wraps behind `head` rows)
    if (head) if (th_status s = image_download(c, states, c->follow_history.get() + at * (size_t)f.n, head * row_floats * sizeof(float))) return s;
    if (tail) if (th_status s = image_download(c, states + head * row_floats, c->follow_history.get(), tail * row_floats * sizeof(float))) return s;
    if (times) for (uint64_t k = 0; k < count; ++k) times[k] = f.times[(size_t)((first + k) % f.depth)];
    follow_info(c, info);
    return TH_OK;
}

th_status th_follow_query(th_context *c, th_follow_info *info, void **device_history, void **device_slots)
{
    TH_REQUIRE(c, "th_follow_query: null context");
    if (info) follow_info(c, info);
    if (device_history) *device_history = c->follow.n ? c->follow_history.get() : nullptr;
    if (device_slots) *device_slots = c->follow.n && c->follow.order >= 0 ? c->follow_slots.get() : nullptr;
    return TH_OK;
}

}  // extern "C"
