// th_histogram.hip - the histogram: the particles of one ring buffer that match a select predicate, counted per bin of one scalar
// of the state, the ring left where it lies.  Measure programs say numbers ABOUT the particles, the density map WHERE they are,
// select WHICH ones; this says how a quantity is DISTRIBUTED - and, through the key mode, the exact k-th order statistic by radix
// select (three passes over the monotone integer key of the float; the host narrows the prefix: Particles.quantiles).  A built-in
// pass: fixed kernels, no hiprtc, no program kind.
//
// Every accumulation is an INTEGER addition, so the result depends on neither the slot order, nor the order of arrival, nor the
// run: a tile-sorted ring, a packed ring's decoded texels and the same ring in texel order give the same bits.  Two kernels:
//   hist_clear_kernel   the `bins` counts and the info block: {particles, 0, 0, 0, 0, 0}
//   hist_tally_kernel   the ring where it lies: a workgroup takes blocks of 1024 slots, four non-temporal loads a lane in flight
//                       before anything is decoded (16 bytes a slot, 8 of a packed ring).  Over tile-sorted slots perm[i] is read
//                       ONLY when the stride clause needs the index: a bin does not depend on who the particle is.  The
//                       predicate is th_select's own (th_select_match.hpp).  A workgroup-private histogram in LDS (4 bytes a
//                       bin, sized by the call) takes the adds as LDS integer atomics; at the end the workgroup flushes its
//                       non-zero bins with global integer atomics, neighbouring lanes neighbouring bins.  live, matched, below,
//                       above and nan are per-lane integers: th_ring.hpp's fold of a workgroup's counters - a butterfly per
//                       wave, one global atomic per counter and workgroup.
// No lane leaves before the wave-wide operations: the loop's bounds are the workgroup's, a lane past the last slot carries "not
// live, no match".  Every index that addresses LDS or memory comes from a value compared in range first.  No float atomics.
#include "th_select_match.hpp"   // SelectClauses, select_match, select_checks: shared with th_select.hip; th_ring.hpp behind it

using namespace thi;

namespace {

constexpr uint32_t kLaneSlots = 4, kBlockSlots = 256u * kLaneSlots;   // slots a lane / a workgroup takes at a time
constexpr uint32_t kMaxGroups = 1024;     // four workgroups a CU: sixteen waves with four loads a lane in flight
constexpr uint32_t kNone = 0xffffffffu;   // "no bin": not matched, below, above, NaN
constexpr int kInfoWords = 6;             // th_histogram_info
enum { kParticles, kLive, kMatched, kBelow, kAbove, kNan };
constexpr uint32_t kTallyWords = 4 * 5;   // LDS: the four waves' five counters (fold_counters), then the workgroup's histogram
static_assert(sizeof(th_histogram_uniforms) == 72 && sizeof(th_histogram_info) == kInfoWords * 8, "th_histogram_*: the header's layout");
static_assert(offsetof(th_histogram_uniforms, channel) == 40 && offsetof(th_histogram_uniforms, reserved) == 68, "th_histogram_uniforms: select, then the rest");
static_assert(TH_HIST_MAX_BINS == 4096, "th_histogram: the scratch and the LDS are sized for 4096 bins");

struct HistParams {
    RingView ring;                    // the buffer where it lies; ring.perm is read only when the stride clause asks who a particle is
    SelectClauses q;                  // the predicate's clauses
    int32_t channel;
    uint32_t bins;
    float lo, hi, scale;              // TH_HIST_LINEAR: scale = (float)bins / (hi - lo)
    uint32_t prefix, top, shift;      // TH_HIST_KEY: prefix = (uint64)key_prefix >> top, top = shift + log2(bins)
    uint32_t *counts;                 // [bins]
    unsigned long long *info;         // [kInfoWords]
};

__global__ __launch_bounds__(256) void hist_clear_kernel(uint32_t *counts, uint32_t bins, unsigned long long *info, unsigned long long particles)
{
    for (uint32_t i = threadIdx.x; i < bins; i += 256u) counts[i] = 0u;
    if (threadIdx.x < (unsigned)kInfoWords) info[threadIdx.x] = threadIdx.x == kParticles ? particles : 0ull;
}

// the channel's value, in the header's words (the test is wave-uniform: the argument segment)
TH_D float hist_value(int32_t channel, v4f s)
{
    if (channel == TH_HIST_X) return s.x;
    if (channel == TH_HIST_Y) return s.y;
    if (channel == TH_HIST_VX) return s.z;
    if (channel == TH_HIST_VY) return s.w;
    const float q = (s.z * s.z) + (s.w * s.w);
    return channel == TH_HIST_SPEED2 ? q : __builtin_sqrtf(q);
}

// the bin of a matched particle's value - below p.bins -, or kNone and one of the three counters
template <int MODE>
TH_D uint32_t hist_bin(const HistParams &p, float v, uint32_t &below, uint32_t &above, uint32_t &nan)
{
    if (v != v) { ++nan; return kNone; }
    if (MODE == TH_HIST_LINEAR) {
        if (v < p.lo) { ++below; return kNone; }
        if (v >= p.hi) { ++above; return kNone; }
        const uint32_t b = (uint32_t)(int)__builtin_floorf((v - p.lo) * p.scale);      // lo <= v < hi: 0 <= b <= bins
        return b < p.bins ? b : p.bins - 1u;
    }
    const uint32_t u = __float_as_uint(v), key = (u >> 31) ? ~u : (u | 0x80000000u);
    const uint32_t head = (uint32_t)((unsigned long long)key >> p.top);
    if (head < p.prefix) { ++below; return kNone; }
    if (head > p.prefix) { ++above; return kNone; }
    return (uint32_t)((unsigned long long)key >> p.shift) & (p.bins - 1u);
}

template <bool PACKED, int MODE>
__global__ __launch_bounds__(256) void hist_tally_kernel(const HistParams p)
{
    extern __shared__ uint32_t lds[];           // kTallyWords counters, then p.bins bins
    uint32_t *tally = lds, *hist = lds + kTallyWords;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < p.bins; i += 256u) hist[i] = 0u;
    __syncthreads();
    uint32_t live = 0u, matched = 0u, below = 0u, above = 0u, nan = 0u;
    const bool indexed = p.ring.perm && p.q.stride > 1u;       // (wave-uniform: the argument segment)
    const uint32_t nblocks = (p.ring.count + kBlockSlots - 1u) / kBlockSlots;
    // `b` is the workgroup's: every lane of the workgroup takes the same turns
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint32_t base = b * kBlockSlots + tid;
        typename Slot<PACKED>::Raw raw[kLaneSlots];       // all of the lane's loads in flight before anything is decoded
        uint32_t t[kLaneSlots];
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) {
            const uint32_t idx = base + k * 256u;
            raw[k] = typename Slot<PACKED>::Raw{};
            t[k] = idx;
            if (idx < p.ring.count) {
                raw[k] = Slot<PACKED>::load(p.ring.in, idx);
                if (indexed) t[k] = __builtin_nontemporal_load(p.ring.perm + idx);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kLaneSlots; ++k) {
            const uint32_t idx = base + k * 256u;
            uint32_t bin = kNone;
            if (idx < p.ring.count) {
                const v4f s = Slot<PACKED>::state(raw[k]);
                const bool is_live = slot_live(s);
                live += is_live ? 1u : 0u;
                if (t[k] < p.ring.count && select_match(p.q, s, is_live, t[k])) {
                    ++matched;
                    bin = hist_bin<MODE>(p, hist_value(p.channel, s), below, above, nan);
                }
            }
            if (bin < p.bins) atomicAdd(&hist[bin], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < p.bins; i += 256u) {
        const uint32_t n = hist[i];
        if (n) atomicAdd(&p.counts[i], n);
    }
    fold_counters<kLive, kMatched, kBelow, kAbove, kNan>(tally, p.info, {live, matched, below, above, nan});      // every lane of the workgroup is here
}

th_status hist_checks(th_context *c, const th_histogram_uniforms *u, int32_t buffer, const char *entry)
{
    TH_REQUIRE(c, "%s: null context", entry);
    TH_REQUIRE(u, "%s: null uniforms", entry);
    if (th_status s = select_checks(c, &u->select, buffer, entry)) return s;
    TH_REQUIRE(u->channel >= TH_HIST_X && u->channel <= TH_HIST_SPEED, "%s: channel %d (TH_HIST_X .. TH_HIST_SPEED)", entry, u->channel);
    TH_REQUIRE(u->mode == TH_HIST_LINEAR || u->mode == TH_HIST_KEY, "%s: mode %d (TH_HIST_LINEAR or TH_HIST_KEY)", entry, u->mode);
    TH_REQUIRE(u->bins >= 1u && u->bins <= (uint32_t)TH_HIST_MAX_BINS, "%s: %u bins (1 .. %d)", entry, u->bins, TH_HIST_MAX_BINS);
    TH_REQUIRE(u->reserved == 0u, "%s: reserved is %u, not 0", entry, u->reserved);
    if (u->mode == TH_HIST_LINEAR) {
        TH_REQUIRE(std::isfinite(u->lo) && std::isfinite(u->hi) && u->lo < u->hi, "%s: the range %g .. %g (finite, lo < hi)", entry, (double)u->lo, (double)u->hi);
        const float width = u->hi - u->lo, scale = (float)u->bins / width;
        TH_REQUIRE(std::isfinite(width) && std::isfinite(scale), "%s: the range %g .. %g has no finite width or scale", entry, (double)u->lo, (double)u->hi);
    } else {
        TH_REQUIRE(is_pow2(u->bins), "%s: %u bins (TH_HIST_KEY: a power of two)", entry, u->bins);
        TH_REQUIRE(u->key_shift <= 32u && u->key_shift + ilog2(u->bins) <= 32u, "%s: key_shift %u and %u bins reach past bit 32", entry, u->key_shift, u->bins);
    }
    return TH_OK;
}

// the checks, the scratch, the two kernels: enqueued, nothing more
th_status hist_enqueue(th_context *c, const th_histogram_uniforms *u, int32_t buffer, const char *entry)
{
    if (th_status s = hist_checks(c, u, buffer, entry)) return s;
    if (th_status s = use(c, true)) return s;             // read-only: the last draw's geometry and a fused launch's statistics stay valid
    if (!c->hist_info) if (th_status s = c->hist_info.alloc(kInfoWords)) return s;
    if (!c->hist_counts) if (th_status s = c->hist_counts.alloc(TH_HIST_MAX_BINS)) return s;
    HistParams p{};
    p.ring = ring_read(c, buffer);
    p.q = select_clauses(c, &u->select);
    p.channel = u->channel; p.bins = u->bins;
    if (u->mode == TH_HIST_LINEAR) {
        p.lo = u->lo; p.hi = u->hi;
        p.scale = (float)u->bins / (u->hi - u->lo);
    } else {
        p.shift = u->key_shift; p.top = u->key_shift + ilog2(u->bins);
        p.prefix = (uint32_t)((unsigned long long)u->key_prefix >> p.top);
    }
    p.counts = c->hist_counts; p.info = c->hist_info;
    hipLaunchKernelGGL(hist_clear_kernel, dim3(1), dim3(256), 0, c->stream, p.counts, p.bins, p.info, (unsigned long long)c->texels());
    const uint32_t nblocks = (p.ring.count + kBlockSlots - 1u) / kBlockSlots, grid = std::min(nblocks, kMaxGroups);
    dispatch_packed(c, [&](auto packed) {
        constexpr bool P = decltype(packed)::value;
        hipLaunchKernelGGL((u->mode == TH_HIST_LINEAR ? hist_tally_kernel<P, TH_HIST_LINEAR> : hist_tally_kernel<P, TH_HIST_KEY>), dim3(grid), dim3(256),
                           (kTallyWords + p.bins) * sizeof(uint32_t), c->stream, p);
    });
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // namespace

extern "C" {

th_status th_histogram_async(th_context *c, const th_histogram_uniforms *u, int32_t buffer, void **device_counts, void **device_info)
{
    if (th_status s = hist_enqueue(c, u, buffer, "th_histogram_async")) return s;
    if (device_counts) *device_counts = c->hist_counts.get();
    if (device_info) *device_info = c->hist_info.get();
    return TH_OK;
}

th_status th_histogram(th_context *c, const th_histogram_uniforms *u, int32_t buffer, uint32_t *counts, th_histogram_info *info)
{
    TH_REQUIRE(c, "th_histogram: null context");
    TH_REQUIRE(info, "th_histogram: null info");
    if (th_status s = hist_enqueue(c, u, buffer, "th_histogram")) return s;
    // the counts go out in front of the info block, whose read-back is the call's one wait
    if (counts) TH_HIP(hipMemcpyAsync(counts, c->hist_counts.get(), (size_t)u->bins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return read_back(c, info, c->hist_info.get(), sizeof *info);
}

}  // extern "C"
