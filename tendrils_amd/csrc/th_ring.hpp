// th_ring.hpp - what the built-in passes that read a ring buffer WHERE IT LIES share (th_measure.hip, th_density.hip, th_select.hip,
// th_histogram.hip, th_follow.hip): the device half first, then what their entry points do alike on the host.
#pragma once
#include "th_ctx.hpp"
#include "th_logic.hpp"          // th::unpack_state (th_packed.inc)

namespace thi {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// a slot as it lies in memory - 16 bytes, or the 8 of a packed ring -, one non-temporal load of it, and the state it holds;
// none(): what stands for a slot past the end - an inert particle
template <bool PACKED> struct Slot;
template <> struct Slot<false> {
    using Raw = v4f;
    TH_D static Raw load(const void *in, uint32_t idx) { return __builtin_nontemporal_load(static_cast<const Raw *>(in) + idx); }
    TH_D static Raw none() { return Raw{th::kInert, th::kInert, 0.0f, 0.0f}; }
    TH_D static v4f state(Raw t) { return t; }
};
template <> struct Slot<true> {
    using Raw = v2u;
    TH_D static Raw load(const void *in, uint32_t idx) { return __builtin_nontemporal_load(static_cast<const Raw *>(in) + idx); }
    TH_D static Raw none() { return Raw{0x80008000u, 0u}; }
    TH_D static v4f state(Raw t) { const float4 s = th::unpack_state(make_uint2(t.x, t.y)); return v4f{s.x, s.y, s.z, s.w}; }
};

TH_D bool slot_live(v4f s) { return !(s.x == th::kInert && s.y == th::kInert); }

// the sum over the wave, in every lane: EVERY lane of the wave must arrive
template <class T> TH_D T wave_sum(T v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }      // (uint32_t, unsigned long long)

// N per-lane counters (uint32_t, or unsigned long long) of a workgroup of 256 into info[WORD_k]: a butterfly per wave, lane 0 of
// each wave stores plain values into lds[wave * N + k] (4 * N words, nothing zeroed, no LDS atomic), one barrier, thread k < N
// adds the four and - if the sum is not zero - issues ONE global integer atomic.  EVERY lane of the workgroup must arrive.
// The words are template arguments: as an array argument indexed by the thread they became a private array, which the compiler
// moved into LDS (3 KiB in density's tally kernel); thread k selects its word among constants instead.
template <int... WORD, class T>
TH_D void fold_counters(T *lds, unsigned long long *info, const T (&lane)[sizeof...(WORD)])
{
    constexpr int N = sizeof...(WORD);
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T sum = wave_sum(lane[k]);
        if ((tid & 63u) == 0u) lds[(tid >> 6) * (uint32_t)N + (uint32_t)k] = sum;
    }
    __syncthreads();
    if (tid >= (uint32_t)N) return;
    uint32_t to = 0u, k = 0u;
    ((to = tid == k++ ? (uint32_t)WORD : to), ...);       // to = WORD_tid
    const T n = lds[tid] + lds[N + tid] + lds[2 * N + tid] + lds[3 * N + tid];
    if (n) atomicAdd(&info[to], (unsigned long long)n);
}

// Which member of a texel set (th_ctx.hpp: TexelSetView) local texel t is, in increasing texel - or kNoRank, above every rank (a
// set has at most 2^28 members), when it is none.  The caller has compared t against the texel count: word t >> 6 exists.
constexpr uint32_t kNoRank = 0xFFFFFFFFu;
TH_D uint32_t texel_rank(const TexelSetView &set, uint32_t t)
{
    const unsigned long long word = set.mask[t >> 6], bit = 1ull << (t & 63u);
    if (!(word & bit)) return kNoRank;                    // (nothing more is loaded for a texel outside the set)
    return set.counts[t >> 6] + (uint32_t)__popcll(word & (bit - 1ull));
}

// ring buffer `buffer` as a pass reads it: float4 or, packed, uint2 per slot, in place; the slot order stays (slot i holds local
// texel perm[i]; null: texel order).  order_out: which of c->orders that is (-1: texel order), for a caller that caches by it
struct RingView { const void *in; const uint32_t *perm; uint32_t count, width, row0; };      // ... this context's texels; the texture's width; the band's first row
inline RingView ring_read(const th_context *c, int32_t buffer, int *order_out = nullptr)
{
    const int order = order_of(c, c->ring[(size_t)buffer]);
    if (order_out) *order_out = order;
    return RingView{c->ring[(size_t)buffer], order >= 0 ? c->orders[(size_t)order].perm.get() : nullptr, (uint32_t)c->texels(), (uint32_t)c->cfg.width, (uint32_t)c->cfg.row0};
}

// what the entry points refuse alike, each under its own name
#define TH_RING_BUFFER_OK(c, buffer, entry) TH_REQUIRE((buffer) >= 0 && (size_t)(buffer) < (c)->ring.size(), "%s: buffer %d out of range (the ring has %zu)", entry, buffer, (c)->ring.size())
#define TH_RING_TEXELS_OK(c, entry) TH_REQUIRE((c)->texels() > 0 && (c)->texels() <= (1ull << 28), "%s: %zu particles", entry, (c)->texels())

// f(std::bool_constant<true>) on a packed ring, <false> on an f32 one: a kernel's instantiation is decltype(packed)::value
template <class F> void dispatch_packed(const th_context *c, F f) { if (c->packed) f(std::bool_constant<true>{}); else f(std::bool_constant<false>{}); }

}  // namespace thi
