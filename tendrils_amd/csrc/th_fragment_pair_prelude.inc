R"TH_PRELUDE(// th_fragment_pair_prelude.inc - what th_fragment_program_compile puts behind th_fragment_prelude.inc (th_fragprog.hip embeds
// this file as text, like that one): the two entry points of a stage that runs in th_draw_stages_pair's ONE rasterisation of
// both passes of draw().  There every fragment carries the flow pass's varying and the view pass's colour side by side:
// colors[2 * at] and colors[2 * at + 1] belong to the fragment at keys[at] (th_deposit.hip: dep_put, th_bins.hip: bins_put, mode
// 2), and each target is blended from its half.  A stage is the fragment shader of ONE pass: it runs over its pass's half `half`
// (0: flow, 1: view) of every pair and leaves the other half alone; two stages are two launches, the flow pass's first.  The
// record's pass, the target's shape and the uniform block are the half's own; the flow field and the colour map are the
// context's as they were before the call - nothing has blended yet - so a VIEW stage that names th_flow, which after a flow pass
// would read what that pass left, never comes here (th_draw_stages_pair then runs the two passes one after the other).  Nor does a
// program that reads th_line: f.line is null.  The lane bodies are th_fragment_prelude.inc's - they take the colour index apart
// from the key index.
struct th_fragment_pair_args {
    th_fragment_args f;              // keys: 32-bit texel keys, one a fragment; colors: TWO varyings a fragment
    unsigned half;                   // 0 | 1: which of a fragment's two varyings is this stage's
};
static_assert(sizeof(th_fragment_pair_args) == 72, "th_fragment_pair_args: layout shared with th_fragprog.hip");
struct th_fragment_pair_bins_args {
    th_fragment_bins_args b;         // colors: TWO varyings a place of the store
    unsigned half;
};
static_assert(sizeof(th_fragment_pair_bins_args) == 120, "th_fragment_pair_bins_args: layout shared with th_fragprog.hip");

// th_fragment_kernel's walk: one lane per fragment, grid-stride (total < 2^31, so 2 * at + 1 < 2^32).  A lane reads its key and
// its half - ONE 16-byte load - and writes that half back - ONE 16-byte store: a wave touches every other 16 bytes of 2 KiB.
// No LDS, no atomics; nothing is written but colors[2 * at + half], at < total.
extern "C" __global__ __launch_bounds__(256) void th_fragment_pair_kernel(const th_fragment_pair_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.f, u);
    const unsigned *keys = static_cast<const unsigned *>(a.f.keys);
    const unsigned half = a.half & 1u;
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.f.total; at += gridDim.x * 256u)
        th_fragment_lane(f, a.f, keys[at], 2u * at + half);
}

// th_fragment_bins_kernel's walk over the page store of a binned pass, the same skips: the varyings of place `at` are
// colors[2 * at] and colors[2 * at + 1].  The store holds up to 2^32 places, so 2 * at need not fit 32 bits: the lane body is
// handed the record with `colors` moved on by `at + half` texels and indexes it with `at` again.
extern "C" __global__ __launch_bounds__(256) void th_fragment_pair_bins_kernel(const th_fragment_pair_bins_args a, const th_program_uniform_block u)
{
    if (a.b.replicas != TH_BIN_REPLICAS || a.b.page_shift != TH_BIN_PAGE_SHIFT) return;
    if (a.b.totals[TH_BINS_TOT_FLAGS] != 0u || a.b.totals[TH_BINS_TOT_OOB] != 0u) return;
    const unsigned b = blockIdx.x;
    if (b >= a.b.nbins) return;
    const unsigned list_cap = a.b.max_pages << TH_BIN_PAGE_SHIFT;
    const unsigned *cursor = a.b.bin_cursor + (size_t)(b & 31u) * ((a.b.nbins + 31u) >> 5) + (b >> 5);
    unsigned first[TH_BIN_REPLICAS + 1u];
    first[0] = 0u;
#pragma unroll
    for (unsigned r = 0; r < TH_BIN_REPLICAS; ++r) {
        const unsigned n = cursor[(size_t)r * a.b.bin_stride];
        first[r + 1u] = first[r] + (n < list_cap ? n : list_cap);
    }
    const unsigned n = first[TH_BIN_REPLICAS], rounds = (n + 255u) >> 8;
    if (blockIdx.y >= rounds) return;
    th_fragment_pass f = th_fragment_pass_of(a.b.f, u);
    const unsigned long long *keys = static_cast<const unsigned long long *>(a.b.f.keys);
    const size_t half = a.half & 1u;
    th_fragment_args moved = a.b.f;
    for (unsigned round = blockIdx.y; round < rounds; round += gridDim.y) {
        const unsigned w = (round << 8) + threadIdx.x;
        if (w >= n) continue;
        unsigned r = 0u, base = 0u;
#pragma unroll
        for (unsigned q = 1; q < TH_BIN_REPLICAS; ++q) if (w >= first[q]) { r = q; base = first[q]; }
        const unsigned list = b * TH_BIN_REPLICAS + r, v = w - base, pn = v >> TH_BIN_PAGE_SHIFT;
        unsigned id = list;
        if (pn != 0u) {
            if (pn >= a.b.max_pages) continue;
            id = a.b.page_table[(size_t)list * a.b.max_pages + pn];
            if (id == 0u) continue;
        }
        if (id >= a.b.pages) continue;                   // (0xffffffff among them)
        const unsigned at = (id << TH_BIN_PAGE_SHIFT) | (v & ((1u << TH_BIN_PAGE_SHIFT) - 1u));
        const unsigned long long key = keys[at];
        if (key == ~0ull) continue;
        moved.colors = a.b.f.colors + ((size_t)at + half);
        th_fragment_place(f, moved, key, at);
    }
}
)TH_PRELUDE"
