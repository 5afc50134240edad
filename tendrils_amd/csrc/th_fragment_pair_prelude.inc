R"TH_PRELUDE(// th_fragment_pair_prelude.inc - what th_fragment_program_compile puts behind th_fragment_prelude.inc (th_fragprog.hip embeds
// this file as text, like that one): the two entry points of a stage that runs in th_draw_stages_pair's ONE rasterisation of
// both passes of draw().  There every fragment carries the flow pass's varying and the view pass's colour side by side:
// colors[2 * at] and colors[2 * at + 1] belong to the fragment at keys[at] (th_deposit.hip: dep_put, th_bins.hip: bins_put, mode
// 2), and each target is blended from its half.  A stage is the fragment shader of ONE pass: it runs over its pass's half `half`
// (0: flow, 1: view) of every pair and leaves the other half alone; two stages are two launches, the flow pass's first.  The
// record's pass, the target's shape and the uniform block are the half's own; the flow field and the colour map are the
// context's as they were before the call - nothing has blended yet - so a VIEW stage that names th_flow, which after a flow pass
// would read what that pass left, never comes here (th_draw_stages_pair then runs the two passes one after the other).  Nor does a
// program that reads th_line: f.line is null.  The lane bodies and both walks are th_fragment_prelude.inc's - they take the
// varying's address apart from the key.
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

// th_fragment_kernel's harness (th_fragment_stream; total < 2^31, so 2 * at + 1 < 2^32).  A lane reads its key and its half - ONE
// 16-byte load - and writes that half back - ONE 16-byte store: a wave touches every other 16 bytes of 2 KiB.  Nothing is written
// but colors[2 * at + half], at < total.
extern "C" __global__ __launch_bounds__(256) void th_fragment_pair_kernel(const th_fragment_pair_args a, const th_program_uniform_block u)
{
    th_fragment_stream<unsigned, false, true>(a.f, u, nullptr, a.half & 1u);
}

// th_fragment_bins_kernel's walk over the page store of a binned pass: the varyings of place `at` are colors[2 * at] and
// colors[2 * at + 1].  The store holds up to 2^32 places, so 2 * at need not fit 32 bits: the index is 64-bit.
extern "C" __global__ __launch_bounds__(256) void th_fragment_pair_bins_kernel(const th_fragment_pair_bins_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.b.f, u);
    const size_t half = a.half & 1u;
    th_bins_walk(th_fragment_store_of(a.b), [&](unsigned long long key, unsigned at) { th_fragment_place(f, key, a.b.f.colors + (2 * (size_t)at + half)); });
}
)TH_PRELUDE"
