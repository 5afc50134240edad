R"TH_PRELUDE(// th_fragment_prelude.inc - what th_fragment_program_compile puts in front of a fragment program, after the text of
// th_taps.inc and th_bins_walk.inc (th_fragprog.hip embeds this file as text: the first and the last line make it one raw string literal).
// Self-contained: no project header, only what hiprtc's built-in headers give.  Compiled with the product's arithmetic flags
// (-ffp-contract=off: a*b+c stays two rounded fp32 operations, as in the reference's shaders).
//
// A fragment program defines ONE device function,
//     __device__ float4 th_fragment_main(const th_fragment_pass &f);
// main() of the fragment shader of one pass of draw() (the second of renderShader: [vert, frag] / flowShader: [vert, frag]): it
// is called once per fragment the pass's lines cover and returns gl_FragColor, which the library blends into the target in
// primitive order (SRC_ALPHA / ONE_MINUS_SRC_ALPHA) as it blends the varying of a pass without this stage.  There is no
// destination texel to read (GL has none either), no `discard` and nothing of the particles: a source that names th_particles
// does not compile.  Of the line the fragment belongs to it sees th_line(f), below.  A fragment that wants to leave its texel alone returns
// alpha 0 WITH FINITE COLOUR: the blend is dst = src * a + dst * (1 - a), and 0 * inf or 0 * NaN is NaN.
//
// th_fragment_args is the launch record th_fragprog.hip fills (same layout there; the static_asserts pin the sizes).
#define TH_PASS_FLOW 0
#define TH_PASS_VIEW 1
struct th_fragment_args {
    const void *keys;            // per fragment: th_fragment_kernel - 32-bit texel keys; th_fragment_band_kernel - 64-bit
                                 // owner << 56 | texel << 32 | stream index
    float4 *colors;              // per fragment, in the keys' order: the varying in, gl_FragColor out
    const float4 *flow;          // fw x fh, as it was before this pass
    const float4 *colormap;      // cw x ch (null: none is held)
    unsigned total;              // fragments of the pass
    int fw, fh, cw, ch;          // (the target, flow field or view image, is fw x fh)
    int pass;
    unsigned div_mul, div_shift; // texel / fw for every texel < 2^32: m = floor(2^32 (2^l - fw) / fw) + 1 with l = ceil(log2 fw),
                                 // t = mulhi(m, n), q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0); div_shift = sh1 | sh2 << 8
};
static_assert(sizeof(th_fragment_args) == 64, "th_fragment_args: layout shared with th_fragprog.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_fragment_pass {
    unsigned x, y;               // the window texel of the target: column, row (row 0 is the target's first row)
    float2 coord;                // gl_FragCoord.xy: (x + 0.5, y + 0.5)
    float2 viewRes;              // the target's width and height
    float4 color;                // the varying, as the library interpolated it along the line's snapped endpoints
    int pass;                    // TH_PASS_FLOW | TH_PASS_VIEW
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(f))
    const th_fragment_args *args;
    const struct th_fragment_line *line;      // th_line(f); null in the entry points of a program that does not read it
};

// The fragment's line, as the library's raster stage has it (th_fragline.hip writes one record per fragment for a pass whose
// program names th_line; a program that does not pays nothing and launches what it always did):
struct __attribute__((aligned(16))) th_fragment_line {
    unsigned line;               // stream index of the fragment's line: column * H + row of the WHOLE particle texture (GL's
                                 // primitive index; the low word of the band and bin keys)
    float along;                 // the parameter the library mixed `color` with: 0 at the line's first vertex (the previous
                                 // state), 1 at its second, unclamped outside them; 0 when both endpoints snap to one point
    float across;                // signed distance of the texel centre from the line through the SNAPPED endpoints, in texels:
                                 // positive to the left of first -> second vertex, with y as the target's rows count
    float length;                // distance between the snapped endpoints, in texels
};
static_assert(sizeof(th_fragment_line) == 16, "th_fragment_line: layout shared with th_fragline.hip");
static __device__ const th_fragment_line th_fragment_no_line = {0u, 0.0f, 0.0f, 0.0f};
__device__ __forceinline__ const th_fragment_line &th_line(const th_fragment_pass &f) { return f.line ? *f.line : th_fragment_no_line; }

__device__ float4 th_fragment_main(const th_fragment_pass &f);

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_fragment_pass &f)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(f.uniforms);
}

// texture2D(flow, (u, v)) / texture2D(colorMap, (u, v)): NEAREST, CLAMP_TO_EDGE, always inside the texture (th_taps.inc).  The
// flow is the field as it was BEFORE this pass, also in a pass that draws into it: every fragment has run before anything blends.
__device__ __forceinline__ float4 th_flow(const th_fragment_pass &f, float u, float v)
{
    const th_fragment_args &a = *f.args;
    return a.flow[(size_t)th_tap_nearest(v, a.fh) * a.fw + th_tap_nearest(u, a.fw)];
}
__device__ __forceinline__ float2 th_flow_res(const th_fragment_pass &f) { return make_float2((float)f.args->fw, (float)f.args->fh); }
// no colour map held: the 1 x 1 zero texture, as the built-in view stage reads it
__device__ __forceinline__ float4 th_colormap(const th_fragment_pass &f, float u, float v)
{
    const th_fragment_args &a = *f.args;
    if (!a.colormap) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return a.colormap[(size_t)th_tap_nearest(v, a.ch) * a.cw + th_tap_nearest(u, a.cw)];
}
__device__ __forceinline__ float2 th_colormap_res(const th_fragment_pass &f)
{
    const th_fragment_args &a = *f.args;
    return a.colormap ? make_float2((float)a.cw, (float)a.ch) : make_float2(1.0f, 1.0f);
}

// One fragment at window texel (x, y): ONE 16-byte load of *color, the program, ONE 16-byte store back.
typedef float th_float4_load __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void th_fragment_shade(th_fragment_pass &f, unsigned x, unsigned y, float4 *color)
{
    f.x = x; f.y = y;
    f.coord = make_float2((float)x + 0.5f, (float)y + 0.5f);
    th_float4_load *slot = reinterpret_cast<th_float4_load *>(color);
    const th_float4_load c = *slot;
    f.color = make_float4(c.x, c.y, c.z, c.w);
    const float4 o = th_fragment_main(f);
    th_float4_load out;
    out.x = o.x; out.y = o.y; out.z = o.z; out.w = o.w;
    *slot = out;
}
// ... under a texel key: split into (x, y) with the record's multiplier (five integer operations, no division)
__device__ __forceinline__ void th_fragment_lane(th_fragment_pass &f, const th_fragment_args &a, unsigned texel, float4 *color)
{
    const unsigned t = __umulhi(a.div_mul, texel);
    const unsigned y = (t + ((texel - t) >> (a.div_shift & 0xffu))) >> (a.div_shift >> 8);
    th_fragment_shade(f, texel - y * (unsigned)a.fw, y, color);
}
// ... under a key of the page store: x and y are its two 12-bit fields
__device__ __forceinline__ void th_fragment_place(th_fragment_pass &f, unsigned long long key, float4 *color)
{
    th_fragment_shade(f, (unsigned)(key >> 32) & 0xfffu, (unsigned)(key >> 44) & 0xfffu, color);
}
__device__ __forceinline__ th_fragment_pass th_fragment_pass_of(const th_fragment_args &a, const th_program_uniform_block &u)
{
    th_fragment_pass f;
    f.viewRes = make_float2((float)a.fw, (float)a.fh);
    f.pass = a.pass;
    f.uniforms = u.bytes;
    f.args = &a;
    f.line = nullptr;
    return f;
}

// The harness of the stream-ordered entry points: one lane per fragment of the pass, 256-thread workgroups, grid-stride
// (total < 2^31).  Key: 32-bit texel keys, or the 64-bit keys of an emit (th_draw_stages_emit) - owner << 56 | texel << 32 | stream
// index, the texel of the WHOLE target whatever rows of the particle texture the context holds.  LINES: lines[at] belongs to the
// fragment at keys[at]; a lane loads its 16-byte record once, beside its varying.  PAIR: two varyings a fragment
// (th_fragment_pair_prelude.inc), this stage's at colors[2 * at + half]; otherwise colors[at].  A wave reads its keys and its
// varyings, contiguous, and writes the varyings back where it read them; the record is the kernel's argument (scalar loads).
// No LDS, no atomics; nothing is written but the lane's varying.
template <class Key, bool LINES, bool PAIR>
__device__ __forceinline__ void th_fragment_stream(const th_fragment_args &a, const th_program_uniform_block &u, const th_fragment_line *lines, unsigned half)
{
    th_fragment_pass f = th_fragment_pass_of(a, u);
    const Key *keys = static_cast<const Key *>(a.keys);
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.total; at += gridDim.x * 256u) {
        th_fragment_line line;
        if constexpr (LINES) { line = lines[at]; f.line = &line; }
        unsigned texel;
        if constexpr (sizeof(Key) == 8) texel = (unsigned)(keys[at] >> 32) & 0xffffffu;
        else texel = keys[at];
        th_fragment_lane(f, a, texel, a.colors + (PAIR ? 2u * at + half : at));
    }
}

// An entry point per key width and no switch in one kernel: each loop loads keys of one width, and neither carries the other's
// registers.
extern "C" __global__ __launch_bounds__(256) void th_fragment_kernel(const th_fragment_args a, const th_program_uniform_block u)
{
    th_fragment_stream<unsigned, false, false>(a, u, nullptr, 0u);
}

extern "C" __global__ __launch_bounds__(256) void th_fragment_band_kernel(const th_fragment_args a, const th_program_uniform_block u)
{
    th_fragment_stream<unsigned long long, false, false>(a, u, nullptr, 0u);
}

// ---- the two entry points of a program that reads the fragment's line (th_line) -------------------------------------------------
// A record of its own (th_fragprog.hip: the same layout): the other entry points keep theirs.
struct th_fragment_line_args {
    th_fragment_args f;
    const th_fragment_line *lines;   // per fragment, in the keys' order
};
static_assert(sizeof(th_fragment_line_args) == 72, "th_fragment_line_args: layout shared with th_fragprog.hip");

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_kernel(const th_fragment_line_args a, const th_program_uniform_block u)
{
    th_fragment_stream<unsigned, true, false>(a.f, u, a.lines, 0u);
}

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_band_kernel(const th_fragment_line_args a, const th_program_uniform_block u)
{
    th_fragment_stream<unsigned long long, true, false>(a.f, u, a.lines, 0u);
}

// ---- the same stage over the fragments of a BINNED pass (th_bins.hip), where they lie in its page store -----------------------
// The walk is th_bins_walk (th_bins_walk.inc, whose text stands in front of this one): a place's key in keys[place], its varying
// in colors[place] - where the ordinary bins' blend, the crowd's regroup and the long and giant runs all fetch it later.  Nothing
// is written but colors[place] of live places.  The record is th_fragprog.hip's, the same layout.
struct th_fragment_bins_args {
    th_fragment_args f;              // keys: the store's 64-bit keys; colors: its varyings; total, div_mul, div_shift: unused (0)
    const unsigned *bin_cursor;      // the lists' cursors
    const unsigned *page_table;      // per list max_pages entries
    const unsigned *totals;          // the pass's totals
    unsigned bin_stride, max_pages, nbins;
    unsigned pages;                  // pages of the store: every page id is below it
    unsigned replicas, page_shift;   // th_bins_replicas, th_bins_page_shift (the library fills them from the constants this text was built with)
};
static_assert(sizeof(th_fragment_bins_args) == 112, "th_fragment_bins_args: layout shared with th_fragprog.hip");
__device__ __forceinline__ th_bins_store th_fragment_store_of(const th_fragment_bins_args &a)
{
    return th_bins_store{static_cast<const unsigned long long *>(a.f.keys), a.bin_cursor, a.page_table, a.totals, a.bin_stride, a.max_pages, a.nbins, a.pages};
}

extern "C" __global__ __launch_bounds__(256) void th_fragment_bins_kernel(const th_fragment_bins_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.f, u);
    th_bins_walk(th_fragment_store_of(a), [&](unsigned long long key, unsigned at) { th_fragment_place(f, key, a.f.colors + at); });
}

// ---- ... and of a program that reads the fragment's line, over the same store (TH_OPT_LINE_BINS) -------------------------------
// lines[at] belongs to the fragment at place `at` (th_fragline.hip writes it from the place's key and the line's snapped
// endpoints: line_record's numbers, as in a stream-ordered pass).  A record of its own (th_fragprog.hip: the same layout); a lane
// loads its 16-byte record once, beside its varying - as th_fragment_line_kernel does.
struct th_fragment_line_bins_args {
    th_fragment_bins_args b;
    const th_fragment_line *lines;   // per place of the store
};
static_assert(sizeof(th_fragment_line_bins_args) == 120, "th_fragment_line_bins_args: layout shared with th_fragprog.hip");

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_bins_kernel(const th_fragment_line_bins_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.b.f, u);
    th_bins_walk(th_fragment_store_of(a.b), [&](unsigned long long key, unsigned at) {
        const th_fragment_line line = a.lines[at];
        f.line = &line;
        th_fragment_place(f, key, a.b.f.colors + at);
    });
}
)TH_PRELUDE"
