R"TH_PRELUDE(// th_fragment_prelude.inc - what th_fragment_program_compile puts in front of a fragment program, after the text of
// th_taps.inc (th_fragprog.hip embeds this file as text: the first and the last line make it one raw string literal).
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

// One fragment: its texel split into (x, y) with the record's multiplier (five integer operations, no division), ONE 16-byte
// load of colors[at], the program, ONE 16-byte store back.
typedef float th_float4_load __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void th_fragment_lane(th_fragment_pass &f, const th_fragment_args &a, unsigned texel, unsigned at)
{
    const unsigned t = __umulhi(a.div_mul, texel);
    const unsigned y = (t + ((texel - t) >> (a.div_shift & 0xffu))) >> (a.div_shift >> 8);
    const unsigned x = texel - y * (unsigned)a.fw;
    f.x = x; f.y = y;
    f.coord = make_float2((float)x + 0.5f, (float)y + 0.5f);
    th_float4_load *slot = reinterpret_cast<th_float4_load *>(a.colors + at);
    const th_float4_load c = *slot;
    f.color = make_float4(c.x, c.y, c.z, c.w);
    const float4 o = th_fragment_main(f);
    th_float4_load out;
    out.x = o.x; out.y = o.y; out.z = o.z; out.w = o.w;
    *slot = out;
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

// The harness: one lane per fragment of the pass, 256-thread workgroups, grid-stride (total < 2^31).  A wave reads 256 bytes of
// keys and 1 KiB of varyings, contiguous, and writes that KiB back where it read it; the record is the kernel's argument (scalar
// loads).  No LDS, no atomics; nothing is written but colors[at], at < total.
extern "C" __global__ __launch_bounds__(256) void th_fragment_kernel(const th_fragment_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a, u);
    const unsigned *keys = static_cast<const unsigned *>(a.keys);
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.total; at += gridDim.x * 256u)
        th_fragment_lane(f, a, keys[at], at);
}

// The same stage over the fragments of an emit (th_draw_stages_emit), under their 64-bit keys: the texel is bits 32 .. 55 - of
// the WHOLE target, whatever rows of the particle texture the context holds.  An entry point of its own and no switch in one
// kernel: each loop loads keys of one width, and neither carries the other's registers.
extern "C" __global__ __launch_bounds__(256) void th_fragment_band_kernel(const th_fragment_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a, u);
    const unsigned long long *keys = static_cast<const unsigned long long *>(a.keys);
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.total; at += gridDim.x * 256u)
        th_fragment_lane(f, a, (unsigned)(keys[at] >> 32) & 0xffffffu, at);
}

// ---- the two entry points of a program that reads the fragment's line (th_line) -------------------------------------------------
// th_fragment_kernel and th_fragment_band_kernel with the pass's line records behind the record they take: lines[at] belongs to
// the fragment at keys[at] / colors[at].  A record of its own (th_fragprog.hip: FragmentLineArgs, the same layout): the three
// other entry points keep theirs.  A lane loads its 16-byte record once, beside its varying.
struct th_fragment_line_args {
    th_fragment_args f;
    const th_fragment_line *lines;   // per fragment, in the keys' order
};
static_assert(sizeof(th_fragment_line_args) == 72, "th_fragment_line_args: layout shared with th_fragprog.hip");

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_kernel(const th_fragment_line_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.f, u);
    const unsigned *keys = static_cast<const unsigned *>(a.f.keys);
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.f.total; at += gridDim.x * 256u) {
        const th_fragment_line line = a.lines[at];
        f.line = &line;
        th_fragment_lane(f, a.f, keys[at], at);
    }
}

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_band_kernel(const th_fragment_line_args a, const th_program_uniform_block u)
{
    th_fragment_pass f = th_fragment_pass_of(a.f, u);
    const unsigned long long *keys = static_cast<const unsigned long long *>(a.f.keys);
    for (unsigned at = blockIdx.x * 256u + threadIdx.x; at < a.f.total; at += gridDim.x * 256u) {
        const th_fragment_line line = a.lines[at];
        f.line = &line;
        th_fragment_lane(f, a.f, (unsigned)(keys[at] >> 32) & 0xffffffu, at);
    }
}

// ---- the same stage over the fragments of a BINNED pass (th_bins.hip), where they lie in its page store -----------------------
// Between the emitting pass and the blends every fragment of a binned pass lies at a PLACE of the store: its key
// (y << 44 | x << 32 | stream index of its line; all ones: a place handed out and not written) in frag_keys[place], its varying
// in colors[place] - where the ordinary bins' blend, the crowd's regroup and the long and giant runs all fetch it later.  A bin
// is TH_BIN_REPLICAS lists of pages of 2^TH_BIN_PAGE_SHIFT places; list l = bin * TH_BIN_REPLICAS + r has handed out the places
// v < cursor(bin, r); place v lies in page v >> TH_BIN_PAGE_SHIFT of the list - page 0 is page l of the store, a further page n
// is page_table[l * max_pages + n] (0: none was published, 0xffffffff: the pool was dry) - at v's low bits.  The lines below
// restate th_bins.hip's arithmetic (list_cursor, page_of, place_of: this text cannot include the library's headers); the record
// is th_fragprog.hip's FragmentBinsArgs, the same layout.
#define TH_BIN_REPLICAS 16u
#define TH_BIN_PAGE_SHIFT 8u
#define TH_BINS_TOT_OOB 1
#define TH_BINS_TOT_FLAGS 2
struct th_fragment_bins_args {
    th_fragment_args f;              // keys: the store's 64-bit keys; colors: its varyings; total, div_mul, div_shift: unused (0)
    const unsigned *bin_cursor;      // the lists' cursors: list r of bin b at r * bin_stride + (b & 31) * ((nbins + 31) >> 5) + (b >> 5)
    const unsigned *page_table;      // per list max_pages entries
    const unsigned *totals;          // the pass's totals: [TH_BINS_TOT_OOB], [TH_BINS_TOT_FLAGS] not 0 - a pass nobody will blend
    unsigned bin_stride, max_pages, nbins;
    unsigned pages;                  // pages of the store: every page id is below it
    unsigned replicas, page_shift;   // TH_BIN_REPLICAS, TH_BIN_PAGE_SHIFT as the library was built (anything else: the kernel does nothing)
};
static_assert(sizeof(th_fragment_bins_args) == 112, "th_fragment_bins_args: layout shared with th_fragprog.hip");

// One fragment of a binned pass: x and y are the key's two 12-bit fields (no division), ONE 16-byte load of colors[at], the
// program, ONE 16-byte store back - th_fragment_lane's body behind another split of the key.
__device__ __forceinline__ void th_fragment_place(th_fragment_pass &f, const th_fragment_args &a, unsigned long long key, unsigned at)
{
    const unsigned x = (unsigned)(key >> 32) & 0xfffu, y = (unsigned)(key >> 44) & 0xfffu;
    f.x = x; f.y = y;
    f.coord = make_float2((float)x + 0.5f, (float)y + 0.5f);
    th_float4_load *slot = reinterpret_cast<th_float4_load *>(a.colors + at);
    const th_float4_load c = *slot;
    f.color = make_float4(c.x, c.y, c.z, c.w);
    const float4 o = th_fragment_main(f);
    th_float4_load out;
    out.x = o.x; out.y = o.y; out.z = o.z; out.w = o.w;
    *slot = out;
}

// The harness: blockIdx.x is a bin, whose places - its lists walked one after the other, as bins_blend_kernel walks them - go to
// the workgroup's 256 lanes in rounds; blockIdx.y deals the rounds of one bin to gridDim.y workgroups (a crowded target puts half
// a million fragments into one bin).  The grid is sized by bins, not by fragments: the cursors are on the device.  Skipped: the
// whole pass when it raised a flag or asked for a row nobody holds (it is repeated or abandoned, its table not to be trusted);
// places at or beyond a list's cursor; pages the table does not hold (entry 0 or 0xffffffff, page number >= max_pages, an id
// outside the store); places whose key is the empty key.  No LDS (a lane's list is found among sixteen running sums the wave
// holds in scalar registers), no atomics; nothing is written but colors[place] of live places.
extern "C" __global__ __launch_bounds__(256) void th_fragment_bins_kernel(const th_fragment_bins_args a, const th_program_uniform_block u)
{
    if (a.replicas != TH_BIN_REPLICAS || a.page_shift != TH_BIN_PAGE_SHIFT) return;
    if (a.totals[TH_BINS_TOT_FLAGS] != 0u || a.totals[TH_BINS_TOT_OOB] != 0u) return;
    const unsigned b = blockIdx.x;
    if (b >= a.nbins) return;
    // first place of every list in the walk; a list holds at most max_pages pages (a cursor beyond them: the pass was flagged)
    const unsigned list_cap = a.max_pages << TH_BIN_PAGE_SHIFT;
    const unsigned *cursor = a.bin_cursor + (size_t)(b & 31u) * ((a.nbins + 31u) >> 5) + (b >> 5);
    unsigned first[TH_BIN_REPLICAS + 1u];
    first[0] = 0u;
#pragma unroll
    for (unsigned r = 0; r < TH_BIN_REPLICAS; ++r) {
        const unsigned n = cursor[(size_t)r * a.bin_stride];
        first[r + 1u] = first[r] + (n < list_cap ? n : list_cap);
    }
    const unsigned n = first[TH_BIN_REPLICAS], rounds = (n + 255u) >> 8;
    if (blockIdx.y >= rounds) return;
    th_fragment_pass f = th_fragment_pass_of(a.f, u);
    const unsigned long long *keys = static_cast<const unsigned long long *>(a.f.keys);
    for (unsigned round = blockIdx.y; round < rounds; round += gridDim.y) {
        const unsigned w = (round << 8) + threadIdx.x;
        if (w >= n) continue;
        unsigned r = 0u, base = 0u;
#pragma unroll
        for (unsigned q = 1; q < TH_BIN_REPLICAS; ++q) if (w >= first[q]) { r = q; base = first[q]; }
        const unsigned list = b * TH_BIN_REPLICAS + r, v = w - base, pn = v >> TH_BIN_PAGE_SHIFT;
        unsigned id = list;
        if (pn != 0u) {
            if (pn >= a.max_pages) continue;
            id = a.page_table[(size_t)list * a.max_pages + pn];
            if (id == 0u) continue;
        }
        if (id >= a.pages) continue;                     // (0xffffffff among them)
        const unsigned at = (id << TH_BIN_PAGE_SHIFT) | (v & ((1u << TH_BIN_PAGE_SHIFT) - 1u));
        const unsigned long long key = keys[at];
        if (key == ~0ull) continue;
        th_fragment_place(f, a.f, key, at);
    }
}

// ---- ... and of a program that reads the fragment's line, over the same store (TH_OPT_LINE_BINS) -------------------------------
// th_fragment_bins_kernel with the pass's line records behind the record it takes: lines[at] belongs to the fragment at place
// `at` (th_fragline.hip writes it from the place's key and the line's snapped endpoints: line_record's numbers, as in a
// stream-ordered pass).  A record of its own (th_fragprog.hip: FragmentLineBinsArgs, the same layout); the walk above, and a lane
// loads its 16-byte record once, beside its varying - as th_fragment_line_kernel does.
struct th_fragment_line_bins_args {
    th_fragment_bins_args b;
    const th_fragment_line *lines;   // per place of the store
};
static_assert(sizeof(th_fragment_line_bins_args) == 120, "th_fragment_line_bins_args: layout shared with th_fragprog.hip");

extern "C" __global__ __launch_bounds__(256) void th_fragment_line_bins_kernel(const th_fragment_line_bins_args a, const th_program_uniform_block u)
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
        const th_fragment_line line = a.lines[at];
        f.line = &line;
        th_fragment_place(f, a.b.f, key, at);
    }
}
)TH_PRELUDE"
