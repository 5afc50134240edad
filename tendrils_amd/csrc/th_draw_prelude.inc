R"TH_PRELUDE(// th_draw_prelude.inc - what th_draw_program_compile puts in front of a draw program, after the text of th_taps.inc and of
// th_stream.inc (th_drawprog.hip embeds this file as text: the first and the last line make it one raw string literal).
// Self-contained: no project header, only what hiprtc's built-in headers give.  Compiled with the product's arithmetic flags
// (-ffp-contract=off: a*b+c stays two rounded fp32 operations, as in the reference's shaders).
//
// A draw program defines ONE device function,
//     __device__ th_vertex th_vertex_main(const th_vertex_pass &v);
// main() of the vertex shader of one pass of draw() (renderShader / flowShader under particles.draw(..., gl.LINES)): it is
// called once per vertex of the stream and returns gl_Position.xy (w = 1) and the vec4 varying.  Everything behind it - the
// line's hexagon, clipping, snapping, scan conversion, the varying along the snapped endpoints, the blend in primitive order -
// is the library's (th_raster.hpp), and the fragment stage is gl_FragColor = the varying.
//
// th_draw_args is the launch record th_drawprog.hip fills (same layout there; the static_asserts pin the sizes).
struct th_draw_args {
    const float4 *cur, *prev;    // buffers[0], buffers[1]: f32 texels in texel order
    void *vertices;              // 32 bytes per stream vertex: { float px, py; unsigned live, pad; float c[4] }
    const float4 *flow;          // fw x fh, as it was before this pass
    const float4 *colormap;      // cw x ch (null: none is held)
    double inv_x, inv_y;         // 1/(max(W,2)-1), 1/(max(2H,2)-1): Particles.generateLUT
    unsigned W, H, count;        // the particle texture; count = 2 W H stream vertices
    int fw, fh, cw, ch;
    unsigned reserved0;
    const unsigned *perm;        // th_draw_vertex_slots_kernel alone: cur / prev are held in a slot order, perm[slot] = particle id
};
static_assert(sizeof(th_draw_args) == 96, "th_draw_args: layout shared with th_drawprog.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_vertex_pass {
    float2 uv;                   // the attribute, as the stream holds it: fp32 of the doubles i / (W - 1), j / (2H - 1)
    float4 state;                // stateAtFrame(uv, dataRes, previous, particles): the texel AND the buffer the lookup selects
    bool from_current;           // ... `particles` (else `previous`)
    unsigned column, vertex;     // i, j of the stream: column i of the particle texture, vertex j of 2H
    unsigned line;               // the stream index of the vertex's line, i * H + (j >> 1): the order the lines are blended in
    float2 dataRes, geomRes;     // (W, H), (W, 2H)
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(v))
    const th_draw_args *args;
};
struct th_vertex {
    float2 position;             // gl_Position.xy (w = 1); a non-finite one, or one beyond 1024, draws nothing
    float4 color;                // the varying: the fragment's colour
    unsigned live = 1u;          // 0: th_discard_vertex()
};

__device__ th_vertex th_vertex_main(const th_vertex_pass &v);

// the vertex of an `if(state.xy != inert)` that was not taken: a line with such a vertex draws nothing
__device__ __forceinline__ th_vertex th_discard_vertex()
{
    th_vertex o;
    o.position = make_float2(0.0f, 0.0f);
    o.color = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o.live = 0u;
    return o;
}

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_vertex_pass &v)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(v.uniforms);
}

// texture2D(flow, (u, w)) / texture2D(colorMap, (u, w)): NEAREST, CLAMP_TO_EDGE, always inside the texture (th_taps.inc).  The
// flow is the field as it was BEFORE this pass, also in a pass that draws into it: every vertex has run before anything blends.
__device__ __forceinline__ float4 th_flow(const th_vertex_pass &v, float u, float w)
{
    const th_draw_args &a = *v.args;
    return a.flow[(size_t)th_tap_nearest(w, a.fh) * a.fw + th_tap_nearest(u, a.fw)];
}
__device__ __forceinline__ float2 th_flow_res(const th_vertex_pass &v) { return make_float2((float)v.args->fw, (float)v.args->fh); }
// no colour map held: the 1 x 1 zero texture, as the built-in view stage reads it
__device__ __forceinline__ float4 th_colormap(const th_vertex_pass &v, float u, float w)
{
    const th_draw_args &a = *v.args;
    if (!a.colormap) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return a.colormap[(size_t)th_tap_nearest(w, a.ch) * a.cw + th_tap_nearest(u, a.cw)];
}
__device__ __forceinline__ float2 th_colormap_res(const th_vertex_pass &v)
{
    const th_draw_args &a = *v.args;
    return a.colormap ? make_float2((float)a.cw, (float)a.ch) : make_float2(1.0f, 1.0f);
}

// The harness: one lane per stream vertex, 256-thread workgroups, grid-stride.  Lane `idx` writes record `idx` of the vertex
// buffer - record 2 (row W + column) + (j & 1): a line's two vertices are 64 adjacent bytes, a wave's stores one contiguous
// 2 KiB run, two 16-byte stores per lane; the state texel comes in as one 16-byte load.  The record is the kernel's argument
// (scalar loads); no LDS, no atomics.
typedef float th_float4_load __attribute__((ext_vector_type(4)));
extern "C" __global__ __launch_bounds__(256) void th_draw_vertex_kernel(const th_draw_args a, const th_program_uniform_block u)
{
    th_vertex_pass v;
    v.dataRes = make_float2((float)a.W, (float)a.H);
    v.geomRes = make_float2((float)a.W, (float)(2u * a.H));
    v.uniforms = u.bytes;
    v.args = &a;
    float4 *records = static_cast<float4 *>(a.vertices);
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
        const unsigned t = idx >> 1, row = t / a.W, col = t - row * a.W;
        const unsigned j = 2u * row + (idx & 1u);
        const th_stream_at<float4> s = th_stream_lookup(col, j, a.inv_x, a.inv_y, (int)a.W, (int)a.H, 0u, a.cur, a.prev);
        v.uv = make_float2(s.uvx, s.uvy);
        v.from_current = s.from_cur;
        // (as ONE 16-byte load: read as a float4 struct, the compiler fetches .xy first and .zw behind the program's inert test)
        const th_float4_load t4 = *reinterpret_cast<const th_float4_load *>(s.tex + ((size_t)s.row * a.W + (size_t)s.col));
        v.state = make_float4(t4.x, t4.y, t4.z, t4.w);
        v.column = col;
        v.vertex = j;
        v.line = col * a.H + row;
        const th_vertex o = th_vertex_main(v);
        records[2u * (size_t)idx] = make_float4(o.position.x, o.position.y, __uint_as_float(o.live ? 1u : 0u), 0.0f);
        records[2u * (size_t)idx + 1u] = o.color;
    }
}

// The same stage over a ring held in a SLOT order (the tile-sorted order the integrator steps over): one lane per slot s,
// a.perm[s] its particle - texel (column, row) - and a.cur[s] / a.prev[s] that particle's texels: coalesced 16-byte loads whatever
// the order.  Both stream vertices of the particle's line go through th_vertex_main and their records are written where the
// other kernel writes them - 64 adjacent bytes per lane at the line's texel index, scattered between lanes - so that whatever
// reads the buffer finds it the same.  th_stream_lookup still chooses texel and buffer; only for shapes whose lookup lands on
// the line's own texel is this kernel launched (th_draw.hip: deposit_prepare), and the texel is then the slot's.
// th_vertex_pass is field for field what the kernel above hands the program.
extern "C" __global__ __launch_bounds__(256) void th_draw_vertex_slots_kernel(const th_draw_args a, const th_program_uniform_block u)
{
    th_vertex_pass v;
    v.dataRes = make_float2((float)a.W, (float)a.H);
    v.geomRes = make_float2((float)a.W, (float)(2u * a.H));
    v.uniforms = u.bytes;
    v.args = &a;
    float4 *records = static_cast<float4 *>(a.vertices);
    const unsigned slots = a.count >> 1;
    for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < slots; s += gridDim.x * 256u) {
        const unsigned t = a.perm[s], row = t / a.W, col = t - row * a.W;
        const th_float4_load own_cur = *reinterpret_cast<const th_float4_load *>(a.cur + s);
        const th_float4_load own_prev = *reinterpret_cast<const th_float4_load *>(a.prev + s);
        v.column = col;
        v.line = col * a.H + row;
#pragma unroll
        for (unsigned e = 0; e < 2u; ++e) {
            const unsigned j = 2u * row + e;
            const th_stream_at<float4> at = th_stream_lookup(col, j, a.inv_x, a.inv_y, (int)a.W, (int)a.H, 0u, a.cur, a.prev);
            v.uv = make_float2(at.uvx, at.uvy);
            v.from_current = at.from_cur;
            const th_float4_load t4 = at.from_cur ? own_cur : own_prev;
            v.state = make_float4(t4.x, t4.y, t4.z, t4.w);
            v.vertex = j;
            const th_vertex o = th_vertex_main(v);
            const size_t idx = 2u * (size_t)t + e;
            records[2u * idx] = make_float4(o.position.x, o.position.y, __uint_as_float(o.live ? 1u : 0u), 0.0f);
            records[2u * idx + 1u] = o.color;
        }
    }
}

// The same stage over a ROW BAND (th_draw_program_emit: a context that holds rows row0 .. row0 + rows of the W x H texture;
// the whole texture is the band of all rows).  The record is its own: a th_draw_args at its head - what th_flow / th_colormap
// read through v.args; H the WHOLE texture's height, count = 2 W rows, the band's stream vertices, cur / prev the band's rows -
// and behind it what only a band has.
struct th_draw_band_args {
    th_draw_args a;
    const float4 *halo_lo, *halo_hi;   // row row0 - 1 / row0 + rows of the neighbouring bands, as th_deposit_set_halo takes them:
                                       // W texels of buffers[0], then W of buffers[1] (null: nobody supplied it)
    unsigned *oob;                     // set to 1 when a lookup lands on a row that neither the band nor a halo row holds
    unsigned row0, rows;
};
static_assert(sizeof(th_draw_band_args) == 128, "th_draw_band_args: layout shared with th_drawprog.hip");
// One lane per stream vertex of the band, as th_draw_vertex_kernel: lane `idx` is vertex e = idx & 1 of the line of the band's
// texel idx >> 1 and writes record `idx` - where the raster stage reads it, by LOCAL row (dep_vertex_read) - in two 16-byte
// stores; the state comes in as one 16-byte load.  What the program sees is the GLOBAL stream: j = 2 (row0 + local row) + e,
// line = column H + global row, dataRes / geomRes the whole texture's - field for field what the unsharded kernel hands it for
// the same particle.  th_stream_lookup counts the row it lands on from row0: -1 and `rows` are the neighbours' edge rows, read
// from the halo rows (chosen as dep_fetch chooses, th_raster.hpp); where that row is absent the flag is raised - the pass is
// refused - and the load goes to the band's nearest row instead: never out of bounds.  No LDS, no atomics.
extern "C" __global__ __launch_bounds__(256) void th_draw_vertex_band_kernel(const th_draw_band_args b, const th_program_uniform_block u)
{
    const th_draw_args &a = b.a;
    th_vertex_pass v;
    v.dataRes = make_float2((float)a.W, (float)a.H);
    v.geomRes = make_float2((float)a.W, (float)(2u * a.H));
    v.uniforms = u.bytes;
    v.args = &b.a;
    float4 *records = static_cast<float4 *>(a.vertices);
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
        const unsigned t = idx >> 1, local = t / a.W, col = t - local * a.W;
        const unsigned row = b.row0 + local;
        const unsigned j = 2u * row + (idx & 1u);
        const th_stream_at<float4> s = th_stream_lookup(col, j, a.inv_x, a.inv_y, (int)a.W, (int)a.H, b.row0, a.cur, a.prev);
        v.uv = make_float2(s.uvx, s.uvy);
        v.from_current = s.from_cur;
        // (one unconditional load from a selected address, as dep_fetch)
        const int held = s.row < 0 ? 0 : (s.row < (int)b.rows ? s.row : (int)b.rows - 1);
        const float4 *from = s.tex + ((size_t)held * a.W + (size_t)s.col);
        if (held != s.row) {
            const float4 *halo = s.row == -1 ? b.halo_lo : (s.row == (int)b.rows ? b.halo_hi : nullptr);
            if (halo) from = halo + (s.from_cur ? 0u : a.W) + s.col;
            else *b.oob = 1u;
        }
        const th_float4_load t4 = *reinterpret_cast<const th_float4_load *>(from);
        v.state = make_float4(t4.x, t4.y, t4.z, t4.w);
        v.column = col;
        v.vertex = j;
        v.line = col * a.H + row;
        const th_vertex o = th_vertex_main(v);
        records[2u * (size_t)idx] = make_float4(o.position.x, o.position.y, __uint_as_float(o.live ? 1u : 0u), 0.0f);
        records[2u * (size_t)idx + 1u] = o.color;
    }
}
)TH_PRELUDE"
