// th_drawprog.hip - draw programs: a caller's vertex stage in one pass of draw().  The reference's third seam (th_program.hip and
// th_screen.hip have the other two): new Tendrils(gl, { renderShader, flowShader }) (src/index.js:70-71, 114-120) - the shader
// pair particles.draw(..., gl.LINES) runs in the two passes of draw(); the vertex stage itself is a template over an `apply`
// function there (src/flow/vert/main.vert).  Here the caller's vertex shader is HIP source for one device function,
// th_vertex_main (th_draw_prelude.inc), compiled for gfx950 at run time like the other two kinds (th_program.hip:
// program_compile).  It runs once per vertex of the stream into a context-owned vertex buffer; the pipeline the built-in pass of
// the same context would take - binned (th_bins.hip) or stream-ordered (th_deposit.hip) - then draws the lines from that buffer
// instead of from the library's own vertex stage: everything behind the vertex stage is the same code (th_raster.hpp:
// dep_vertex_read).  The buffer is texel-indexed and the raster stage of such a pass reads nothing else, so the binned pass
// walks it in texel order and a tile-sorted ring stays as it is: only the vertex kernel follows the slots
// (th_draw_vertex_slots_kernel).
#include "th_ctx.hpp"

using namespace thi;

namespace {

// the tap rules and the stream lookup as text (th_taps.inc, th_stream.inc: the library's kernels compile the same lines), then
// the prelude
#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#undef TH_TAPS
#define TH_STREAM(...) #__VA_ARGS__
const char kStream[] =
#include "th_stream.inc"
    ;
#undef TH_STREAM
const char kPrelude[] =
#include "th_draw_prelude.inc"
    ;

// the launch record (th_draw_prelude.inc: th_draw_args, th_program_uniform_block - the same layout)
struct DrawArgs {
    const float4 *cur, *prev;
    void *vertices;
    const float4 *flow, *colormap;
    double inv_x, inv_y;
    uint32_t W, H, count;
    int32_t fw, fh, cw, ch;
    uint32_t reserved0;
    const uint32_t *perm;        // th_draw_vertex_slots_kernel: slot -> particle id of the order cur / prev are held in
};
using KernArgs = ProgramKernArgs<DrawArgs>;
static_assert(sizeof(DrawArgs) == 96 && offsetof(DrawArgs, perm) == 88 && offsetof(KernArgs, u) == 96 && sizeof(KernArgs) == 96 + kUniformBytes,
              "launch record: layout shared with th_draw_prelude.inc");

// ... and a row band's (th_draw_band_args: a th_draw_args at its head, then what only a band has)
struct BandArgs {
    DrawArgs a;
    const float4 *halo_lo, *halo_hi;
    uint32_t *oob;
    uint32_t row0, rows;
};
using BandKernArgs = ProgramKernArgs<BandArgs>;
static_assert(sizeof(BandArgs) == 128 && offsetof(BandArgs, halo_lo) == 96 && offsetof(BandArgs, row0) == 120 && offsetof(BandKernArgs, u) == 128 &&
              sizeof(BandKernArgs) == 128 + kUniformBytes, "a band's launch record: layout shared with th_draw_prelude.inc");

// what the records of all three vertex kernels say alike: the buffer they fill, what th_flow / th_colormap tap, the stream's scales
// and shape (H: the whole texture's), `lines` lines of the rows this context holds
void record_shared(const th_context *c, const th::DepositParams &p, size_t lines, DrawArgs &a)
{
    a.vertices = c->draw_vertices.get();
    a.flow = c->flow; a.fw = c->fw; a.fh = c->fh;
    a.colormap = c->colormap; a.cw = c->cmap_w; a.ch = c->cmap_h;
    a.inv_x = p.inv_x; a.inv_y = p.inv_y;
    a.W = p.W; a.H = p.H; a.count = (uint32_t)(2 * lines);
}

// what every vertex kernel needs and the raster stage of `p` then reads: the module, the pass's mode and line width, the vertex buffer
th_status vertex_buffer(th_context *c, const PassSpec &s, th::DepositParams &p, size_t lines, ProgramModule **m)
{
    if (th_status st = program_loaded(c, s.vertex, m)) return st;
    if (s.pass == TH_PASS_VIEW) p.mode = 1;
    p.line_half = 0.5f * drawn_line_width(c, s.pass);
    if (th_status st = c->draw_vertices.reserve(4 * lines, 4 * lines)) return st;
    p.vertices = c->draw_vertices;
    return TH_OK;
}

// the record and the uniform block travel in the kernel's argument segment; a memory-bound pass (program_launch)
template <class Record> th_status vertex_launch(th_context *c, hipFunction_t fn, size_t lanes, Record &k)
{
    if (!lanes) return TH_OK;
    LaunchTimer timer;                                  // (th_kernel_timing: the vertex kernel alone)
    if (th_status st = timer.begin(c)) return st;
    if (th_status st = program_launch(c, fn, lanes, k)) return st;
    return timer.end(c);
}

}  // namespace

th_status thi::vertex_stage_run(th_context *c, const PassSpec &s, th::DepositParams &p, bool bins)
{
    const size_t lines = c->texels();
    TH_REQUIRE(2 * (uint64_t)lines <= 0x7fffffffull, "a %dx%d particle texture is beyond what a draw program's vertex kernel indexes", c->cfg.width, c->cfg.height);
    ProgramModule *m = nullptr;
    if (th_status st = vertex_buffer(c, s, p, lines, &m)) return st;
    KernArgs k{};
    DrawArgs &a = k.a;
    hipFunction_t fn = m->entry[kDrawVertex];
    size_t lanes = 2 * lines;                           // (one per stream vertex)
    const int order = bins ? order_of(c, c->ring[0]) : -1;
    if (order >= 0) {
        // over sorted slots (f32 texels, both buffers in ONE order: the gate, align_slot_orders): one lane per slot
        a.cur = c->ring[0]; a.prev = c->ring[1]; a.perm = c->orders[(size_t)order].perm;
        fn = m->entry[kDrawSlots]; lanes = lines;
    } else {
        float4 *cur = nullptr, *prev = nullptr;             // (a packed ring: f32 copies, as th_program_run sees it)
        if (th_status st = unpacked_view(c, c->ring[0], 0, &cur)) return st;
        if (th_status st = unpacked_view(c, c->ring[1], 1, &prev)) return st;
        a.cur = cur; a.prev = prev;
    }
    record_shared(c, p, lines, a);
    k.set_uniforms(s.uniforms, s.uniform_bytes);
    return vertex_launch(c, fn, lanes, k);
}

// by local row, what the program makes of the GLOBAL stream (the neighbours' edge rows from the halo rows): th_draw_vertex_band_kernel
th_status thi::vertex_stage_band(th_context *c, const PassSpec &s, th::DepositParams &p)
{
    const size_t lines = c->texels();
    TH_REQUIRE(2 * (uint64_t)lines <= 0x7fffffffull, "a band of %dx%d particles is beyond what a draw program's vertex kernel indexes", c->cfg.width, c->cfg.height);
    ProgramModule *m = nullptr;
    if (th_status st = vertex_buffer(c, s, p, lines, &m)) return st;
    BandKernArgs k{};
    DrawArgs &a = k.a.a;
    float4 *cur = nullptr, *prev = nullptr;             // (a packed ring: f32 copies, as the halo rows are)
    if (th_status st = unpacked_view(c, c->ring[0], 0, &cur)) return st;
    if (th_status st = unpacked_view(c, c->ring[1], 1, &prev)) return st;
    a.cur = cur; a.prev = prev;
    record_shared(c, p, lines, a);                     // (count: the band's vertices)
    k.a.halo_lo = p.halo_lo; k.a.halo_hi = p.halo_hi; k.a.oob = p.oob;
    k.a.row0 = p.row0; k.a.rows = p.rows;
    k.set_uniforms(s.uniforms, s.uniform_bytes);
    return vertex_launch(c, m->entry[kDrawBand], 2 * lines, k);
}

extern "C" {

th_status th_draw_program_compile(const char *source, const char *name, th_program **out)
{
    return program_compile(kDrawProgram, std::string(kTaps) + "\n" + kStream + "\n" + kPrelude, source, name, out);
}

// One pass of draw() with the program as its vertex stage, through the pipeline the built-in pass of this context would take, as
// th_flow_deposit / th_view_draw go about it (th_draw.hip: pass_run).
th_status th_draw_program_run(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t pass, uint64_t *fragments)
{
    if (th_status s = use(c, pass == TH_PASS_VIEW)) return s;      // (the view pass writes no state and no flow: th_view_draw)
    if (th_status s = program_run_args(prog, kDrawProgram, "th_draw_program_run", uniforms, uniform_bytes)) return s;
    TH_REQUIRE(pass == TH_PASS_FLOW || pass == TH_PASS_VIEW, "unknown pass %d", pass);
    // (this LOCAL pass has no exchange to go through; a band's program pass is th_draw_program_emit / th_draw_program_sharded)
    if (th_status s = refuse_band(c, "draw program", "a band's pass goes through the owners' exchange, which carries the built-in stages alone")) return s;
    draw_moves_nothing(c);
    return pass_run(c, program_pass(pass, prog, uniforms, uniform_bytes), fragments);
}

// The program pass of a row band - what th_deposit_emit / th_view_emit are to the built-in stages (th_shard.hip: pass_emit), keyed
// and parted by owner for th_deposit_merge (flow) / th_view_merge (view).  Unlike those two it tells th_draw_query what it emitted.
th_status th_draw_program_emit(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t pass,
                               uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (th_status s = use(c, pass == TH_PASS_VIEW)) return s;
    if (th_status s = program_run_args(prog, kDrawProgram, "th_draw_program_emit", uniforms, uniform_bytes)) return s;
    TH_REQUIRE(pass == TH_PASS_FLOW || pass == TH_PASS_VIEW, "unknown pass %d", pass);
    TH_REQUIRE(count && keys_dev && colors_dev, "null outputs");
    const th_status emitted = pass_emit(c, program_pass(pass, prog, uniforms, uniform_bytes), count, keys_dev, colors_dev);
    if (emitted == TH_OK) draw_streamed(c, *count);
    return emitted;
}

}  // extern "C"
