// th_fragprog.hip - fragment programs: a caller's fragment stage in one pass of draw().  The second half of the reference's
// shader pairs, new Tendrils(gl, { flowShader: [vert, frag], renderShader: [vert, frag] }) (src/index.js:70-71, 114-120);
// th_drawprog.hip has the first.  The caller's fragment shader is HIP source for one device function, th_fragment_main
// (th_fragment_prelude.inc), compiled for gfx950 at run time like the other kinds (th_program.hip: program_compile).  It runs
// once per fragment, in place over the array the stream-ordered pipeline holds between its emit and its sort - texel key beside
// interpolated varying -, so nothing of the raster or blend kernels knows of it: the entry points here load the stage and describe
// the pass with it (PassSpec::fragment) to the body every pass goes through (th_draw.hip: pass_run / pass_emit); it travels down as
// an argument, and deposit_run (th_draw.hip) / emit_parted (th_shard.hip) call fragment_stage_run where the fragments lie.
// Under TH_OPT_STAGE_BINS a local pass with a stage may go through the bins (th_bins.hip): its fragments then lie in the page
// store, and bins_pass_emit (th_draw.hip) calls fragment_stage_run_bins between the emitting pass and the blends.
// A program whose source names th_line reads the fragment's line: its pass stays stream-ordered, fragment_stage_run has the line
// kernel (th_fragline.hip) write a record per fragment beside key and varying, and launches the two entry points that take them.
// Under TH_OPT_LINE_BINS as well such a pass goes through the bins like the others: fragment_stage_run_bins has th_fragline.hip's
// two other kernels write a record per place of the store and launches the entry point that takes those.
// th_draw_stages_pair draws both passes with their stages from ONE rasterisation where that gives the two passes' bits (th_draw's
// mode 2: two varyings a fragment): both stages then travel down in the one argument, and fragment_stage_run / _run_bins launch
// a pair entry point (th_fragment_pair_prelude.inc) once per stage, each over its half of the pairs.
// Eight entry points (th_ctx.hpp: FragmentEntry), one way to launch them: a record - the context's part, where the fragments lie,
// what the entry point takes behind that - and stage_launch.
#include "th_ctx.hpp"

using namespace thi;

namespace {

// the tap rules as text (th_taps.inc: the library's kernels compile the same lines), the walk over a binned pass's page store as
// text (th_bins_walk.inc: th_fragline.hip compiles the same lines, and ties their constants to th_bins.hip's), then the prelude
#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#undef TH_TAPS
#define TH_BINS_WALK(...) #__VA_ARGS__
const char kBinsWalk[] =
#include "th_bins_walk.inc"
    ;
#undef TH_BINS_WALK
const char kPrelude[] =
#include "th_fragment_prelude.inc"
    ;
// ... and behind it the two entry points of th_draw_stages_pair's one rasterisation
const char kPairPrelude[] =
#include "th_fragment_pair_prelude.inc"
    ;

// the launch record (th_fragment_prelude.inc: th_fragment_args, th_program_uniform_block - the same layout)
struct FragmentArgs {
    const void *keys;
    float4 *colors;
    const float4 *flow, *colormap;
    uint32_t total;
    int32_t fw, fh, cw, ch;
    int32_t pass;
    uint32_t div_mul, div_shift;
};
// ... of the entry points over the page store (th_fragment_bins_args): the first record, then where the bins' lists lie.
// `replicas` / `page_shift` keep their place in the layout; the kernels' constants are th_bins_walk.inc's own, which
// th_fragline.hip's static_assert holds to the library's
struct FragmentBinsArgs {
    FragmentArgs f;
    const uint32_t *bin_cursor, *page_table, *totals;
    uint32_t bin_stride, max_pages, nbins, pages;
    uint32_t replicas, page_shift;
};
// ... of the entry points of a program that reads th_line (th_fragment_line_args, th_fragment_line_bins_args): either record,
// then the line records of the fragments / of the places (th_fragline.hip)
template <class First> struct WithLines {
    First first;
    const th::FragmentLine *lines;
};
// ... and of th_fragment_pair_kernel / th_fragment_pair_bins_kernel (th_fragment_pair_prelude.inc: th_fragment_pair_args,
// th_fragment_pair_bins_args): either record, then which of a fragment's two varyings the stage runs over - both passes from
// one rasterisation (p.mode == 2: th_draw_stages_pair)
template <class First> struct WithHalf {
    First first;
    uint32_t half;
};
template <class Args, size_t Bytes, size_t Last> constexpr bool record_is()      // sizeof, the offset of what stands behind `first`, the uniform block behind both
{
    using K = ProgramKernArgs<Args>;
    return sizeof(Args) == Bytes && offsetof(Args, first) == 0 && sizeof(Args::first) == Last && offsetof(K, u) == (Bytes + 15) / 16 * 16 && sizeof(K) == (Bytes + 15) / 16 * 16 + kUniformBytes;
}
static_assert(sizeof(FragmentArgs) == 64 && offsetof(FragmentArgs, total) == 32 && offsetof(FragmentArgs, div_mul) == 56 && offsetof(ProgramKernArgs<FragmentArgs>, u) == 64 &&
              sizeof(ProgramKernArgs<FragmentArgs>) == 64 + kUniformBytes, "launch record: layout shared with th_fragment_prelude.inc");
static_assert(sizeof(FragmentBinsArgs) == 112 && offsetof(FragmentBinsArgs, bin_cursor) == 64 && offsetof(FragmentBinsArgs, bin_stride) == 88 &&
              offsetof(FragmentBinsArgs, replicas) == 104 && offsetof(ProgramKernArgs<FragmentBinsArgs>, u) == 112 && sizeof(ProgramKernArgs<FragmentBinsArgs>) == 112 + kUniformBytes,
              "bins launch record: layout shared with th_fragment_prelude.inc");
static_assert(record_is<WithLines<FragmentArgs>, 72, 64>() && offsetof(WithLines<FragmentArgs>, lines) == 64 && record_is<WithLines<FragmentBinsArgs>, 120, 112>() &&
              offsetof(WithLines<FragmentBinsArgs>, lines) == 112 && sizeof(th::FragmentLine) == 16, "line launch records: layout shared with th_fragment_prelude.inc");
static_assert(record_is<WithHalf<FragmentArgs>, 72, 64>() && offsetof(WithHalf<FragmentArgs>, half) == 64 && record_is<WithHalf<FragmentBinsArgs>, 120, 112>() &&
              offsetof(WithHalf<FragmentBinsArgs>, half) == 112, "pair launch records: layout shared with th_fragment_pair_prelude.inc");
// A bin's rounds of 256 places are dealt to this many workgroups (gridDim.y).  Every workgroup reads its bin's sixteen cursors
// before it knows whether a round is left for it, and on an ordinary target - 1 700 places a bin at 1080p, seven rounds - most
// of a wide deal's workgroups find none: the kernel's time is then the time of starting them (8 160 bins x 128: 0.88 ms for a
// pass whose bytes copy in 0.10).  A crowded target - most fragments in a few hundred bins of tens of thousands of places -
// wants the wider deal: a workgroup walks its rounds one behind the other, a chain of three loads and a store each.  Which of
// the two the target is was the last draw's to say, as for the early blend (deposit_run_bins).  Measured, ms a pass, ordinary /
// crowded target: deal 2: 0.130 / 0.460, 8: 0.161 / 0.356, 32: 0.303 / 0.437, 128: 0.877 / 0.890 (profiles/fragment_program_bins.txt).
using th::kBinsStageDeal;                  // (2; th_kernels.hpp: the line records of a binned pass are dealt alike)
using th::kBinsStageDealCrowded;           // (8)

// n / d for every 32-bit n by one multiplication (Granlund & Montgomery 1994, the round-up form): the multiplier and both shifts
void divide_by(uint32_t d, uint32_t &mul, uint32_t &shifts)
{
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) ++l;
    mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1u);
    shifts = (l < 1u ? l : 1u) | ((l > 1u ? l - 1u : 0u) << 8);
}

// a slot of th_draw_stages: null, or a program of `kind` with its block
th_status stage_args(const th_program *prog, ProgramKind kind, const char *entry, const char *slot, const void *uniforms, uint32_t uniform_bytes)
{
    if (!prog) {
        TH_REQUIRE(uniform_bytes == 0, "%s: %u %s uniform bytes and no %s program", entry, uniform_bytes, slot, slot);
        return TH_OK;
    }
    TH_REQUIRE(prog->kind == kind, "%s takes a %s as its %s stage: '%s' is a %s", entry, program_kind_name(kind), slot, prog->name.c_str(), program_kind_name(prog->kind));
    TH_REQUIRE(uniform_bytes <= kUniformBytes, "%s uniform block of %u bytes (at most %u)", slot, uniform_bytes, kUniformBytes);
    TH_REQUIRE(uniforms || uniform_bytes == 0, "null %s uniforms", slot);
    return TH_OK;
}

// what both entry points refuse before anything is launched
th_status stages_args(const th_context *c, const th_draw_stages *s, int32_t pass, const char *entry, const char *builtin_calls)
{
    TH_REQUIRE(c, "null context");
    TH_REQUIRE(s, "null stages");
    TH_REQUIRE(s->vertex || s->fragment, "%s with neither a vertex nor a fragment program: the library's own stages are %s", entry, builtin_calls);
    if (th_status st = stage_args(s->vertex, kDrawProgram, entry, "vertex", s->vertex_uniforms, s->vertex_uniform_bytes)) return st;
    if (th_status st = stage_args(s->fragment, kFragmentProgram, entry, "fragment", s->fragment_uniforms, s->fragment_uniform_bytes)) return st;
    TH_REQUIRE(pass == TH_PASS_FLOW || pass == TH_PASS_VIEW, "unknown pass %d", pass);
    TH_REQUIRE(s->vertex || s->builtin, "%s without a vertex program needs `builtin`: the %s of the library's vertex stage", entry,
               pass == TH_PASS_VIEW ? "th_render_uniforms" : "th_deposit_uniforms");
    return TH_OK;
}

// the pass th_draw_stages names: its vertex slot, and its fragment stage as this context loaded it (`stage`: the caller's storage)
th_status stages_pass(th_context *c, const th_draw_stages *s, int32_t pass, FragmentStage &stage, PassSpec &spec)
{
    spec = s->vertex ? program_pass(pass, s->vertex, s->vertex_uniforms, s->vertex_uniform_bytes) : builtin_pass(pass, s->builtin);
    if (!s->fragment) return TH_OK;
    if (th_status st = program_loaded(c, s->fragment, &stage.module)) return st;
    stage.uniforms = s->fragment_uniforms; stage.uniform_bytes = s->fragment_uniform_bytes; stage.pass = pass;
    spec.fragment = &stage;
    return TH_OK;
}

// does `source` name the identifier `word`?  (anywhere: a comment counts - the pass then pays for records nobody reads)
bool names_identifier(const char *source, const char *word)
{
    auto part = [](char ch) { return ch == '_' || (ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z'); };
    const size_t n = strlen(word);
    for (const char *at = strstr(source, word); at; at = strstr(at + 1, word))
        if ((at == source || !part(at[-1])) && !part(at[n])) return true;
    return false;
}

// the context's part of a record: the pass, and the textures as they were before it
void stage_context(const th_context *c, const FragmentStage &stage, FragmentArgs &a)
{
    a.flow = c->flow; a.fw = c->fw; a.fh = c->fh;
    a.colormap = c->colormap; a.cw = c->cmap_w; a.ch = c->cmap_h;
    a.pass = stage.pass;
}
// the record every stream-ordered entry point starts with ...
void stage_record(const th_context *c, const FragmentStage &stage, const th::DepositParams &p, uint32_t total, FragmentArgs &a)
{
    stage_context(c, stage, a);
    a.keys = p.keys64 ? static_cast<const void *>(p.keys64) : static_cast<const void *>(p.keys);
    a.colors = p.colors;
    a.total = total;
    divide_by((uint32_t)c->fw, a.div_mul, a.div_shift);
}
// ... and every entry point over the page store (total: none - the cursors are on the device)
void stage_record(const th_context *c, const FragmentStage &stage, const th::DepositParams &p, uint32_t, FragmentBinsArgs &a)
{
    stage_context(c, stage, a.f);
    a.f.keys = p.frag_keys; a.f.colors = p.colors;
    a.bin_cursor = p.bin_cursor; a.bin_stride = p.bin_stride;
    a.page_table = p.page_table; a.max_pages = p.max_pages;
    a.totals = p.totals;
    a.nbins = p.nbins; a.pages = p.nbins * th::kBinReplicas + p.pool_pages;
    a.replicas = th::kBinReplicas; a.page_shift = (uint32_t)__builtin_ctz(th::kBinPage);
}

// where a stage's workgroups go: over `lanes` fragments on the grid of the streaming passes, or (lanes 0) a bin of the page
// store a workgroup column, its rounds dealt to `deal` workgroups
struct StageGrid { size_t lanes; int bins, deal; };

// the filled record with the stage's uniforms behind it, to the stage's entry point `entry`; th_kernel_timing: this launch alone
template <class Args> th_status stage_launch(th_context *c, const FragmentStage &stage, FragmentEntry entry, ProgramKernArgs<Args> &k, const StageGrid &g)
{
    k.set_uniforms(stage.uniforms, stage.uniform_bytes);
    const hipFunction_t fn = stage.module->entry[entry];
    LaunchTimer timer;
    if (th_status s = timer.begin(c)) return s;
    if (th_status s = g.lanes ? program_launch(c, fn, g.lanes, k) : program_launch_grid(c, fn, g.bins, &k, sizeof k, g.deal)) return s;
    return timer.end(c);
}

// both passes from one rasterisation: two varyings a fragment (a place), and `pair` the two stages - the flow pass's over the
// first of every two, then the view pass's over the second (module null: that half stays as the library interpolated it); each
// launch in an event pair of its own
template <class First> th_status stage_launch_pair(th_context *c, const FragmentStage *pair, const th::DepositParams &p, uint32_t total, FragmentEntry entry, const StageGrid &g)
{
    for (uint32_t half = 0; half < 2; ++half) {
        if (!pair[half].module) continue;
        ProgramKernArgs<WithHalf<First>> k{};
        stage_record(c, pair[half], p, total, k.a.first);
        k.a.half = half;
        if (th_status s = stage_launch(c, pair[half], entry, k, g)) return s;
    }
    return TH_OK;
}

// `stage` alone: its record, with the line records behind it for a program that reads th_line
template <class First> th_status stage_launch_one(th_context *c, const FragmentStage &stage, const th::DepositParams &p, uint32_t total, FragmentEntry entry,
                                                  const th::FragmentLine *lines, const StageGrid &g)
{
    if (lines) {
        ProgramKernArgs<WithLines<First>> k{};
        stage_record(c, stage, p, total, k.a.first);
        k.a.lines = lines;
        return stage_launch(c, stage, entry, k, g);
    }
    ProgramKernArgs<First> k{};
    stage_record(c, stage, p, total, k.a);
    return stage_launch(c, stage, entry, k, g);
}

}  // namespace

th_status thi::fragment_stage_run(th_context *c, const FragmentStage &stage, const th::DepositParams &p, uint32_t total)
{
    const StageGrid grid{total, 0, 0};
    if (p.mode == 2) {
        TH_REQUIRE(p.keys && !p.keys64 && p.colors, "the stages of both passes over one rasterisation: 32-bit texel keys, two varyings a fragment");
        return stage_launch_pair<FragmentArgs>(c, &stage, p, total, kFragmentPair, grid);
    }
    if (!stage_reads_line(&stage)) return stage_launch_one<FragmentArgs>(c, stage, p, total, p.keys64 ? kFragmentBand : kFragmentStream, nullptr, grid);
    // the fragments' line records first, beside the keys and varyings the scatter has just written (mode 2: no stage reads them)
    TH_REQUIRE(c->dep_fraglines && c->dep_capacity >= total && (p.keys64 || p.keys), "a stage that reads the line: a record per fragment, keys to read the texels from");
    th::launch_fragment_lines(p, c->dep_fraglines, c->stream);
    TH_HIP(hipGetLastError());
    return stage_launch_one<FragmentArgs>(c, stage, p, total, p.keys64 ? kFragmentLineBand : kFragmentLine, c->dep_fraglines, grid);
}

th_status thi::fragment_stage_run_bins(th_context *c, const FragmentStage &stage, const th::DepositParams &p, bool crowded, bool program)
{
    TH_REQUIRE(p.frag_keys && p.colors && p.nbins, "a fragment stage over the bins: a store to run over");
    const StageGrid grid{0, (int)p.nbins, crowded ? kBinsStageDealCrowded : kBinsStageDeal};
    if (p.mode == 2) {
        TH_REQUIRE(c->bins_pairs && p.colors == c->bins_colors, "the stages of both passes over the bins: a store of two varyings a place");
        return stage_launch_pair<FragmentBinsArgs>(c, &stage, p, 0, kFragmentPairBins, grid);
    }
    if (!stage_reads_line(&stage)) return stage_launch_one<FragmentBinsArgs>(c, stage, p, 0, kFragmentBins, nullptr, grid);
    // the places' line records first, behind the emitting pass on this stream (bins_pass_emit reserved them for this store)
    const size_t places = ((size_t)p.nbins * th::kBinReplicas + p.pool_pages) * th::kBinPage;
    TH_REQUIRE(c->opt.line_bins && c->bins_line_ends && c->bins_lines && c->bins_lines_places >= places && p.frag_keys == c->bins_keys,
               "a stage that reads the line over the bins: the lines' endpoints and a record per place of the store");
    th::launch_fragment_line_ends(p, c->bins_line_ends, c->stream, program);
    th::launch_fragment_lines_bins(p, c->bins_line_ends, c->bins_lines, grid.deal, c->stream);
    TH_HIP(hipGetLastError());
    return stage_launch_one<FragmentBinsArgs>(c, stage, p, 0, kFragmentLineBins, c->bins_lines, grid);
}

extern "C" {

th_status th_fragment_program_compile(const char *source, const char *name, th_program **out)
{
    if (th_status s = program_compile(kFragmentProgram, std::string(kTaps) + "\n" + kBinsWalk + "\n" + kPrelude + "\n" + kPairPrelude, source, name, out)) return s;
    // who pays for the line records: decided here, once (the compiler has accepted the text; an identifier in a comment counts)
    (*out)->reads_line = names_identifier(source, "th_line");
    // ... and whether, as the view pass's stage, it keeps th_draw_stages_pair to two passes (th_flow_res is another identifier)
    (*out)->names_flow = names_identifier(source, "th_flow");
    return TH_OK;
}

// One pass of draw() with the stages of `s`, through the body every local pass goes through (pass_run): with a fragment stage
// deposit_prepare leaves the bins and the frame's pipeline count alone, deposit_run reuses nothing and calls the stage between
// its scatter and its sort - or, under TH_OPT_STAGE_BINS, the pass takes the pipeline it would take without the stage, and a
// binned one runs the stage over its page store.  What such a pass leaves of its lines (c->drawn) is no other pass's to reuse.
th_status th_draw_stages_run(th_context *c, const th_draw_stages *s, int32_t pass, uint64_t *fragments)
{
    if (th_status st = stages_args(c, s, pass, "th_draw_stages_run", "th_flow_deposit / th_view_draw")) return st;
    if (th_status st = use(c, pass == TH_PASS_VIEW)) return st;
    if (th_status st = refuse_band(c, "draw stages", "a band's pass goes through th_draw_stages_emit and the owners' exchange")) return st;
    FragmentStage stage{}; PassSpec spec;
    if (th_status st = stages_pass(c, s, pass, stage, spec)) return st;
    draw_moves_nothing(c);
    return pass_run(c, spec, fragments);
}

// Both passes of draw() with a caller's fragment stage in either or both.  Where one rasterisation gives the bits of the two
// passes run one after the other it is th_draw's pass (p.mode == 2: every fragment carries both passes' varyings side by side)
// with both stages handed down as one argument - deposit_run / bins_pass_emit call fragment_stage_run / _run_bins where the
// fragments lie, and those launch each stage over its half, the flow pass's first, before anything blends.  That is so when
// the lines are the library's own in both passes (no vertex program: a draw program in mode 2 is not built), both passes draw
// them equally wide, no stage reads th_line (the line records lie beside one varying a fragment) and the VIEW pass's stage does
// not name th_flow: run in sequence it would see the field after the flow pass has blended into it, here every stage runs
// before anything blends.  Every other pair of slots is the two passes through pass_run, one after the other.
th_status th_draw_stages_pair(th_context *c, const th_draw_stages *flow, const th_draw_stages *view, uint64_t *fragments, int32_t *rasterisations)
{
    const char *const entry = "th_draw_stages_pair";
    TH_REQUIRE(c, "null context");
    TH_REQUIRE(flow && view, "null stages");
    TH_REQUIRE(flow->fragment || view->fragment, "%s with no fragment program in either pass: both passes with the library's fragment stage are th_draw, or th_draw_stages_run pass by pass", entry);
    const th_draw_stages *const slots[2] = {flow, view};
    for (int32_t pass = 0; pass < 2; ++pass) {
        const th_draw_stages *s = slots[pass];
        if (th_status st = stage_args(s->vertex, kDrawProgram, entry, "vertex", s->vertex_uniforms, s->vertex_uniform_bytes)) return st;
        if (th_status st = stage_args(s->fragment, kFragmentProgram, entry, "fragment", s->fragment_uniforms, s->fragment_uniform_bytes)) return st;
        TH_REQUIRE(s->vertex || s->builtin, "%s: the %s pass without a vertex program needs `builtin`: the %s of the library's vertex stage", entry,
                   pass == TH_PASS_VIEW ? "view" : "flow", pass == TH_PASS_VIEW ? "th_render_uniforms" : "th_deposit_uniforms");
    }
    const th_deposit_uniforms *du = static_cast<const th_deposit_uniforms *>(flow->builtin);
    const th_render_uniforms *ru = static_cast<const th_render_uniforms *>(view->builtin);
    if (!flow->vertex && !view->vertex) if (th_status st = shared_uniforms(du, ru)) return st;
    if (th_status st = use(c)) return st;
    if (th_status st = refuse_band(c, "the draw stages of both passes", "a band's passes go through th_draw_stages_emit and the owners' exchange, pass by pass")) return st;
    const bool one = !flow->vertex && !view->vertex && drawn_line_width(c, TH_PASS_FLOW) == drawn_line_width(c, TH_PASS_VIEW) &&
                     !(flow->fragment && flow->fragment->reads_line) && !(view->fragment && (view->fragment->reads_line || view->fragment->names_flow));
    if (rasterisations) *rasterisations = one ? 1 : 2;
    draw_moves_nothing(c);
    if (!one) {
        // (*fragments: the flow pass's, as th_draw reports them of two widths; th_draw_query has the view pass's afterwards)
        for (int32_t pass = 0; pass < 2; ++pass) {
            FragmentStage stage{}; PassSpec spec;
            if (th_status st = stages_pass(c, slots[pass], pass, stage, spec)) return st;
            if (th_status st = pass_run(c, spec, pass == TH_PASS_FLOW ? fragments : nullptr)) return st;
        }
        return TH_OK;
    }
    FragmentStage pair[2] = {};
    for (int32_t pass = 0; pass < 2; ++pass) {
        const th_draw_stages *s = slots[pass];
        pair[pass].pass = pass;
        if (!s->fragment) continue;                      // (module null: this half is blended as the library interpolated it)
        if (th_status st = program_loaded(c, s->fragment, &pair[pass].module)) return st;
        pair[pass].uniforms = s->fragment_uniforms; pair[pass].uniform_bytes = s->fragment_uniform_bytes;
    }
    if (th_status st = view_storage(c)) return st;
    const th_status ran = draw_pass(c, fragments, false, pair, [&](th::DepositParams &p, bool first, bool *bins) -> th_status {
        if (th_status st = deposit_prepare(c, du, p, first, bins, false, pair)) return st;
        p.mode = 2;
        view_fields(c, ru, p);
        p.view = c->view;
        return TH_OK;
    });
    c->drawn.valid = false;          // (deposit_run has said what it left: no built-in pass reuses the lines of a pass with a caller's stage)
    return ran;
}

// ... and of a row band (a whole-texture context: the band of all rows), through pass_emit: emit_parted calls the stage behind its
// scatter, before it parts the fragments by owner.  Like th_draw_program_emit it tells th_draw_query what it emitted.  (use(): the
// view pass keeps what a step left for the draw only with a vertex program - as th_draw_program_emit does and th_view_emit does not)
th_status th_draw_stages_emit(th_context *c, const th_draw_stages *s, int32_t pass, uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (th_status st = stages_args(c, s, pass, "th_draw_stages_emit", "th_deposit_emit / th_view_emit")) return st;
    TH_REQUIRE(count && keys_dev && colors_dev, "null outputs");
    if (th_status st = use(c, pass == TH_PASS_VIEW && s->vertex)) return st;
    *count = 0; *keys_dev = nullptr; *colors_dev = nullptr;
    FragmentStage stage{}; PassSpec spec;
    if (th_status st = stages_pass(c, s, pass, stage, spec)) return st;
    const th_status emitted = pass_emit(c, spec, count, keys_dev, colors_dev);
    if (emitted == TH_OK) draw_streamed(c, *count);
    return emitted;
}

}  // extern "C"
