// th_screen.hip - screen programs: a caller's HIP pass over a view image, the colour map or a caller's texture.  The reference's
// other seam (th_program.hip has the first): Screen.render() (src/screen/index.js) draws one full-screen triangle with
// whatever shader is bound into whatever framebuffer is bound - the demo's frame ends with one, its blur over
// tendrils.buffers[0] into the screen (src/demo.main.js:1084-1102).  Here the caller's shader is HIP source for one device
// function, th_screen (th_screen_prelude.inc), compiled for gfx950 at run time like a state program (th_program.hip:
// program_compile) and run once per texel of the target; the harness in the prelude blends or stores what it returns.
#include "th_ctx.hpp"

using namespace thi;

namespace {

// the tap and rounding rules as text (th_taps.inc: the library's kernels compile the same lines), then the prelude
#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#undef TH_TAPS
const char kPrelude[] =
#include "th_screen_prelude.inc"
    ;

// the launch record (th_screen_prelude.inc: th_screen_args, th_program_uniform_block - the same layout)
struct ScreenUnit {
    const void *texels;
    int32_t w, h, format, reserved;
};
struct ScreenArgs {
    void *dst;
    uint32_t w, h, count;
    int32_t format;
    int32_t gl_blend;
    int32_t n_units;
    uint32_t reserved[4];
    ScreenUnit unit[TH_MAX_BLEND_VIEWS];
};
using KernArgs = ProgramKernArgs<ScreenArgs>;
static_assert(sizeof(ScreenUnit) == 24 && sizeof(ScreenArgs) == 240 && offsetof(KernArgs, u) == 240 && sizeof(KernArgs) == 240 + kUniformBytes,
              "launch record: layout shared with th_screen_prelude.inc");

constexpr uint32_t kScreenViews = view_bit(TH_VIEW_FLOW + 1) - 1u;      // a unit is any of the sources, TH_VIEW_TEXTURE .. TH_VIEW_FLOW
const char *const kSourceNames[] = {"TH_VIEW_TEXTURE", "TH_VIEW_FRAMES", "TH_VIEW_SPAWN_IMAGE", "TH_VIEW_BUFFER", "TH_VIEW_SCREEN", "TH_VIEW_COLORMAP", "TH_VIEW_FLOW"};

}  // namespace

extern "C" {

th_status th_screen_program_compile(const char *source, const char *name, th_program **out)
{
    return program_compile(kScreenProgram, std::string(kTaps) + "\n" + kPrelude, source, name, out);
}

// Writes its target (and reads it with gl_blend = 1) and nothing else: the ring, its slot orders, the statistics a fused
// launch took and the line records of the last draw pass stay as they are (use(c, true)).
th_status th_screen_run(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes,
                        const th_screen_unit *units, int32_t n_units, int32_t target, int32_t target_index, int32_t gl_blend)
{
    if (th_status s = use(c, true)) return s;
    if (th_status s = program_run_args(prog, kScreenProgram, "th_screen_run", uniforms, uniform_bytes)) return s;
    TH_REQUIRE(n_units >= 0 && n_units <= TH_MAX_BLEND_VIEWS && (units || n_units == 0), "a screen pass takes 0..%d units (got %d) - or null units", TH_MAX_BLEND_VIEWS, n_units);
    const bool band = c->cfg.height != c->cfg.global_height;
    bool views = target == TH_SCREEN_TARGET_VIEW;
    for (int32_t i = 0; i < n_units; ++i) views = views || units[i].source == TH_VIEW_BUFFER || units[i].source == TH_VIEW_SCREEN;
    if (target == TH_SCREEN_TARGET_VIEW && band)
        return fail(TH_ERR_UNSUPPORTED, "screen pass into the view on a row-band shard (%d of %d rows): a band's view image holds only what it owns", c->cfg.height, c->cfg.global_height);
    if (views) if (th_status s = view_storage(c)) return s;      // (here for the order of the refusals, and before a.dst is taken: view_image's own call then finds the storage there)
    KernArgs k{};
    ScreenArgs &a = k.a;
    if (target == TH_SCREEN_TARGET_VIEW) {
        a.dst = c->view; a.w = (uint32_t)c->view_w; a.h = (uint32_t)c->view_h; a.format = TH_TEX_RGBA8;
    } else if (target == TH_SCREEN_TARGET_COLORMAP) {
        if (th_status s = colormap_storage(c)) return s;
        a.dst = c->colormap.get(); a.w = (uint32_t)c->cmap_w; a.h = (uint32_t)c->cmap_h; a.format = TH_TEX_RGBA32F;
    } else if (target == TH_SCREEN_TARGET_TEXTURE) {
        Image t;
        if (th_status s = view_image(c, TH_VIEW_TEXTURE, target_index, view_bit(TH_VIEW_TEXTURE), "target", -1, &t)) return s;
        TH_REQUIRE(t.format == TH_TEX_RGBA32F || t.format == TH_TEX_RGBA8, "target: texture slot %d holds a one-channel texture (a pass renders into RGBA32F or RGBA8)", target_index);
        a.dst = const_cast<void *>(t.texels); a.w = (uint32_t)t.w; a.h = (uint32_t)t.h; a.format = t.format;
    } else return fail(TH_ERR_INVALID, "unknown screen target %d", target);
    TH_REQUIRE((uint64_t)a.w * a.h <= 0x7fffffffull, "a %ux%u target is beyond what a screen pass indexes", a.w, a.h);
    a.count = a.w * a.h;
    for (int32_t i = 0; i < n_units; ++i) {
        Image v;
        if (th_status s = view_image(c, units[i].source, units[i].index, kScreenViews, "unit", i, &v)) return s;
        TH_REQUIRE(tap_size_ok(v), "unit %d: a %dx%d RGBA8 texture is beyond what a tap samples (65536 a side)", i, v.w, v.h);
        // GL's feedback loop - undefined there, a race here: the pass would read texels other lanes are writing
        TH_REQUIRE(v.texels != a.dst, "unit %d (%s %d) is the memory this pass renders into: a pass cannot sample its own target", i, kSourceNames[units[i].source], units[i].index);
        a.unit[i] = ScreenUnit{v.texels, v.w, v.h, v.format, 0};
    }
    a.n_units = n_units; a.gl_blend = gl_blend != 0;
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    if (!a.count) return TH_OK;
    // the record and the uniform block travel in the kernel's argument segment; a memory-bound pass (program_launch)
    k.set_uniforms(uniforms, uniform_bytes);
    return program_launch(c, m->entry[kScreenRun], a.count, k);
}

}  // extern "C"
