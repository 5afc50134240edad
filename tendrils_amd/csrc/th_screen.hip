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
struct KernArgs {
    ScreenArgs a;
    alignas(16) unsigned char u[kUniformBytes];
};
static_assert(sizeof(ScreenUnit) == 24 && sizeof(ScreenArgs) == 240 && offsetof(KernArgs, u) == 240 && sizeof(KernArgs) == 240 + kUniformBytes,
              "launch record: layout shared with th_screen_prelude.inc");

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
    if (views) if (th_status s = view_storage(c)) return s;
    KernArgs k{};
    ScreenArgs &a = k.a;
    if (target == TH_SCREEN_TARGET_VIEW) {
        a.dst = c->view; a.w = (uint32_t)c->view_w; a.h = (uint32_t)c->view_h; a.format = TH_TEX_RGBA8;
    } else if (target == TH_SCREEN_TARGET_COLORMAP) {
        if (th_status s = colormap_storage(c)) return s;
        a.dst = c->colormap.get(); a.w = (uint32_t)c->cmap_w; a.h = (uint32_t)c->cmap_h; a.format = TH_TEX_RGBA32F;
    } else if (target == TH_SCREEN_TARGET_TEXTURE) {
        TH_REQUIRE(target_index >= 0 && target_index < TH_MAX_TEXTURES, "target: texture slot %d outside 0..%d", target_index, TH_MAX_TEXTURES - 1);
        const th_context::Texture &t = c->textures[target_index];
        TH_REQUIRE(t.texels, "target: texture slot %d is empty (call th_texture_upload)", target_index);
        TH_REQUIRE(t.format == TH_TEX_RGBA32F || t.format == TH_TEX_RGBA8, "target: texture slot %d holds a one-channel texture (a pass renders into RGBA32F or RGBA8)", target_index);
        a.dst = t.texels.get(); a.w = (uint32_t)t.w; a.h = (uint32_t)t.h; a.format = t.format;
    } else return fail(TH_ERR_INVALID, "unknown screen target %d", target);
    TH_REQUIRE((uint64_t)a.w * a.h <= 0x7fffffffull, "a %ux%u target is beyond what a screen pass indexes", a.w, a.h);
    a.count = a.w * a.h;
    for (int32_t i = 0; i < n_units; ++i) {
        ScreenUnit &v = a.unit[i];
        const th_screen_unit &in = units[i];
        if (in.source == TH_VIEW_TEXTURE) {
            TH_REQUIRE(in.index >= 0 && in.index < TH_MAX_TEXTURES, "unit %d: texture slot %d outside 0..%d", i, in.index, TH_MAX_TEXTURES - 1);
            const th_context::Texture &t = c->textures[in.index];
            TH_REQUIRE(t.texels, "unit %d: texture slot %d is empty (call th_texture_upload)", i, in.index);
            v.texels = t.texels.get(); v.w = t.w; v.h = t.h; v.format = t.format;
        } else if (in.source == TH_VIEW_FRAMES) {
            TH_REQUIRE(in.index == 0 || in.index == 1, "unit %d: frame buffer %d (OpticalFlow has buffers 0 and 1)", i, in.index);
            TH_REQUIRE(c->frames[in.index], "unit %d: no frame buffers (call th_frames_resize)", i);
            v.texels = c->frames[in.index].get(); v.w = c->frw; v.h = c->frh; v.format = TH_TEX_RGBA8;
        } else if (in.source == TH_VIEW_SPAWN_IMAGE) {
            TH_REQUIRE(c->image, "unit %d: no spawn image (call th_spawn_image_upload)", i);
            v.texels = c->image.get(); v.w = c->iw; v.h = c->ih; v.format = TH_TEX_RGBA32F;
        } else if (in.source == TH_VIEW_BUFFER) {
            TH_REQUIRE(in.index >= 0 && in.index < (int32_t)c->view_ring.size(), "unit %d: no view buffer %d (there are %zu)", i, in.index, c->view_ring.size());
            v.texels = c->view_ring[(size_t)in.index]; v.w = c->view_w; v.h = c->view_h; v.format = TH_TEX_RGBA8;
        } else if (in.source == TH_VIEW_SCREEN) {
            v.texels = c->view_screen.get(); v.w = c->view_w; v.h = c->view_h; v.format = TH_TEX_RGBA8;
        } else if (in.source == TH_VIEW_COLORMAP) {
            if (th_status s = colormap_storage(c)) return s;
            v.texels = c->colormap.get(); v.w = c->cmap_w; v.h = c->cmap_h; v.format = TH_TEX_RGBA32F;
        } else if (in.source == TH_VIEW_FLOW) {
            TH_REQUIRE(c->flow, "unit %d: no flow field", i);
            v.texels = c->flow.get(); v.w = c->fw; v.h = c->fh; v.format = TH_TEX_RGBA32F;
        } else return fail(TH_ERR_INVALID, "unit %d: unknown source %d", i, in.source);
        TH_REQUIRE(v.format != TH_TEX_RGBA8 || (v.w <= 65536 && v.h <= 65536), "unit %d: a %dx%d RGBA8 texture is beyond what a tap samples (65536 a side)", i, v.w, v.h);
        // GL's feedback loop - undefined there, a race here: the pass would read texels other lanes are writing
        TH_REQUIRE(v.texels != a.dst, "unit %d (%s %d) is the memory this pass renders into: a pass cannot sample its own target", i, kSourceNames[in.source], in.index);
    }
    a.n_units = n_units; a.gl_blend = gl_blend != 0;
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    if (!a.count) return TH_OK;
    if (uniform_bytes) memcpy(k.u, uniforms, uniform_bytes);
    // the record and the uniform block travel in the kernel's argument segment (th_program_run).  A memory-bound pass: at most
    // 256 CUs x 8 workgroups, the rest of the texels by the grid's stride
    size_t bytes = sizeof k;
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &k, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
    const uint32_t blocks = (a.count + 255u) / 256u, cap = 256u * 8u;
    TH_HIP(hipModuleLaunchKernel(m->fn, blocks < cap ? blocks : cap, 1, 1, 256, 1, 1, 0, c->stream, nullptr, extra));
    return TH_OK;
}

}  // extern "C"
