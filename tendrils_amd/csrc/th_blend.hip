// th_blend.hip - the demo's colour-map blend: Blend.draw(tendrils.colorMap) (src/screen/blend/index.js, main.frag,
// src/blend/sum.glsl; src/demo.main.js:541-560, 1068-1079) as one pass over the colour map, and the caller's textures it
// reads (AudioTexture, src/audio/data-texture.js; any FBO a host blends in).  Semantics as captured from the reference's own
// Blend (tests/golden/blend_*.npz, tests/blend_restatement.py):
//   uv = gl_FragCoord.xy / resolution of the TARGET; every view NEAREST / CLAMP_TO_EDGE at that uv, whatever its shape;
//   a float texture is tapped at clamp(floor(uv * size)) in fp32 (dep_nearest), an RGBA8 one through the 16-bit fixed-point
//   coordinate the captured GL uses for 8-bit textures (nearest_texel_fx16, as the optical-flow pass reads its frames);
//   a one-channel float texture arrives as (L, L, L, 1); RGBA8 as (c * 257) * (1 / 65535);
//   sum += vec4(color.rgb * (color.a * alpha), color.a * alpha) view by view; nothing is clamped;
//   Blend.draw leaves the GL's blend state alone: after a Tendrils.step() the target receives
//   sum * sum.a + dst * (1 - sum.a) (dst = 0 after the clear), before the first one `sum` itself.
// Memory-bound: 16 B stored per texel of the colour map, the taps come from textures far smaller than it (or, at most, as
// large) through L2.  No LDS, no atomics.
#include "th_ctx.hpp"

using namespace thi;

namespace {

struct BlendView {
    const void *texels;
    int32_t w, h, format;        // TH_TEX_*
    float alpha;
};

// by value, as the kernel's argument: the format switch and the view loop are uniform, the table is read through scalar loads
struct BlendParams {
    float4 *dst;                 // the colour map, w x h
    uint32_t w, count;
    float wf, hf;
    int32_t n;                   // views
    int32_t gl_blend;            // SRC_ALPHA / ONE_MINUS_SRC_ALPHA over the destination (else: the sum is stored)
    int32_t keep;                // the destination is read (clear = 0); else it is the cleared target, zeros
    BlendView v[TH_MAX_BLEND_VIEWS];
};

// texture2D(views[i], uv)
TH_D float4 blend_tap(const BlendView &v, float uvx, float uvy)
{
    if (v.format == TH_TEX_RGBA8) {
        const uchar4 t = static_cast<const uchar4 *>(v.texels)[(size_t)th::nearest_texel_fx16(uvy, (unsigned)v.h) * v.w +
                                                               th::nearest_texel_fx16(uvx, (unsigned)v.w)];
        return make_float4(th::unorm8(t.x), th::unorm8(t.y), th::unorm8(t.z), th::unorm8(t.w));
    }
    const size_t at = (size_t)th::dep_nearest(uvy, v.h) * v.w + th::dep_nearest(uvx, v.w);
    if (v.format == TH_TEX_L32F) {
        const float l = static_cast<const float *>(v.texels)[at];
        return make_float4(l, l, l, 1.0f);
    }
    return static_cast<const float4 *>(v.texels)[at];
}

// one lane per texel of the target, neighbouring lanes neighbouring texels of a row: every store is 16 B per lane, coalesced
__global__ __launch_bounds__(256) void colormap_blend_kernel(const BlendParams p)
{
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < p.count; idx += gridDim.x * 256u) {
        const uint32_t y = idx / p.w, x = idx - y * p.w;
        const float uvx = ((float)x + 0.5f) / p.wf, uvy = ((float)y + 0.5f) / p.hf;      // gl_FragCoord.xy / resolution
        float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int i = 0; i < p.n; ++i) {
            const float4 c = blend_tap(p.v[i], uvx, uvy);
            const float a = c.w * p.v[i].alpha;                                           // sum + preAlpha(color.rgb, color.a * alpha)
            sum = make_float4(sum.x + c.x * a, sum.y + c.y * a, sum.z + c.z * a, sum.w + a);
        }
        if (p.gl_blend) {
            const float4 d = p.keep ? p.dst[idx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float sa = sum.w, ia = 1.0f - sa;
            sum = make_float4(sum.x * sa + d.x * ia, sum.y * sa + d.y * ia, sum.z * sa + d.z * ia, sum.w * sa + d.w * ia);
        }
        p.dst[idx] = sum;
    }
}

constexpr uint32_t kBlendViews = view_bit(TH_VIEW_TEXTURE) | view_bit(TH_VIEW_FRAMES) | view_bit(TH_VIEW_SPAWN_IMAGE);      // what a blend sums

size_t texel_bytes(int32_t format) { return format == TH_TEX_RGBA32F ? sizeof(float4) : 4; }

// a float texture: a side below 2^24 (its taps are computed in fp32, as the flow's and the spawn image's); an 8-bit one: what
// its fixed-point tap holds (tap_size_ok)
bool shape_ok(int32_t format, int32_t w, int32_t h)
{
    const int32_t side = format == TH_TEX_RGBA8 ? kRgba8MaxSide : (1 << 24) - 1;
    return w > 0 && h > 0 && w <= side && h <= side && (uint64_t)w * h < (1ull << 28);
}

}  // namespace

namespace thi {

// the colour map as the reference has it before anyone sets one: a 1 x 1 float FBO, zeros (src/index.js:94-96)
th_status colormap_storage(th_context *c)
{
    if (c->colormap) return TH_OK;
    if (th_status s = c->colormap.alloc(1)) return s;
    c->cmap_w = c->cmap_h = 1;
    TH_HIP(hipMemsetAsync(c->colormap, 0, sizeof(float4), c->stream));
    return TH_OK;
}

th_status view_image(th_context *c, int32_t source, int32_t index, uint32_t accepted, const char *noun, int32_t ordinal, Image *out)
{
    // "unit 3: ..." / "target: ..." (put together only when something is wrong)
    auto refuse = [&](const char *fmt, auto... args) {
        const std::string who = ordinal < 0 ? std::string(noun) : std::string(noun) + " " + std::to_string(ordinal);
        return fail(TH_ERR_INVALID, (who + ": " + fmt).c_str(), args...);
    };
    if (source < 0 || source >= 32 || !(accepted & view_bit(source))) return refuse("unknown source %d", source);
    if (source == TH_VIEW_BUFFER || source == TH_VIEW_SCREEN) if (th_status s = view_storage(c)) return s;
    if (source == TH_VIEW_TEXTURE) {
        if (index < 0 || index >= TH_MAX_TEXTURES) return refuse("texture slot %d outside 0..%d", index, TH_MAX_TEXTURES - 1);
        const th_context::Texture &t = c->textures[index];
        if (!t.texels) return refuse("texture slot %d is empty (call th_texture_upload)", index);
        *out = Image{t.texels.get(), t.w, t.h, t.format};
    } else if (source == TH_VIEW_FRAMES) {
        if (index != 0 && index != 1) return refuse("frame buffer %d (OpticalFlow has buffers 0 and 1)", index);
        if (!c->frames[index]) return refuse("no frame buffers (call th_frames_resize)");
        *out = Image{c->frames[index].get(), c->frw, c->frh, TH_TEX_RGBA8};
    } else if (source == TH_VIEW_SPAWN_IMAGE) {
        if (!c->image) return refuse("no spawn image (call th_spawn_image_upload)");
        *out = Image{c->image.get(), c->iw, c->ih, TH_TEX_RGBA32F};
    } else if (source == TH_VIEW_BUFFER) {
        if (index < 0 || index >= (int32_t)c->view_ring.size()) return refuse("no view buffer %d (there are %zu)", index, c->view_ring.size());
        *out = Image{c->view_ring[(size_t)index], c->view_w, c->view_h, TH_TEX_RGBA8};
    } else if (source == TH_VIEW_SCREEN) {
        *out = Image{c->view_screen.get(), c->view_w, c->view_h, TH_TEX_RGBA8};
    } else if (source == TH_VIEW_COLORMAP) {
        if (th_status s = colormap_storage(c)) return s;
        *out = Image{c->colormap.get(), c->cmap_w, c->cmap_h, TH_TEX_RGBA32F};
    } else {                                    // TH_VIEW_FLOW
        if (!c->flow) return refuse("no flow field");
        *out = Image{c->flow.get(), c->fw, c->fh, TH_TEX_RGBA32F};
    }
    return TH_OK;
}

}  // namespace thi

extern "C" {

th_status th_texture_upload(th_context *c, int32_t slot, int32_t format, const void *texels, int32_t w, int32_t h)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(slot >= 0 && slot < TH_MAX_TEXTURES, "texture slot %d outside 0..%d", slot, TH_MAX_TEXTURES - 1);
    TH_REQUIRE(format == TH_TEX_RGBA32F || format == TH_TEX_RGBA8 || format == TH_TEX_L32F, "unknown texture format %d", format);
    TH_REQUIRE(texels && shape_ok(format, w, h), "bad texture %dx%d (an RGBA8 texture: at most 65536 a side) or null texels", w, h);
    th_context::Texture &t = c->textures[slot];
    const size_t bytes = (size_t)w * h * texel_bytes(format);
    if (w != t.w || h != t.h || format != t.format) {      // (a blend under way may still read the old texels)
        if (th_status s = image_reshape(c, t.texels, t.w, t.h, w, h, texel_bytes(format))) return s;
        t.format = format;
    }
    // (pageable host memory: the copy is staged by the runtime; the caller may reuse `texels` when the call returns, as after
    // th_frames_upload)
    return image_upload(c, t.texels, texels, bytes);
}

th_status th_texture_download(th_context *c, int32_t slot, void *texels)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(slot >= 0 && slot < TH_MAX_TEXTURES, "texture slot %d outside 0..%d", slot, TH_MAX_TEXTURES - 1);
    const th_context::Texture &t = c->textures[slot];
    TH_REQUIRE(texels && t.texels, "texture slot %d is empty (call th_texture_upload) or null texels", slot);
    return image_download(c, texels, t.texels, (size_t)t.w * t.h * texel_bytes(t.format));
}

th_status th_colormap_resize(th_context *c, int32_t w, int32_t h)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(w > 0 && h > 0 && w < (1 << 24) && h < (1 << 24) && (uint64_t)w * h < (1ull << 28), "bad colour map %dx%d", w, h);
    if (c->colormap && w == c->cmap_w && h == c->cmap_h) return TH_OK;      // gl-fbo: same shape is a no-op
    if (th_status s = image_reshape(c, c->colormap, c->cmap_w, c->cmap_h, w, h)) return s;
    TH_HIP(hipMemsetAsync(c->colormap, 0, (size_t)w * h * sizeof(float4), c->stream));
    return TH_OK;
}

th_status th_colormap_shape(th_context *c, int32_t *w, int32_t *h)
{
    TH_REQUIRE(c && w && h, "null argument");
    *w = c->colormap ? c->cmap_w : 1; *h = c->colormap ? c->cmap_h : 1;
    return TH_OK;
}

th_status th_colormap_download(th_context *c, float *rgba)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(rgba, "null pixels");
    if (th_status s = colormap_storage(c)) return s;
    return image_download(c, rgba, c->colormap, (size_t)c->cmap_w * c->cmap_h * sizeof(float4));
}

// Writes the colour map (and reads it with clear = 0) and nothing else: the ring, its slot orders, the statistics a fused
// launch took and the line records of the last draw pass stay as they are (use(c, true)).
th_status th_colormap_blend(th_context *c, const th_blend_view *views, int32_t n, int32_t gl_blend, int32_t clear)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(views && n >= 1 && n <= TH_MAX_BLEND_VIEWS, "a blend takes 1..%d views (got %d)", TH_MAX_BLEND_VIEWS, n);
    BlendParams p{};
    for (int32_t i = 0; i < n; ++i) {
        Image img;
        if (th_status s = view_image(c, views[i].source, views[i].index, kBlendViews, "view", i, &img)) return s;
        // (the frames alone: an RGBA8 texture beyond the rule is refused where it is uploaded - shape_ok)
        TH_REQUIRE(views[i].source != TH_VIEW_FRAMES || tap_size_ok(img), "view %d: %dx%d frames are beyond what a blend samples (65536 a side)", i, img.w, img.h);
        p.v[i] = BlendView{img.texels, img.w, img.h, img.format, views[i].alpha};
    }
    if (th_status s = colormap_storage(c)) return s;
    p.dst = c->colormap;
    p.w = (uint32_t)c->cmap_w; p.count = (uint32_t)((size_t)c->cmap_w * c->cmap_h);
    p.wf = (float)c->cmap_w; p.hf = (float)c->cmap_h;
    p.n = n; p.gl_blend = gl_blend != 0; p.keep = clear == 0;
    // a memory-bound pass: the grid of the streaming passes, the rest of the texels by its stride
    hipLaunchKernelGGL(colormap_blend_kernel, dim3(th::grid_for(p.count, 8)), dim3(256), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // extern "C"
