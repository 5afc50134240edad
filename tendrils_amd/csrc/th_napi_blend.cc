// th_napi_blend.cc - a small N-API addon of its own (lib/tendrils_blend.node) binding the colour-map blend of
// include/tendrils_hip.h for the Node host (tendrils_amd/js/blend.js): th_texture_upload, th_colormap_resize / _shape /
// _blend / _download (th_texture_download, a read-back for tests, is left to the ctypes binding).  Like the flow-lines,
// sharded-spawn and user-program addons it takes the context handle the main addon (th_napi.cc) hands out - an external
// wrapping a th_context ** - and leaves the main addon's exports as they are.
#include <node_api.h>

#include <cstdint>
#include <string>

#include "tendrils_hip.h"

namespace {

napi_value fail(napi_env env, th_status st, const char *what)
{
    const std::string msg = std::string("tendrils_hip ") + what + ": status " + std::to_string((int)st) + ": " + th_last_error();
    napi_throw_error(env, nullptr, msg.c_str());
    return nullptr;
}

napi_value bad(napi_env env, const char *what)
{
    napi_throw_type_error(env, nullptr, what);
    return nullptr;
}

napi_value undefined(napi_env env)
{
    napi_value undef;
    napi_get_undefined(env, &undef);
    return undef;
}

th_context *context(napi_env env, napi_value v)
{
    void *slot = nullptr;
    if (napi_get_value_external(env, v, &slot) != napi_ok || !slot) return nullptr;
    return *static_cast<th_context **>(slot);         // (null once the handle was destroyed)
}

// a typed array of one element type: its data and length in elements
bool typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *n)
{
    bool is = false;
    napi_typedarray_type type;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return false;
    if (napi_get_typedarray_info(env, v, &type, n, data, nullptr, nullptr) != napi_ok) return false;
    return type == want || (want == napi_uint8_array && type == napi_uint8_clamped_array);
}

bool ints(napi_env env, const napi_value *argv, int n, int32_t *out)
{
    for (int k = 0; k < n; ++k)
        if (napi_get_value_int32(env, argv[k], &out[k]) != napi_ok) return false;
    return true;
}

size_t texel_elements(int32_t format) { return format == TH_TEX_L32F ? 1 : 4; }      // floats (bytes: RGBA8) a texel

// textureUpload(handle, slot, format, texels: Float32Array (RGBA32F, L32F) | Uint8Array (RGBA8), w, h)
napi_value TextureUpload(napi_env env, napi_callback_info info)
{
    size_t argc = 6;
    napi_value argv[6];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 6) return bad(env, "textureUpload: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "textureUpload: bad context");
    int32_t slot, format, shape[2];
    if (!ints(env, argv + 1, 1, &slot) || !ints(env, argv + 2, 1, &format) || !ints(env, argv + 4, 2, shape)) return bad(env, "textureUpload: bad arguments");
    if (format != TH_TEX_RGBA32F && format != TH_TEX_RGBA8 && format != TH_TEX_L32F) return bad(env, "textureUpload: unknown format");
    void *data = nullptr;
    size_t n = 0;
    if (!typed(env, argv[3], format == TH_TEX_RGBA8 ? napi_uint8_array : napi_float32_array, &data, &n))
        return bad(env, "textureUpload: the texels are a Float32Array (RGBA32F, L32F) or a Uint8Array (RGBA8)");
    if (shape[0] <= 0 || shape[1] <= 0 || n < (size_t)shape[0] * (size_t)shape[1] * texel_elements(format))
        return bad(env, "textureUpload: fewer texels than the shape holds");
    if (th_status s = th_texture_upload(ctx, slot, format, data, shape[0], shape[1])) return fail(env, s, "th_texture_upload");
    return undefined(env);
}

// colormapResize(handle, w, h)
napi_value ColormapResize(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3) return bad(env, "colormapResize: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "colormapResize: bad context");
    int32_t shape[2];
    if (!ints(env, argv + 1, 2, shape)) return bad(env, "colormapResize: bad arguments");
    if (th_status s = th_colormap_resize(ctx, shape[0], shape[1])) return fail(env, s, "th_colormap_resize");
    return undefined(env);
}

// colormapShape(handle) -> [w, h]
napi_value ColormapShape(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1) return bad(env, "colormapShape: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "colormapShape: bad context");
    int32_t w = 0, h = 0;
    if (th_status s = th_colormap_shape(ctx, &w, &h)) return fail(env, s, "th_colormap_shape");
    napi_value out, v;
    napi_create_array_with_length(env, 2, &out);
    napi_create_int32(env, w, &v); napi_set_element(env, out, 0, v);
    napi_create_int32(env, h, &v); napi_set_element(env, out, 1, v);
    return out;
}

// colormapBlend(handle, views: Int32Array [source, index] per view, alphas: Float32Array, glBlend, clear)
napi_value ColormapBlend(napi_env env, napi_callback_info info)
{
    size_t argc = 5;
    napi_value argv[5];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 5) return bad(env, "colormapBlend: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "colormapBlend: bad context");
    void *pairs = nullptr, *alphas = nullptr;
    size_t npairs = 0, nalphas = 0;
    if (!typed(env, argv[1], napi_int32_array, &pairs, &npairs) || !typed(env, argv[2], napi_float32_array, &alphas, &nalphas) ||
        npairs != 2 * nalphas)
        return bad(env, "colormapBlend: views are an Int32Array of [source, index] pairs, alphas a Float32Array of as many");
    bool flags[2];
    for (int k = 0; k < 2; ++k)
        if (napi_get_value_bool(env, argv[3 + k], &flags[k]) != napi_ok) return bad(env, "colormapBlend: glBlend and clear are booleans");
    th_blend_view views[TH_MAX_BLEND_VIEWS];
    // (more views than the table holds: the library refuses the count - and says so - before it reads a view)
    const size_t n = nalphas <= TH_MAX_BLEND_VIEWS ? nalphas : TH_MAX_BLEND_VIEWS;
    for (size_t i = 0; i < n; ++i) {
        views[i].source = static_cast<const int32_t *>(pairs)[2 * i];
        views[i].index = static_cast<const int32_t *>(pairs)[2 * i + 1];
        views[i].alpha = static_cast<const float *>(alphas)[i];
    }
    if (th_status s = th_colormap_blend(ctx, views, nalphas <= TH_MAX_BLEND_VIEWS ? (int32_t)n : TH_MAX_BLEND_VIEWS + 1, flags[0], flags[1])) return fail(env, s, "th_colormap_blend");
    return undefined(env);
}

// colormapDownload(handle) -> Float32Array, w x h RGBA32F
napi_value ColormapDownload(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1) return bad(env, "colormapDownload: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "colormapDownload: bad context");
    int32_t w = 0, h = 0;
    if (th_status s = th_colormap_shape(ctx, &w, &h)) return fail(env, s, "th_colormap_shape");
    const size_t floats = (size_t)w * (size_t)h * 4;
    void *data = nullptr;
    napi_value buffer, out;
    if (napi_create_arraybuffer(env, floats * sizeof(float), &data, &buffer) != napi_ok) return bad(env, "colormapDownload: no memory");
    if (th_status s = th_colormap_download(ctx, static_cast<float *>(data))) return fail(env, s, "th_colormap_download");
    napi_create_typedarray(env, napi_float32_array, floats, buffer, 0, &out);
    return out;
}

napi_value Init(napi_env env, napi_value exports)
{
    napi_property_descriptor props[] = {
        {"textureUpload", nullptr, TextureUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"colormapResize", nullptr, ColormapResize, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"colormapShape", nullptr, ColormapShape, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"colormapBlend", nullptr, ColormapBlend, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"colormapDownload", nullptr, ColormapDownload, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    const struct { const char *name; int32_t value; } constants[] = {
        {"TEX_RGBA32F", TH_TEX_RGBA32F}, {"TEX_RGBA8", TH_TEX_RGBA8}, {"TEX_L32F", TH_TEX_L32F},
        {"VIEW_TEXTURE", TH_VIEW_TEXTURE}, {"VIEW_FRAMES", TH_VIEW_FRAMES}, {"VIEW_SPAWN_IMAGE", TH_VIEW_SPAWN_IMAGE},
        {"MAX_TEXTURES", TH_MAX_TEXTURES}, {"MAX_BLEND_VIEWS", TH_MAX_BLEND_VIEWS}};
    for (const auto &c : constants) {
        napi_value v;
        napi_create_int32(env, c.value, &v);
        napi_set_named_property(env, exports, c.name, v);
    }
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
