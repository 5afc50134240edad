// th_napi_flowline.cc - a second, small N-API addon (lib/tendrils_flow_lines.node) binding the flow-line calls of
// include/tendrils_hip.h for the Node host (tendrils_amd/js/flow-line.js).  It takes the context handle the main addon
// (th_napi.cc) hands out: an external wrapping a th_context **.
#include <node_api.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "tendrils_hip.h"

namespace {

napi_value fail(napi_env env, th_status st, const char *what)
{
    char msg[640];
    snprintf(msg, sizeof msg, "tendrils_hip %s: status %d: %s", what, (int)st, th_last_error());
    napi_throw_error(env, nullptr, msg);
    return nullptr;
}

napi_value bad(napi_env env, const char *what)
{
    napi_throw_type_error(env, nullptr, what);
    return nullptr;
}

void *typed(napi_env env, napi_value v, napi_typedarray_type want, size_t *len)
{
    napi_typedarray_type t;
    void *data = nullptr;
    size_t n = 0;
    if (napi_get_typedarray_info(env, v, &t, &n, &data, nullptr, nullptr) != napi_ok || t != want) return nullptr;
    *len = n;
    return data ? data : (void *)"";     // (an empty array may have no storage)
}

// flowLineAttributes(points: Float32Array [n*2], times: Float64Array [n], closed: bool) -> {position, normal, miter,
// previous, time, dt}: Float32Arrays
napi_value Attributes(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3) return bad(env, "flowLineAttributes: bad arguments");
    size_t np = 0, nt = 0;
    const float *pts = static_cast<const float *>(typed(env, argv[0], napi_float32_array, &np));
    const double *tms = static_cast<const double *>(typed(env, argv[1], napi_float64_array, &nt));
    bool closed = false;
    if (!pts || !tms || np != 2 * nt || napi_get_value_bool(env, argv[2], &closed) != napi_ok) return bad(env, "flowLineAttributes: bad arguments");
    int32_t nv = 0;
    if (th_status s = th_flow_line_attributes(pts, tms, (int32_t)nt, closed, 0, &nv, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return fail(env, s, "th_flow_line_attributes");
    static const char *names[6] = {"position", "normal", "miter", "previous", "time", "dt"};
    static const int sizes[6] = {2, 2, 1, 2, 1, 1};
    napi_value out;
    napi_create_object(env, &out);
    float *data[6];
    for (int k = 0; k < 6; ++k) {
        napi_value ab, arr;
        void *raw = nullptr;
        const size_t n = (size_t)nv * sizes[k];
        if (napi_create_arraybuffer(env, n * sizeof(float), &raw, &ab) != napi_ok ||
            napi_create_typedarray(env, napi_float32_array, n, ab, 0, &arr) != napi_ok)
            return bad(env, "flowLineAttributes: out of memory");
        data[k] = static_cast<float *>(raw);
        napi_set_named_property(env, out, names[k], arr);
    }
    if (nv)
        if (th_status s = th_flow_line_attributes(pts, tms, (int32_t)nt, closed, nv, &nv, data[0], data[1], data[2], data[3], data[4], data[5]))
            return fail(env, s, "th_flow_line_attributes");
    return out;
}

// flowLines(handle, uniforms: Float32Array [speed, rad, crestShape, speedLimit, viewSize.x, viewSize.y], points: Float32Array,
//           times: Float64Array, offsets: Int32Array [nlines + 1], closed: Int32Array [nlines])
napi_value Lines(napi_env env, napi_callback_info info)
{
    size_t argc = 6;
    napi_value argv[6];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 6) return bad(env, "flowLines: bad arguments");
    void *slot = nullptr;
    if (napi_get_value_external(env, argv[0], &slot) != napi_ok || !slot) return bad(env, "flowLines: bad context");
    th_context *ctx = *static_cast<th_context **>(slot);
    size_t nu = 0, np = 0, nt = 0, no = 0, nc = 0;
    const float *uf = static_cast<const float *>(typed(env, argv[1], napi_float32_array, &nu));
    const float *pts = static_cast<const float *>(typed(env, argv[2], napi_float32_array, &np));
    const double *tms = static_cast<const double *>(typed(env, argv[3], napi_float64_array, &nt));
    const int32_t *offs = static_cast<const int32_t *>(typed(env, argv[4], napi_int32_array, &no));
    const int32_t *cl = static_cast<const int32_t *>(typed(env, argv[5], napi_int32_array, &nc));
    if (!uf || nu != 6 || !pts || !tms || !offs || !cl || np != 2 * nt || (no ? no != nc + 1 : nc != 0))
        return bad(env, "flowLines: bad arguments");
    const int32_t nlines = (int32_t)nc;
    for (int32_t i = 0; i <= nlines; ++i)
        if (offs[i] < 0 || (size_t)offs[i] > nt) return bad(env, "flowLines: offsets out of range");
    th_flow_line_uniforms u{};
    u.speed = uf[0]; u.rad = uf[1]; u.crestShape = uf[2]; u.speedLimit = uf[3]; u.viewSize[0] = uf[4]; u.viewSize[1] = uf[5];
    if (th_status s = th_flow_lines(ctx, &u, pts, tms, nlines ? offs : nullptr, nlines ? cl : nullptr, nlines))
        return fail(env, s, "th_flow_lines");
    napi_value undef;
    napi_get_undefined(env, &undef);
    return undef;
}

napi_value Init(napi_env env, napi_value exports)
{
    napi_property_descriptor props[] = {
        {"flowLineAttributes", nullptr, Attributes, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"flowLines", nullptr, Lines, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
