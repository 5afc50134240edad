// th_napi_spawn.cc - a small N-API addon of its own (lib/tendrils_spawn_sharded.node) binding the sharded best-sample spawn of
// include/tendrils_hip.h for the Node host (tendrils_amd/js/particles.js): th_spawn_sample_sharded, th_spawn_query and the
// option that sizes its chunks.  Like the flow-lines addon (th_napi_flowline.cc) it takes the context handle the main addon
// (th_napi.cc) hands out - an external wrapping a th_context ** - and leaves the main addon's exports as they are.
#include <node_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

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

th_context *context(napi_env env, napi_value v)
{
    void *slot = nullptr;
    if (napi_get_value_external(env, v, &slot) != napi_ok || !slot) return nullptr;
    return *static_cast<th_context **>(slot);         // (null once the handle was destroyed)
}

// spawnSampleSharded(handle, Float32Array(17) float uniforms, samples, apply, source, target): th_spawn_sample on a row-band
// shard, every rank collectively - the taps' texels fetched from the ranks that own them
napi_value SpawnSampleSharded(napi_env env, napi_callback_info info)
{
    size_t argc = 6;
    napi_value argv[6];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 6) return bad(env, "spawnSampleSharded: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "spawnSampleSharded: bad context");
    napi_typedarray_type type;
    void *data = nullptr;
    size_t n = 0;
    int32_t v[4];
    if (napi_get_typedarray_info(env, argv[1], &type, &n, &data, nullptr, nullptr) != napi_ok || type != napi_float32_array || n != 17 || !data)
        return bad(env, "spawnSampleSharded: the uniforms are a Float32Array of 17");
    for (int k = 0; k < 4; ++k)
        if (napi_get_value_int32(env, argv[2 + k], &v[k]) != napi_ok) return bad(env, "spawnSampleSharded: bad arguments");
    th_spawn_sample_uniforms u{};
    memcpy(&u, data, 17 * sizeof(float));
    u.samples = v[0]; u.apply = v[1];
    if (th_status s = th_spawn_sample_sharded(ctx, &u, v[2], v[3])) return fail(env, s, "th_spawn_sample_sharded");
    napi_value undef;
    napi_get_undefined(env, &undef);
    return undef;
}

// spawnQuery(handle) -> {taps, localTaps, sentBytes, receivedBytes, chunks} of the last spawnSampleSharded
napi_value SpawnQuery(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1) return bad(env, "spawnQuery: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "spawnQuery: bad context");
    th_spawn_info q{};
    if (th_status s = th_spawn_query(ctx, &q)) return fail(env, s, "th_spawn_query");
    napi_value out, v;
    napi_create_object(env, &out);
    const char *names[4] = {"taps", "localTaps", "sentBytes", "receivedBytes"};
    const uint64_t values[4] = {q.taps, q.local_taps, q.sent_bytes, q.received_bytes};
    for (int k = 0; k < 4; ++k) {
        napi_create_double(env, (double)values[k], &v);
        napi_set_named_property(env, out, names[k], v);
    }
    napi_create_int32(env, q.chunks, &v);
    napi_set_named_property(env, out, "chunks", v);
    return out;
}

napi_value Init(napi_env env, napi_value exports)
{
    napi_property_descriptor props[] = {
        {"spawnSampleSharded", nullptr, SpawnSampleSharded, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"spawnQuery", nullptr, SpawnQuery, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    napi_value v;
    napi_create_int32(env, TH_OPT_SPAWN_CHUNK_ROWS, &v);           // (Particles.option('spawnChunkRows'))
    napi_set_named_property(env, exports, "OPT_SPAWN_CHUNK_ROWS", v);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
