// th_napi_program.cc - a small N-API addon of its own (lib/tendrils_program.node) binding the user programs of
// include/tendrils_hip.h for the Node host (tendrils_amd/js/particles.js): th_program_compile / _log / _run / _query /
// _destroy.  Like the flow-lines and sharded-spawn addons (th_napi_flowline.cc, th_napi_spawn.cc) it takes the context handle
// the main addon (th_napi.cc) hands out - an external wrapping a th_context ** - and leaves the main addon's exports as they are.
#include <node_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "tendrils_hip.h"

namespace {

napi_value fail(napi_env env, th_status st, const char *what, const char *more = "")
{
    const std::string msg = std::string("tendrils_hip ") + what + ": status " + std::to_string((int)st) + ": " + th_last_error() +
                            (*more ? "\n" : "") + more;
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

// a program's handle: an external wrapping a th_program * that programDestroy - or the collector - frees once
void release(napi_env, void *data, void *)
{
    th_program **slot = static_cast<th_program **>(data);
    if (*slot) (void)th_program_destroy(*slot);
    delete slot;
}

th_program **program(napi_env env, napi_value v)
{
    void *slot = nullptr;
    if (napi_get_value_external(env, v, &slot) != napi_ok || !slot) return nullptr;
    return static_cast<th_program **>(slot);
}

bool string_of(napi_env env, napi_value v, std::string &out)
{
    size_t n = 0;
    if (napi_get_value_string_utf8(env, v, nullptr, 0, &n) != napi_ok) return false;
    out.resize(n + 1);
    if (napi_get_value_string_utf8(env, v, &out[0], n + 1, &n) != napi_ok) return false;
    out.resize(n);
    return true;
}

// programCompile(source, name) -> handle; throws with the compiler's output when the source does not compile
napi_value ProgramCompile(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    std::string source, name;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || !string_of(env, argv[0], source))
        return bad(env, "programCompile: the source is a string");
    if (argc < 2 || !string_of(env, argv[1], name)) name = "user_program";
    th_program *p = nullptr;
    if (th_status s = th_program_compile(source.c_str(), name.c_str(), &p)) return fail(env, s, "th_program_compile", th_program_log());
    th_program **slot = new th_program *(p);
    napi_value out;
    if (napi_create_external(env, slot, release, nullptr, &out) != napi_ok) { release(env, slot, nullptr); return bad(env, "programCompile: no handle"); }
    return out;
}

// programLog() -> the compiler's output of this thread's last programCompile
napi_value ProgramLog(napi_env env, napi_callback_info)
{
    napi_value out;
    napi_create_string_utf8(env, th_program_log(), NAPI_AUTO_LENGTH, &out);
    return out;
}

napi_value ProgramDestroy(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1) return bad(env, "programDestroy: bad arguments");
    th_program **slot = program(env, argv[0]);
    if (!slot) return bad(env, "programDestroy: bad program");
    if (*slot) { (void)th_program_destroy(*slot); *slot = nullptr; }
    return undefined(env);
}

// programRun(handle, program, uniforms: ArrayBuffer | typed array | null, source, target): one pass of the program
napi_value ProgramRun(napi_env env, napi_callback_info info)
{
    size_t argc = 5;
    napi_value argv[5];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 5) return bad(env, "programRun: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "programRun: bad context");
    th_program **slot = program(env, argv[1]);
    if (!slot || !*slot) return bad(env, "programRun: bad (or destroyed) program");
    void *data = nullptr;
    size_t bytes = 0;
    bool is = false;
    if (napi_is_arraybuffer(env, argv[2], &is) == napi_ok && is) {
        if (napi_get_arraybuffer_info(env, argv[2], &data, &bytes) != napi_ok) return bad(env, "programRun: bad uniforms");
    } else if (napi_is_typedarray(env, argv[2], &is) == napi_ok && is) {
        napi_typedarray_type type;
        size_t n = 0;
        if (napi_get_typedarray_info(env, argv[2], &type, &n, &data, nullptr, nullptr) != napi_ok) return bad(env, "programRun: bad uniforms");
        const size_t width[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        if ((size_t)type >= sizeof width / sizeof *width) return bad(env, "programRun: bad uniforms");
        bytes = n * width[type];
    } else {
        napi_valuetype t;
        if (napi_typeof(env, argv[2], &t) != napi_ok || (t != napi_null && t != napi_undefined))
            return bad(env, "programRun: the uniforms are an ArrayBuffer, a typed array or null");
    }
    int32_t v[2];
    for (int k = 0; k < 2; ++k)
        if (napi_get_value_int32(env, argv[3 + k], &v[k]) != napi_ok) return bad(env, "programRun: bad arguments");
    if (bytes > 0xffffffffu) return bad(env, "programRun: bad uniforms");
    if (th_status s = th_program_run(ctx, *slot, data, (uint32_t)bytes, v[0], v[1])) return fail(env, s, "th_program_run");
    return undefined(env);
}

// programQuery(handle, program) -> {vgprs, sgprs, ldsBytes, scratchBytes, codeBytes}
napi_value ProgramQuery(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2) return bad(env, "programQuery: bad arguments");
    th_context *ctx = context(env, argv[0]);
    if (!ctx) return bad(env, "programQuery: bad context");
    th_program **slot = program(env, argv[1]);
    if (!slot || !*slot) return bad(env, "programQuery: bad (or destroyed) program");
    th_program_info q{};
    if (th_status s = th_program_query(ctx, *slot, &q)) return fail(env, s, "th_program_query");
    napi_value out, v;
    napi_create_object(env, &out);
    const char *names[5] = {"vgprs", "sgprs", "ldsBytes", "scratchBytes", "codeBytes"};
    const uint32_t values[5] = {q.vgprs, q.sgprs, q.lds_bytes, q.scratch_bytes, q.code_bytes};
    for (int k = 0; k < 5; ++k) {
        napi_create_uint32(env, values[k], &v);
        napi_set_named_property(env, out, names[k], v);
    }
    return out;
}

napi_value Init(napi_env env, napi_value exports)
{
    napi_property_descriptor props[] = {
        {"programCompile", nullptr, ProgramCompile, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"programLog", nullptr, ProgramLog, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"programDestroy", nullptr, ProgramDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"programRun", nullptr, ProgramRun, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"programQuery", nullptr, ProgramQuery, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    napi_value v;
    napi_create_int32(env, TH_SOURCE_NONE, &v);
    napi_set_named_property(env, exports, "SOURCE_NONE", v);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
