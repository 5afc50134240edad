R"TH_PRELUDE(// th_step_prelude.inc - what th_step_program_compile puts in front of a step program, behind the text of th_taps.inc
// and of th_packed.inc (the packed-state codec, as namespace th)
// (th_stepprog.hip embeds this file as text: the first and the last line make it one raw string literal).  Self-contained: no
// project header, only what hiprtc's built-in headers give.  Compiled with the product's arithmetic flags (-ffp-contract=off:
// a*b+c stays two rounded fp32 operations, as in the reference's shaders).
//
// A step program defines ONE device function,
//     __device__ float4 th_step_main(const th_step_pass &s);
// one step of one particle's integrator: it is called once per state texel and step and returns the texel's next state.  It is a
// state program (th_program_prelude.inc: th_main) under one restriction, which is what lets the library run n steps of it in one
// launch with the state in registers (th_step_kernel below): of the ring it sees its OWN texel alone.  There is no
// th_particles(): a source that names it does not compile, and that is the whole enforcement.  Everything else a pass may read -
// the flow field, spawn data that is not the ring, `targets`, the uniform block - does not change inside a run of steps.
//
// th_step_args is the launch record th_stepprog.hip fills (same layout there; the static_assert pins the size).
struct th_step_args {
    const float4 *in;            // state 0 of this launch (this context's rows)
    float4 *out;                 // state nsteps
    float4 *out_prev;            // state nsteps - 1 (0: not stored - a single step, whose input buffer holds it already)
    const float4 *data;          // spawnData (0: none)
    const float4 *flow;
    const float4 *targets;
    const unsigned *perm;        // 0: texel order; else slot i of in / out / out_prev holds texel perm[i] of this context's rows
    unsigned count, width, rows, row0, global_height;
    int dw, dh, fw, fh;
    unsigned nsteps;             // steps of this launch (1 .. 32)
    unsigned step0;              // index within the CALL of this launch's first step
    float dt;
    float times[32];             // this launch's steps' `time`
};
static_assert(sizeof(th_step_args) == 232, "th_step_args: layout shared with th_stepprog.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_step_pass {
    int x, y;                    // this texel in the WHOLE texture: gl_FragCoord.xy - 0.5 of the unsharded run
    unsigned index;              // y * dataRes.x + x, the particle's index in the whole texture
    float2 dataRes;              // the whole state texture (dataRes)
    float2 geomRes;              // (dataRes.x, 2 dataRes.y): src/index.js:195-197
    float2 uv;                   // gl_FragCoord.xy / dataRes, in fp32: ((float)x + 0.5f) / dataRes.x, ((float)y + 0.5f) / dataRes.y
    float4 self;                 // this particle's state before this step
    float time, dt;              // this step's timer values (th_step_program_run: times[step], dt)
    unsigned step;               // this step's index within the call, 0 .. n - 1 (it keeps counting across the call's launches)
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(s))
    const th_step_args *args;
};

__device__ float4 th_step_main(const th_step_pass &s);

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_step_pass &s)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(s.uniforms);
}

// texture2D(spawnData, (u, v)) / texture2D(flow, (u, v)): NEAREST, CLAMP_TO_EDGE (th_taps.inc: th_tap_nearest - the texel a
// state program's th_nearest_texel names, for every coordinate).  Without spawnData: zeros.
__device__ __forceinline__ float4 th_data(const th_step_pass &s, float u, float v)
{
    const th_step_args &a = *s.args;
    if (!a.data) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return a.data[th_tap_nearest(v, a.dh) * a.dw + th_tap_nearest(u, a.dw)];
}
__device__ __forceinline__ float4 th_flow(const th_step_pass &s, float u, float v)
{
    const th_step_args &a = *s.args;
    return a.flow[th_tap_nearest(v, a.fh) * a.fw + th_tap_nearest(u, a.fw)];
}
__device__ __forceinline__ float2 th_data_res(const th_step_pass &s) { return make_float2((float)s.args->dw, (float)s.args->dh); }
__device__ __forceinline__ float2 th_flow_res(const th_step_pass &s) { return make_float2((float)s.args->fw, (float)s.args->fh); }
// this texel of tendrils.targets (src/index.js:105)
__device__ __forceinline__ float4 th_targets(const th_step_pass &s)
{
    const th_step_args &a = *s.args;
    return a.targets[(unsigned)(s.y - (int)a.row0) * a.width + (unsigned)s.x];
}

// The harness: one thread per slot, 256-thread workgroups.  The slot's state comes in as one 16-byte non-temporal load, the
// steps of the launch run with the state in registers (the step count and so times[k] are wave-uniform: scalar loads from the
// argument segment), states nsteps and nsteps - 1 leave as one 16-byte non-temporal store each.  A lane touches its own slot
// alone, so `out` or `out_prev` may be `in`.  The step loop is not unrolled: its body is the caller's.
// Everything a program sees of WHO it is - x, y, index, uv, its targets texel - derives from the particle id `pid` (its texel
// within this context's rows); the loads and stores are at the slot.
__device__ __forceinline__ void th_step_slot(const th_step_args &a, th_step_pass &s, unsigned idx, unsigned pid)
{
    typedef float th_v4f __attribute__((ext_vector_type(4)));
    const unsigned row = pid / a.width;
    s.x = (int)(pid - row * a.width);
    s.y = (int)(row + a.row0);
    s.index = pid + a.row0 * a.width;
    s.uv = make_float2(((float)s.x + 0.5f) / s.dataRes.x, ((float)s.y + 0.5f) / s.dataRes.y);
    const th_v4f v0 = __builtin_nontemporal_load(reinterpret_cast<const th_v4f *>(a.in + idx));
    float4 prev = make_float4(v0.x, v0.y, v0.z, v0.w), cur = prev;
#pragma clang loop unroll(disable)
    for (unsigned k = 0; k < a.nsteps; ++k) {
        prev = cur;
        s.self = cur;
        s.time = a.times[k];
        s.step = a.step0 + k;
        cur = th_step_main(s);
    }
    const th_v4f v = {cur.x, cur.y, cur.z, cur.w};
    __builtin_nontemporal_store(v, reinterpret_cast<th_v4f *>(a.out + idx));
    if (a.out_prev) {
        const th_v4f w = {prev.x, prev.y, prev.z, prev.w};
        __builtin_nontemporal_store(w, reinterpret_cast<th_v4f *>(a.out_prev + idx));
    }
}

// Texel order (perm null): grid-stride over the texels, slot = texel.  Tile-sorted slots (th_stepprog.hip launches a grid that is
// a multiple of 8): workgroup b sweeps the (b & 7)-th eighth of the slots, as the built-in fused integrator does - workgroups b
// and b + 8 have been seen to share an XCD, whose L2 then serves the band of the field that eighth taps (a speed matter only).
// perm[slot] is read once, non-temporal.  The test on a.perm is wave-uniform (the argument segment).
extern "C" __global__ __launch_bounds__(256) void th_step_kernel(const th_step_args a, const th_program_uniform_block u)
{
    th_step_pass s;
    s.dataRes = make_float2((float)a.width, (float)a.global_height);
    s.geomRes = make_float2(s.dataRes.x, 2.0f * s.dataRes.y);
    s.dt = a.dt;
    s.uniforms = u.bytes;
    s.args = &a;
    if (!a.perm) {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) th_step_slot(a, s, idx, idx);
    } else {
        const unsigned group = blockIdx.x & 7u, rank = blockIdx.x >> 3, per = (a.count + 7u) >> 3;
        const unsigned lo = group * per, stride = (gridDim.x >> 3) * 256u;
        const unsigned end = lo + per < a.count ? lo + per : a.count;
        for (unsigned idx = lo + rank * 256u + threadIdx.x; idx < end; idx += stride)
            th_step_slot(a, s, idx, __builtin_nontemporal_load(a.perm + idx));
    }
}

// The same harness on a packed ring (TH_STATE_F16, 8 bytes a texel: th_packed.inc, whose text stands in front of this prelude
// as namespace th): `in`, `out` and `out_prev` point at uint2 texels behind the record's float4 * fields, the record itself is
// th_step_kernel's.  The slot's state comes in as one 8-byte non-temporal load and is decoded as every kernel of the library
// decodes it; after EVERY step the result is replaced by what a packed ring would hold of it (quantize_state =
// unpack_state(pack_state(.)) bit for bit, a zero's sign included: tests/test_gpu_packed_codec.py), so a launch of n steps leaves the bits of n single passes; states nsteps and
// nsteps - 1 leave as one 8-byte non-temporal store each (the codec is idempotent on quantised values: packing the carried
// `prev` is exact).  A lane touches its own slot alone, so `out` or `out_prev` may be `in`.
__device__ __forceinline__ void th_step_packed_slot(const th_step_args &a, th_step_pass &s, unsigned idx, unsigned pid)
{
    typedef unsigned th_v2u __attribute__((ext_vector_type(2)));
    const unsigned row = pid / a.width;
    s.x = (int)(pid - row * a.width);
    s.y = (int)(row + a.row0);
    s.index = pid + a.row0 * a.width;
    s.uv = make_float2(((float)s.x + 0.5f) / s.dataRes.x, ((float)s.y + 0.5f) / s.dataRes.y);
    const th_v2u v0 = __builtin_nontemporal_load(reinterpret_cast<const th_v2u *>(a.in) + idx);
    float4 prev = th::unpack_state(make_uint2(v0.x, v0.y)), cur = prev;
#pragma clang loop unroll(disable)
    for (unsigned k = 0; k < a.nsteps; ++k) {
        prev = cur;
        s.self = cur;
        s.time = a.times[k];
        s.step = a.step0 + k;
        cur = th::quantize_state(th_step_main(s));
    }
    const uint2 q = th::pack_state(cur);
    const th_v2u v = {q.x, q.y};
    __builtin_nontemporal_store(v, reinterpret_cast<th_v2u *>(a.out) + idx);
    if (a.out_prev) {
        const uint2 r = th::pack_state(prev);
        const th_v2u w = {r.x, r.y};
        __builtin_nontemporal_store(w, reinterpret_cast<th_v2u *>(a.out_prev) + idx);
    }
}

// th_step_kernel's two loops (th_stepprog.hip launches the first alone on a packed ring: it goes to texel order first)
extern "C" __global__ __launch_bounds__(256) void th_step_packed_kernel(const th_step_args a, const th_program_uniform_block u)
{
    th_step_pass s;
    s.dataRes = make_float2((float)a.width, (float)a.global_height);
    s.geomRes = make_float2(s.dataRes.x, 2.0f * s.dataRes.y);
    s.dt = a.dt;
    s.uniforms = u.bytes;
    s.args = &a;
    if (!a.perm) {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) th_step_packed_slot(a, s, idx, idx);
    } else {
        const unsigned group = blockIdx.x & 7u, rank = blockIdx.x >> 3, per = (a.count + 7u) >> 3;
        const unsigned lo = group * per, stride = (gridDim.x >> 3) * 256u;
        const unsigned end = lo + per < a.count ? lo + per : a.count;
        for (unsigned idx = lo + rank * 256u + threadIdx.x; idx < end; idx += stride)
            th_step_packed_slot(a, s, idx, __builtin_nontemporal_load(a.perm + idx));
    }
}
)TH_PRELUDE"
