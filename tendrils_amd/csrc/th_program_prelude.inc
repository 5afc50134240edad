R"TH_PRELUDE(// th_program_prelude.inc - what th_program_compile puts in front of a user program (th_program.hip embeds this file as text:
// the first and the last line make it one raw string literal).  Self-contained: no project header, only what hiprtc's
// built-in headers give.  Compiled with the product's arithmetic flags (-ffp-contract=off: a*b+c stays two rounded fp32
// operations, as in the reference's shaders).
//
// A user program defines ONE device function,
//     __device__ float4 th_main(const th_pass &p);
// the fragment shader of one full-screen pass over the state ring (src/particles.js:123-145): it is called once per state
// texel and returns that texel's new value (gl_FragColor).
//
// th_program_args is the launch record th_program.hip fills (same layout there; the static_assert pins the size).
struct th_program_args {
    const float4 *particles;     // ring[1] as the pass sees it (this context's rows)
    float4 *out;                 // the render target (this context's rows)
    const float4 *data;          // spawnData (0: none)
    const float4 *flow;
    const float4 *targets;
    unsigned *flag;              // row band: 1 + the first global row th_particles was asked for outside the band
    unsigned count, width, rows, row0, global_height;
    int dw, dh, fw, fh;
    unsigned reserved[3];
};
static_assert(sizeof(th_program_args) == 96, "th_program_args: layout shared with th_program.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_pass {
    int x, y;                    // this texel in the WHOLE texture: gl_FragCoord.xy - 0.5 of the unsharded run
    unsigned index;              // y * dataRes.x + x, the particle's index in the whole texture
    float2 dataRes;              // the whole state texture (dataRes)
    float2 geomRes;              // (dataRes.x, 2 dataRes.y): src/index.js:195-197
    float2 uv;                   // gl_FragCoord.xy / dataRes, in fp32: ((float)x + 0.5f) / dataRes.x, ((float)y + 0.5f) / dataRes.y
    float4 self;                 // texture2D(particles, uv): this texel of the previous state
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(p))
    const th_program_args *args;
};

__device__ float4 th_main(const th_pass &p);

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_pass &p)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(p.uniforms);
}

__device__ __forceinline__ int th_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// NEAREST + CLAMP_TO_EDGE lookup of coordinate u in a texture of n texels: clamp(floor(u * n), 0, n - 1) in fp32
// (a NaN coordinate reads texel 0)
__device__ __forceinline__ int th_nearest_texel(float u, int n)
{
    return th_clampi((int)__builtin_amdgcn_fmed3f(__builtin_floorf(u * (float)n), 0.0f, (float)(n - 1)), n - 1);
}
__device__ __forceinline__ float4 th_load16(const float4 *p)
{
    typedef float th_v4f __attribute__((ext_vector_type(4)));
    th_v4f v = __builtin_nontemporal_load(reinterpret_cast<const th_v4f *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// texel (x, y) of `particles` in WHOLE-texture coordinates, clamped to the texture.  On a row band only the band's own rows
// are there: any other row raises the pass's flag (th_program_run then fails with TH_ERR_UNSUPPORTED) and reads as p.self.
__device__ __forceinline__ float4 th_particles(const th_pass &p, int x, int y)
{
    const th_program_args &a = *p.args;
    x = th_clampi(x, (int)a.width - 1);
    y = th_clampi(y, (int)a.global_height - 1);
    const unsigned row = (unsigned)y - a.row0;           // (wraps below the band)
    if (row >= a.rows) { atomicMax(a.flag, (unsigned)y + 1u); return p.self; }
    return a.particles[row * a.width + (unsigned)x];
}
// texture2D(spawnData, (u, v)) / texture2D(flow, (u, v)): NEAREST, CLAMP_TO_EDGE.  Without spawnData: zeros.
__device__ __forceinline__ float4 th_data(const th_pass &p, float u, float v)
{
    const th_program_args &a = *p.args;
    if (!a.data) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return a.data[th_nearest_texel(v, a.dh) * a.dw + th_nearest_texel(u, a.dw)];
}
__device__ __forceinline__ float4 th_flow(const th_pass &p, float u, float v)
{
    const th_program_args &a = *p.args;
    return a.flow[th_nearest_texel(v, a.fh) * a.fw + th_nearest_texel(u, a.fw)];
}
__device__ __forceinline__ float2 th_data_res(const th_pass &p) { return make_float2((float)p.args->dw, (float)p.args->dh); }
__device__ __forceinline__ float2 th_flow_res(const th_pass &p) { return make_float2((float)p.args->fw, (float)p.args->fh); }
// this texel of tendrils.targets (src/index.js:105)
__device__ __forceinline__ float4 th_targets(const th_pass &p)
{
    const th_program_args &a = *p.args;
    return a.targets[(unsigned)(p.y - (int)a.row0) * a.width + (unsigned)p.x];
}

// The harness: one thread per texel, 256-thread workgroups, grid-stride; the own texel comes in as one 16-byte non-temporal
// load and the result leaves as one 16-byte non-temporal store.
extern "C" __global__ __launch_bounds__(256) void th_program_kernel(const th_program_args a, const th_program_uniform_block u)
{
    typedef float th_v4f __attribute__((ext_vector_type(4)));
    th_pass p;
    p.dataRes = make_float2((float)a.width, (float)a.global_height);
    p.geomRes = make_float2(p.dataRes.x, 2.0f * p.dataRes.y);
    p.uniforms = u.bytes;
    p.args = &a;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
        const unsigned row = idx / a.width;
        p.x = (int)(idx - row * a.width);
        p.y = (int)(row + a.row0);
        p.index = idx + a.row0 * a.width;
        p.uv = make_float2(((float)p.x + 0.5f) / p.dataRes.x, ((float)p.y + 0.5f) / p.dataRes.y);
        p.self = th_load16(a.particles + idx);
        const float4 r = th_main(p);
        const th_v4f v = {r.x, r.y, r.z, r.w};
        __builtin_nontemporal_store(v, reinterpret_cast<th_v4f *>(a.out + idx));
    }
}
)TH_PRELUDE"
