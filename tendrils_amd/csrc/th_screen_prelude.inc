R"TH_PRELUDE(// th_screen_prelude.inc - what th_screen_program_compile puts in front of a screen program, after the text of th_taps.inc
// (th_screen.hip embeds this file as text: the first and the last line make it one raw string literal).  Self-contained: no
// project header, only what hiprtc's built-in headers give.  Compiled with the product's arithmetic flags
// (-ffp-contract=off: a*b+c stays two rounded fp32 operations, as in the reference's shaders).
//
// A screen program defines ONE device function,
//     __device__ float4 th_screen(const th_screen_pass &s);
// main() of a fragment shader under Screen.render() (src/screen/index.js): it is called once per texel of the target and
// returns that texel's colour (gl_FragColor); the harness below blends or stores it.
//
// th_screen_args is the launch record th_screen.hip fills (same layout there; the static_asserts pin the sizes).
struct th_screen_unit_rec {
    const void *texels;
    int w, h, format, reserved;  // format: 0 RGBA32F, 1 RGBA8, 2 L32F (TH_TEX_*)
};
struct th_screen_args {
    void *dst;                   // the target, w x h texels of `format` (RGBA32F or RGBA8)
    unsigned w, h, count;
    int format;
    int gl_blend;                // SRC_ALPHA / ONE_MINUS_SRC_ALPHA over the destination (else: the colour is stored)
    int n_units;
    unsigned reserved[4];
    th_screen_unit_rec unit[8];
};
static_assert(sizeof(th_screen_unit_rec) == 24 && sizeof(th_screen_args) == 240, "th_screen_args: layout shared with th_screen.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_screen_pass {
    int x, y;                    // this texel of the target: gl_FragCoord.xy - 0.5, rows in the order the downloads give them
    float2 res;                  // the target's shape
    float2 uv;                   // gl_FragCoord.xy / res, in fp32: ((float)x + 0.5f) / res.x, ((float)y + 0.5f) / res.y
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(s))
    const th_screen_args *args;
};

__device__ float4 th_screen(const th_screen_pass &s);

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_screen_pass &s)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(s.uniforms);
}

// texel `at` of a unit as the sampler returns it: RGBA8 as UNORM8, a one-channel float texture as (L, L, L, 1)
__device__ __forceinline__ float4 th_unit_texel(const th_screen_unit_rec &t, size_t at)
{
    if (t.format == 1) {
        const uchar4 q = static_cast<const uchar4 *>(t.texels)[at];
        return make_float4(th_tap_unorm8(q.x), th_tap_unorm8(q.y), th_tap_unorm8(q.z), th_tap_unorm8(q.w));
    }
    if (t.format == 2) {
        const float l = static_cast<const float *>(t.texels)[at];
        return make_float4(l, l, l, 1.0f);
    }
    return static_cast<const float4 *>(t.texels)[at];
}
// texture2D(unit, (u, v)): NEAREST, CLAMP_TO_EDGE - a float texture at clamp(floor(u * n), 0, n - 1) in fp32, an RGBA8 one
// through the 16-bit fixed-point coordinate (th_taps.inc: what the colour-map blend taps with).  A unit that is not bound: zeros.
__device__ __forceinline__ float4 th_tex(const th_screen_pass &s, int unit, float u, float v)
{
    const th_screen_args &a = *s.args;
    if ((unsigned)unit >= (unsigned)a.n_units) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const th_screen_unit_rec &t = a.unit[unit];
    if (t.format == 1)
        return th_unit_texel(t, (size_t)th_tap_fx16(v, (unsigned)t.h) * t.w + th_tap_fx16(u, (unsigned)t.w));
    return th_unit_texel(t, (size_t)th_tap_nearest(v, t.h) * t.w + th_tap_nearest(u, t.w));
}
__device__ __forceinline__ int th_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// texel (x, y) of a unit, the coordinates clamped to the texture
__device__ __forceinline__ float4 th_texel(const th_screen_pass &s, int unit, int x, int y)
{
    const th_screen_args &a = *s.args;
    if ((unsigned)unit >= (unsigned)a.n_units) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const th_screen_unit_rec &t = a.unit[unit];
    return th_unit_texel(t, (size_t)th_clampi(y, t.h - 1) * t.w + th_clampi(x, t.w - 1));
}
__device__ __forceinline__ float2 th_tex_res(const th_screen_pass &s, int unit)
{
    const th_screen_args &a = *s.args;
    if ((unsigned)unit >= (unsigned)a.n_units) return make_float2(0.0f, 0.0f);
    return make_float2((float)a.unit[unit].w, (float)a.unit[unit].h);
}

// The harness: one lane per texel of the target, neighbouring lanes neighbouring texels of a row, 256-thread workgroups,
// grid-stride.  The record is the kernel's argument: the unit table comes through scalar loads, the switches on the
// formats and on gl_blend are the same for every lane.  The destination is read only when it is blended over; a float
// target leaves as one 16-byte store per lane, an RGBA8 one as 4 bytes.
extern "C" __global__ __launch_bounds__(256) void th_screen_kernel(const th_screen_args a, const th_program_uniform_block u)
{
    th_screen_pass s;
    s.res = make_float2((float)a.w, (float)a.h);
    s.uniforms = u.bytes;
    s.args = &a;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
        const unsigned y = idx / a.w, x = idx - y * a.w;
        s.x = (int)x;
        s.y = (int)y;
        s.uv = make_float2(((float)x + 0.5f) / s.res.x, ((float)y + 0.5f) / s.res.y);
        float4 c = th_screen(s);
        if (a.format == 1) {
            uchar4 *d = static_cast<uchar4 *>(a.dst) + idx;
            if (a.gl_blend) {
                uchar4 q = *d;
                th_blend_rgba8(q, c);
                *d = q;
            } else *d = th_store_rgba8(c);
        } else {
            float4 *d = static_cast<float4 *>(a.dst) + idx;
            if (a.gl_blend) {        // (th_blend.hip: colormap_blend_kernel)
                const float4 q = *d;
                const float sa = c.w, ia = 1.0f - sa;
                c = make_float4(c.x * sa + q.x * ia, c.y * sa + q.y * ia, c.z * sa + q.z * ia, c.w * sa + q.w * ia);
            }
            *d = c;
        }
    }
}
)TH_PRELUDE"
