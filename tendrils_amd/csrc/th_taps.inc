// th_taps.inc - the texture-tap and RGBA8 rounding rules that the library's own kernels and the text put in front of a
// caller's screen program (th_screen_prelude.inc) must compute alike: ONE copy, read twice.  The includer defines TH_TAPS:
//   th_math.hpp     #define TH_TAPS(...) __VA_ARGS__      the functions themselves (namespace th)
//   th_screen.hip   #define TH_TAPS(...) #__VA_ARGS__     their text, handed to hiprtc in front of the screen prelude
// Hence: no preprocessor directive and no project name inside TH_TAPS( ), only what hipcc and hiprtc both know.
TH_TAPS(
// NEAREST + CLAMP_TO_EDGE on a float texture of n texels: always inside [0, n - 1] (a NaN coordinate: 0)
__device__ __forceinline__ int th_tap_nearest(float u, int n)
{
    float f = __builtin_floorf(u * (float)n);
    if (!(f > 0.0f)) return 0;
    if (f > (float)(n - 1)) return n - 1;
    return (int)f;
}
// ... on an 8-bit-per-channel texture (n <= 65536), with the coordinate precision of the captured reference run: clamp to
// [0, 1), truncate to 16 fractional bits, texel = (coord16 * size) >> 16 (equals floor(u*size) except within 2^-16 of a
// texel boundary).
__device__ __forceinline__ int th_tap_fx16(float u, unsigned n)
{
    float c = __builtin_amdgcn_fmed3f(u, 0.0f, 65535.0f / 65536.0f);
    unsigned fx = (unsigned)(c * 65536.0f);
    return (int)((fx * n) >> 16);
}
// UNORM8 -> float as (c*257) * (1/65535): what the captured reference run did; equals c/255 within 1 ulp.
__device__ __forceinline__ float th_tap_unorm8(unsigned char c) { return ((float)c * 257.0f) * (1.0f / 65535.0f); }

// the RGBA8 drawing buffer's blend (SRC_ALPHA / ONE_MINUS_SRC_ALPHA): the fragment colour is clamped to [0, 1], blended
// with the stored colour c/255 and stored as round(255 x), fragment after fragment (what the captured GL does)
__device__ __forceinline__ void th_blend_rgba8(uchar4 &q, float4 c)
{
    c.x = __builtin_fminf(__builtin_fmaxf(c.x, 0.0f), 1.0f); c.y = __builtin_fminf(__builtin_fmaxf(c.y, 0.0f), 1.0f);
    c.z = __builtin_fminf(__builtin_fmaxf(c.z, 0.0f), 1.0f); c.w = __builtin_fminf(__builtin_fmaxf(c.w, 0.0f), 1.0f);
    const float sa = c.w;
    const float da = 1.0f - sa;
    const float k = 1.0f / 255.0f;
    auto mix8 = [&](float src, unsigned char dst) {
        const float o = src * sa + ((float)dst * k) * da;
        return (unsigned char)(__builtin_fminf(__builtin_fmaxf(o, 0.0f), 1.0f) * 255.0f + 0.5f);
    };
    q = make_uchar4(mix8(c.x, q.x), mix8(c.y, q.y), mix8(c.z, q.z), mix8(c.w, q.w));
}
// ... and the same clamp and rounding with no destination term (the blend disabled)
__device__ __forceinline__ uchar4 th_store_rgba8(float4 c)
{
    auto to8 = [](float v) { return (unsigned char)(__builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); };
    return make_uchar4(to8(c.x), to8(c.y), to8(c.z), to8(c.w));
}
)
