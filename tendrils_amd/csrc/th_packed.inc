// th_packed.inc - the packed-state codec (TH_STATE_F16, config C5: 8 bytes per particle instead of 16) that the library's own
// kernels and the text put in front of a caller's step program (th_step_prelude.inc: th_step_packed_kernel) must compute alike:
// ONE copy, read twice, as th_taps.inc.  The includer defines TH_PACKED, inside namespace th on both sides:
//   th_logic.hpp     #define TH_PACKED(...) __VA_ARGS__      the functions themselves
//   th_stepprog.hip  #define TH_PACKED(...) #__VA_ARGS__     their text, handed to hiprtc in front of the step prelude
// Hence: no preprocessor directive and no project name inside TH_PACKED( ), only what hipcc and hiprtc both know (-1000000.0f
// is th::kInert, src/const/inert.glsl).
//   word 0: position, two SNORM16 over [-2, 2): q = rint(clamp(p * 16384, -32767, 32767));
//           (-32768, -32768) = inert, (-32768, 0) = NaN position
//   word 1: velocity, two IEEE fp16 (round to nearest even)
// The integrator arithmetic is unchanged (fp32, exact or fast) on the DECODED values; only the storage is quantised.  The
// reference has no half path: this encoding is defined by this build (DESIGN.md "packed state") and mirrored for the tests in
// tests/helpers.py.
TH_PACKED(
__device__ __forceinline__ float4 unpack_state(uint2 w)
{
    int xs = (int)(short)(w.x & 0xffffu), ys = (int)(short)(w.x >> 16);
    _Float16 hx, hy;
    unsigned short ux = (unsigned short)(w.y & 0xffffu), uy = (unsigned short)(w.y >> 16);
    __builtin_memcpy(&hx, &ux, 2); __builtin_memcpy(&hy, &uy, 2);
    float4 s;
    s.z = (float)hx; s.w = (float)hy;
    if (xs == -32768) {
        if (ys == -32768) { s.x = -1000000.0f; s.y = -1000000.0f; }
        else { s.x = __builtin_nanf(""); s.y = __builtin_nanf(""); }
    } else {
        s.x = (float)xs * 6.103515625e-05f; s.y = (float)ys * 6.103515625e-05f;       // exact: / 16384
    }
    return s;
}

__device__ __forceinline__ uint2 pack_state(float4 s)
{
    unsigned px;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) px = 0x80008000u;
    else if (s.x != s.x || s.y != s.y) px = 0x00008000u;
    else {
        int xs = (int)__builtin_rintf(__builtin_amdgcn_fmed3f(s.x * 16384.0f, -32767.0f, 32767.0f));
        int ys = (int)__builtin_rintf(__builtin_amdgcn_fmed3f(s.y * 16384.0f, -32767.0f, 32767.0f));
        px = ((unsigned)xs & 0xffffu) | ((unsigned)ys << 16);
    }
    _Float16 hx = (_Float16)s.z, hy = (_Float16)s.w;
    unsigned short ux, uy;
    __builtin_memcpy(&ux, &hx, 2); __builtin_memcpy(&uy, &hy, 2);
    return make_uint2(px, (unsigned)ux | ((unsigned)uy << 16));
}
// unpack_state(pack_state(s)) without the 8 bytes in between: what a packed ring holds of a state, as the next fused step reads it,
// bit for bit for EVERY input (tests/test_gpu_packed_codec.py: every rounding boundary of both formats, planted inside a fused
// launch and read back by a program that tells all 32 bits).  The quantised position is an integer-valued float in
// [-32767, 32767]: the stored short converts back to exactly that float, and never to the sentinel -32768 - but for one value: a
// negative position of magnitude up to half a quantum rounds to -0.0, whose short is 0 and decodes to +0.0.  Hence the scaling
// back as fma(q, 2^-14, +0.0f) and not as a product: the sum takes -0.0 to +0.0 (round to nearest) and leaves every other float
// as it is - q * 2^-14 is exact - and the compiler must keep it (no -fno-signed-zeros in the product's flags).  One v_fma_f32
// where a v_mul_f32 stood: no instruction more per step (q + 0.0f before the product costs two; profiles/packed_codec.txt has
// both, counted and timed).  The velocity goes through fp16 and back, which keeps a zero's sign on both paths; inert and NaN
// positions come back as unpack_state gives them.  (Sixteen instructions fewer per fused step than the words packed, stored in
// registers and unpacked: round 6.)
__device__ __forceinline__ float4 quantize_state(float4 s)
{
    float4 r;
    r.z = (float)(_Float16)s.z; r.w = (float)(_Float16)s.w;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) { r.x = -1000000.0f; r.y = -1000000.0f; }
    else if (s.x != s.x || s.y != s.y) { r.x = __builtin_nanf(""); r.y = __builtin_nanf(""); }
    else {
        r.x = __builtin_fmaf(__builtin_rintf(__builtin_amdgcn_fmed3f(s.x * 16384.0f, -32767.0f, 32767.0f)), 6.103515625e-05f, 0.0f);
        r.y = __builtin_fmaf(__builtin_rintf(__builtin_amdgcn_fmed3f(s.y * 16384.0f, -32767.0f, 32767.0f)), 6.103515625e-05f, 0.0f);
    }
    return r;
}
)
