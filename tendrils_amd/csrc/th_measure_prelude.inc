R"TH_PRELUDE(// th_measure_prelude.inc - what th_measure_program_compile puts in front of a measure program, behind one line
//     #define TH_MEASURE_CHANNELS <the compile call's `channels`, 1 .. 8>
// and the text of th_taps.inc and of th_packed.inc (the packed-state codec, as namespace th)
// (th_measure.hip embeds this file as text: the first and the last line make it one raw string literal).  Self-contained: no
// project header, only what hiprtc's built-in headers give.  Compiled with the product's arithmetic flags (-ffp-contract=off:
// a*b+c stays two rounded fp32 operations).
//
// A measure program defines ONE device function,
//     __device__ th_sample th_measure_main(const th_measure_pass &m);
// called once per particle of one ring buffer: it returns up to TH_MEASURE_CHANNELS numbers, or th_no_sample().  The library
// reduces what the particles return - per channel the sum (in double), the minimum and the maximum, and the count of samples
// taken - and hands the caller one th_measure_result (144 bytes).  A measure writes nothing but that: the ring is read where it
// lies, in whatever slot order it is held.  Of the ring a particle sees its OWN texel alone: there is no th_particles(), and a
// source that names it does not compile (over tile-sorted slots a neighbour's texel would need the inverse table, which step
// programs do not have either).
//
// th_measure_args is the launch record th_measure.hip fills, th_measure_partial what a workgroup leaves and what the library's
// fold returns (same layouts there; the static_asserts pin them).
#ifndef TH_MEASURE_CHANNELS
#error "TH_MEASURE_CHANNELS is not defined: a measure program is compiled through th_measure_program_compile"
#endif
static_assert(TH_MEASURE_CHANNELS >= 1 && TH_MEASURE_CHANNELS <= 8, "a measure program has 1 .. 8 channels");

struct th_measure_partial {
    unsigned long long taken;    // samples taken
    unsigned long long particles;   // (the fold's: a workgroup leaves 0)
    double sum[8];               // channels at and beyond TH_MEASURE_CHANNELS: 0.0 ...
    float min[8];                // ... +inf ...
    float max[8];                // ... -inf
};
static_assert(sizeof(th_measure_partial) == 144 && __builtin_offsetof(th_measure_partial, sum) == 16 &&
                  __builtin_offsetof(th_measure_partial, min) == 80 && __builtin_offsetof(th_measure_partial, max) == 112,
              "th_measure_partial: layout shared with th_measure.hip and th_measure_result");
struct th_measure_args {
    const float4 *in;            // the ring buffer (this context's rows); th_measure_packed_kernel: uint2 texels behind it
    const float4 *flow;
    const unsigned *perm;        // 0: texel order; else slot i of `in` holds texel perm[i] of this context's rows
    th_measure_partial *part;    // one per workgroup
    unsigned count, width, rows, row0, global_height;
    int fw, fh;
    unsigned reserved;
};
static_assert(sizeof(th_measure_args) == 64, "th_measure_args: layout shared with th_measure.hip");
struct __attribute__((aligned(16))) th_program_uniform_block { unsigned char bytes[1024]; };

struct th_measure_pass {
    int x, y;                    // this texel in the WHOLE texture: gl_FragCoord.xy - 0.5 of the unsharded run
    unsigned index;              // y * dataRes.x + x, the particle's index in the whole texture
    float2 dataRes;              // the whole state texture (dataRes)
    float2 uv;                   // gl_FragCoord.xy / dataRes, in fp32: ((float)x + 0.5f) / dataRes.x, ((float)y + 0.5f) / dataRes.y
    float4 self;                 // this particle's state (a packed ring: what its texel decodes to)
    const void *uniforms;        // the caller's uniform block (th_uniforms<T>(m))
    const th_measure_args *args;
};

// what one particle contributes: v[c] to channel c - or nothing at all (take == 0)
struct th_sample { float v[TH_MEASURE_CHANNELS]; int take; };

__device__ th_sample th_measure_main(const th_measure_pass &m);

// this particle contributes nothing: not to `taken`, not to any channel
__device__ __forceinline__ th_sample th_no_sample()
{
    th_sample s;
#pragma unroll
    for (int c = 0; c < TH_MEASURE_CHANNELS; ++c) s.v[c] = 0.0f;
    s.take = 0;
    return s;
}
// a taken sample with every channel 0.0f, to be filled in
__device__ __forceinline__ th_sample th_sample_zero()
{
    th_sample s = th_no_sample();
    s.take = 1;
    return s;
}

// the caller's uniform block as its own struct (the same struct, field for field, as the host packs)
template <class T> __device__ __forceinline__ const T &th_uniforms(const th_measure_pass &m)
{
    static_assert(sizeof(T) <= sizeof(th_program_uniform_block), "a uniform block holds at most 1024 bytes");
    return *static_cast<const T *>(m.uniforms);
}

// texture2D(flow, (u, v)): NEAREST, CLAMP_TO_EDGE (th_taps.inc: th_tap_nearest - the texel a step program's th_flow names)
__device__ __forceinline__ float4 th_flow(const th_measure_pass &m, float u, float v)
{
    const th_measure_args &a = *m.args;
    return a.flow[th_tap_nearest(v, a.fh) * a.fw + th_tap_nearest(u, a.fw)];
}
__device__ __forceinline__ float2 th_flow_res(const th_measure_pass &m) { return make_float2((float)m.args->fw, (float)m.args->fh); }

// What a lane carries through its slots, and what every level of the reduction combines: per channel the sum in double, the
// minimum and the maximum in float (v < mn ? v : mn, v > mx ? v : mx: a NaN never enters either, and poisons its sum), and the
// samples taken.  The identities - 0.0, +inf, -inf, 0 - are what a lane without a slot, or whose particles all returned
// th_no_sample(), brings to the cross-lane step: EVERY lane of a workgroup gets there, with defined values.
struct th_measure_acc {
    double sum[TH_MEASURE_CHANNELS];
    float mn[TH_MEASURE_CHANNELS], mx[TH_MEASURE_CHANNELS];
    unsigned long long taken;
};
__device__ __forceinline__ void th_measure_take(th_measure_acc &r, const th_sample &s)
{
    if (!s.take) return;
    ++r.taken;
#pragma unroll
    for (int c = 0; c < TH_MEASURE_CHANNELS; ++c) {
        const float v = s.v[c];
        r.sum[c] += (double)v;
        r.mn[c] = v < r.mn[c] ? v : r.mn[c];
        r.mx[c] = v > r.mx[c] ? v : r.mx[c];
    }
}
// Everything a program sees of WHO it is - x, y, index, uv - derives from the particle id `pid` (its texel within this
// context's rows); `self` is what the slot holds.
__device__ __forceinline__ void th_measure_who(const th_measure_args &a, th_measure_pass &m, unsigned pid)
{
    const unsigned row = pid / a.width;
    m.x = (int)(pid - row * a.width);
    m.y = (int)(row + a.row0);
    m.index = pid + a.row0 * a.width;
    m.uv = make_float2(((float)m.x + 0.5f) / m.dataRes.x, ((float)m.y + 0.5f) / m.dataRes.y);
}
__device__ __forceinline__ float4 th_measure_load(const th_measure_args &a, unsigned idx)
{
    typedef float th_v4f __attribute__((ext_vector_type(4)));
    const th_v4f v = __builtin_nontemporal_load(reinterpret_cast<const th_v4f *>(a.in + idx));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 th_measure_load_packed(const th_measure_args &a, unsigned idx)
{
    typedef unsigned th_v2u __attribute__((ext_vector_type(2)));
    const th_v2u v = __builtin_nontemporal_load(reinterpret_cast<const th_v2u *>(a.in) + idx);
    return th::unpack_state(make_uint2(v.x, v.y));
}

// The reduction behind the slot loop (stats_kernel's shape, th_kernels.hip): a __shfl_xor butterfly over each wave - all 64
// lanes take part, the loop above it has ended for every one of them -, lane 0 of each wave to LDS, thread 0 folds the four
// waves in wave order and stores the workgroup's partial: one plain store, no atomics - the same ring order gives the same bits.
__device__ __forceinline__ void th_measure_reduce(const th_measure_args &a, th_measure_acc r)
{
    __shared__ th_measure_partial sh[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        r.taken += __shfl_xor(r.taken, o);
#pragma unroll
        for (int c = 0; c < TH_MEASURE_CHANNELS; ++c) {
            r.sum[c] += __shfl_xor(r.sum[c], o);
            const float on = __shfl_xor(r.mn[c], o), ox = __shfl_xor(r.mx[c], o);
            r.mn[c] = on < r.mn[c] ? on : r.mn[c];
            r.mx[c] = ox > r.mx[c] ? ox : r.mx[c];
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
        th_measure_partial &p = sh[threadIdx.x >> 6];
        p.taken = r.taken;
        p.particles = 0ull;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            p.sum[c] = c < TH_MEASURE_CHANNELS ? r.sum[c < TH_MEASURE_CHANNELS ? c : 0] : 0.0;
            p.min[c] = c < TH_MEASURE_CHANNELS ? r.mn[c < TH_MEASURE_CHANNELS ? c : 0] : __builtin_huge_valf();
            p.max[c] = c < TH_MEASURE_CHANNELS ? r.mx[c < TH_MEASURE_CHANNELS ? c : 0] : -__builtin_huge_valf();
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        th_measure_partial t = sh[0];
        for (int w = 1; w < 4; ++w) {
            t.taken += sh[w].taken;
#pragma unroll
            for (int c = 0; c < TH_MEASURE_CHANNELS; ++c) {
                t.sum[c] += sh[w].sum[c];
                t.min[c] = sh[w].min[c] < t.min[c] ? sh[w].min[c] : t.min[c];
                t.max[c] = sh[w].max[c] > t.max[c] ? sh[w].max[c] : t.max[c];
            }
        }
        a.part[blockIdx.x] = t;
    }
}
__device__ __forceinline__ th_measure_acc th_measure_identity()
{
    th_measure_acc r;
#pragma unroll
    for (int c = 0; c < TH_MEASURE_CHANNELS; ++c) { r.sum[c] = 0.0; r.mn[c] = __builtin_huge_valf(); r.mx[c] = -__builtin_huge_valf(); }
    r.taken = 0ull;
    return r;
}

// The harness: 256-thread workgroups, grid-stride over the slots; a slot's state comes in as one 16-byte non-temporal load and
// nothing is stored to the ring.  Texel order (perm null): slot = texel.  Tile-sorted slots: slot i holds texel perm[i] - read
// once, non-temporal -, x / y / index / uv come from the texel and `self` from the slot.  The test on a.perm is wave-uniform
// (the argument segment).  No lane returns early: the ones past the last slot fall out of the loop with the identities.
extern "C" __global__ __launch_bounds__(256) void th_measure_kernel(const th_measure_args a, const th_program_uniform_block u)
{
    th_measure_pass m;
    m.dataRes = make_float2((float)a.width, (float)a.global_height);
    m.uniforms = u.bytes;
    m.args = &a;
    th_measure_acc r = th_measure_identity();
    if (!a.perm) {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
            th_measure_who(a, m, idx);
            m.self = th_measure_load(a, idx);
            th_measure_take(r, th_measure_main(m));
        }
    } else {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
            th_measure_who(a, m, __builtin_nontemporal_load(a.perm + idx));
            m.self = th_measure_load(a, idx);
            th_measure_take(r, th_measure_main(m));
        }
    }
    th_measure_reduce(a, r);
}

// The same harness on a packed ring (TH_STATE_F16, 8 bytes a texel: th_packed.inc, whose text stands in front of this prelude
// as namespace th): `in` points at uint2 texels, read in place - one 8-byte non-temporal load a slot, decoded as every kernel of
// the library decodes it (what a step program sees); the record itself is th_measure_kernel's.
extern "C" __global__ __launch_bounds__(256) void th_measure_packed_kernel(const th_measure_args a, const th_program_uniform_block u)
{
    th_measure_pass m;
    m.dataRes = make_float2((float)a.width, (float)a.global_height);
    m.uniforms = u.bytes;
    m.args = &a;
    th_measure_acc r = th_measure_identity();
    if (!a.perm) {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
            th_measure_who(a, m, idx);
            m.self = th_measure_load_packed(a, idx);
            th_measure_take(r, th_measure_main(m));
        }
    } else {
        for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.count; idx += gridDim.x * 256u) {
            th_measure_who(a, m, __builtin_nontemporal_load(a.perm + idx));
            m.self = th_measure_load_packed(a, idx);
            th_measure_take(r, th_measure_main(m));
        }
    }
    th_measure_reduce(a, r);
}
)TH_PRELUDE"
