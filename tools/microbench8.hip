// microbench8: issue rate of the integer / conversion VALU forms the fused integrator's index chain and flow-tap address can be
// built from (v_cvt_u32_f32, v_floor_f32, the 24-bit multiplies, v_bfe_u32, v_lshl_add_u32, v_add3_u32, the 64-bit address
// forms) and the plain shift / mask a biased-float index would use, against f32 mul / add; then the literal / SGPR-operand forms
// of the biased-float hash chain (profiles/hash_chain_rates.txt).  Eight independent chains per lane
// (no dependent issue back to back), 64 instructions per loop iteration (beside three scalar ones of the loop itself), every CU filled
// with 2, 5 or 8 waves per SIMD.  Rates in lane-ops/s (wave-instructions * 64 per second).
//   hipcc --offload-arch=gfx950 -O3 -o tools/bin/microbench8 tools/microbench8.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kIters = 512;          // x 64 instructions per lane

#define ROUND8(TEXT) TEXT("%0") "\n\t" TEXT("%1") "\n\t" TEXT("%2") "\n\t" TEXT("%3") "\n\t"                             \
                     TEXT("%4") "\n\t" TEXT("%5") "\n\t" TEXT("%6") "\n\t" TEXT("%7") "\n\t"
#define X8(S) S S S S S S S S

// 32-bit forms: one instruction per chain, chain register %0..%7, the loop-invariant inputs from %8 on: `b` in a VGPR
// (OP32), in an SGPR (OP32S), or `b` in a VGPR and a wave-uniform 64-bit lane mask `m` in an SGPR pair as %9 (OP32M)
#define OP32_IN(NAME, TEXT, ...)                                                                                      \
    __global__ __launch_bounds__(256) void k_##NAME(unsigned *out, unsigned seed)                                    \
    {                                                                                                                 \
        unsigned i = blockIdx.x * 256u + threadIdx.x;                                                                 \
        unsigned a0 = i ^ seed, a1 = a0 + 1u, a2 = a0 + 2u, a3 = a0 + 3u, a4 = a0 + 4u, a5 = a0 + 5u, a6 = a0 + 6u,    \
                 a7 = a0 + 7u, b = seed | 1u;                                                                         \
        [[maybe_unused]] const unsigned long long m = ((unsigned long long)(seed * 0x9e3779b9u) << 32) | (seed * 0x85ebca6bu); \
        _Pragma("unroll 1") for (int it = 0; it < kIters; ++it)                                                       \
            asm volatile(X8(ROUND8(TEXT))                                                                              \
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : __VA_ARGS__); \
        unsigned s = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                                           \
        if (s == 0x9e3779b9u) out[i] = s;                                                                             \
    }
#define OP32(NAME, TEXT) OP32_IN(NAME, TEXT, "v"(b))
#define OP32S(NAME, TEXT) OP32_IN(NAME, TEXT, "s"(b))
#define OP32M(NAME, TEXT) OP32_IN(NAME, TEXT, "v"(b), "s"(m))

#define T_CVT(r) "v_cvt_u32_f32 " r ", " r
#define T_FLOOR(r) "v_floor_f32 " r ", " r
#define T_MULF(r) "v_mul_f32 " r ", " r ", %8"
#define T_ADDF(r) "v_add_f32 " r ", " r ", %8"
#define T_MUL24(r) "v_mul_u32_u24 " r ", " r ", %8"
#define T_MULHI24(r) "v_mul_hi_u32_u24 " r ", " r ", %8"
#define T_MAD24(r) "v_mad_u32_u24 " r ", " r ", %8, " r
#define T_BFE(r) "v_bfe_u32 " r ", " r ", 3, 9"
#define T_LSHLADD(r) "v_lshl_add_u32 " r ", " r ", 4, %8"
#define T_ADD3(r) "v_add3_u32 " r ", " r ", %8, " r
#define T_ADDU(r) "v_add_u32 " r ", " r ", %8"
#define T_LSHL(r) "v_lshlrev_b32 " r ", 2, " r
#define T_AND(r) "v_and_b32 " r ", " r ", %8"
OP32(cvt_u32_f32, T_CVT)
OP32(floor_f32, T_FLOOR)
OP32(mul_f32, T_MULF)
OP32(add_f32, T_ADDF)
OP32(mul_u32_u24, T_MUL24)
OP32(mul_hi_u32_u24, T_MULHI24)
OP32(mad_u32_u24, T_MAD24)
OP32(bfe_u32, T_BFE)
OP32(lshl_add_u32, T_LSHLADD)
OP32(add3_u32, T_ADD3)
OP32(add_u32, T_ADDU)
OP32(lshlrev_b32, T_LSHL)
OP32(and_b32, T_AND)
// the forms the biased-float hash index chain is made of (32-bit literals, SGPR operands, the mask select) and ops of the
// step loop the first table left out
#define T_ADDF_LIT(r) "v_add_f32 " r ", 0x4a000000, " r
#define T_ADDF_S(r) "v_add_f32 " r ", %8, " r
#define T_AND_LIT(r) "v_and_b32 " r ", 0xffc, " r
#define T_CNDMASK(r) "v_cndmask_b32 " r ", " r ", %8, %9"
#define T_MAXF(r) "v_max_f32 " r ", " r ", %8"
#define T_FMAC_LIT(r) "v_fmac_f32 " r ", 0xc3908000, %8"
#define T_SUBF(r) "v_sub_f32 " r ", " r ", %8"
OP32(add_f32_lit, T_ADDF_LIT)
OP32S(add_f32_sgpr, T_ADDF_S)
OP32(and_b32_lit, T_AND_LIT)
OP32M(cndmask_b32_sgpr, T_CNDMASK)
OP32(max_f32, T_MAXF)
OP32(fmac_f32_lit, T_FMAC_LIT)
OP32(sub_f32, T_SUBF)

// 64-bit forms: eight 64-bit chains; v_mad_u64_u32 writes its carry to an SGPR pair of its own per chain
__global__ __launch_bounds__(256) void k_mad_u64_u32(unsigned *out, unsigned seed)
{
    unsigned i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long a[8];
    for (int k = 0; k < 8; ++k) a[k] = (unsigned long long)(i ^ seed) + k;
    unsigned b = seed | 1u;
    unsigned long long c[8];
#pragma unroll 1
    for (int it = 0; it < kIters; ++it)
        asm volatile(X8("v_mad_u64_u32 %0, %8, %16, %16, %0\n\tv_mad_u64_u32 %1, %9, %16, %16, %1\n\t"
                        "v_mad_u64_u32 %2, %10, %16, %16, %2\n\tv_mad_u64_u32 %3, %11, %16, %16, %3\n\t"
                        "v_mad_u64_u32 %4, %12, %16, %16, %4\n\tv_mad_u64_u32 %5, %13, %16, %16, %5\n\t"
                        "v_mad_u64_u32 %6, %14, %16, %16, %6\n\tv_mad_u64_u32 %7, %15, %16, %16, %7\n\t")
                     : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                       "=s"(c[0]), "=s"(c[1]), "=s"(c[2]), "=s"(c[3]), "=s"(c[4]), "=s"(c[5]), "=s"(c[6]), "=s"(c[7])
                     : "v"(b));
    unsigned long long s = 0;
    for (int k = 0; k < 8; ++k) s ^= a[k];
    if ((unsigned)s == 0x9e3779b9u) out[i] = (unsigned)s;
}

__global__ __launch_bounds__(256) void k_lshl_add_u64(unsigned *out, unsigned seed)
{
    unsigned i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long a[8];
    for (int k = 0; k < 8; ++k) a[k] = (unsigned long long)(i ^ seed) + k;
    unsigned long long b = seed | 1u;
#pragma unroll 1
    for (int it = 0; it < kIters; ++it)
        asm volatile(X8("v_lshl_add_u64 %0, %0, 2, %8\n\tv_lshl_add_u64 %1, %1, 2, %8\n\t"
                        "v_lshl_add_u64 %2, %2, 2, %8\n\tv_lshl_add_u64 %3, %3, 2, %8\n\t"
                        "v_lshl_add_u64 %4, %4, 2, %8\n\tv_lshl_add_u64 %5, %5, 2, %8\n\t"
                        "v_lshl_add_u64 %6, %6, 2, %8\n\tv_lshl_add_u64 %7, %7, 2, %8\n\t")
                     : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
                     : "v"(b));
    unsigned long long s = 0;
    for (int k = 0; k < 8; ++k) s ^= a[k];
    if ((unsigned)s == 0x9e3779b9u) out[i] = (unsigned)s;
}

typedef void (*Kern)(unsigned *, unsigned);

static void run(const char *name, Kern k, unsigned *out, int cus, int waves_per_simd)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const unsigned blocks = (unsigned)cus * (unsigned)waves_per_simd;       // 4 waves per block: one per SIMD
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, 12345u);
    CK(hipEventRecord(e0));
    for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, 12345u);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double lane_ops = 5.0 * blocks * 256.0 * kIters * 64.0;
    printf("%-20s waves/SIMD %d: %7.3f ms  %6.2f T lane-ops/s\n", name, waves_per_simd, ms, lane_ops / ms / 1e9);
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("device %s CUs %d clock %d kHz\n", prop.gcnArchName, prop.multiProcessorCount, prop.clockRate);
    unsigned *out;
    CK(hipMalloc(&out, (size_t)prop.multiProcessorCount * 8 * 256 * sizeof(unsigned)));
    const struct { const char *n; Kern k; } ops[] = {
        {"v_mul_f32", k_mul_f32}, {"v_add_f32", k_add_f32}, {"v_add_u32", k_add_u32},
        {"v_lshlrev_b32", k_lshlrev_b32}, {"v_and_b32", k_and_b32},
        {"v_cvt_u32_f32", k_cvt_u32_f32}, {"v_floor_f32", k_floor_f32},
        {"v_mul_u32_u24", k_mul_u32_u24}, {"v_mul_hi_u32_u24", k_mul_hi_u32_u24}, {"v_mad_u32_u24", k_mad_u32_u24},
        {"v_bfe_u32", k_bfe_u32}, {"v_lshl_add_u32", k_lshl_add_u32}, {"v_add3_u32", k_add3_u32},
        {"v_mad_u64_u32", k_mad_u64_u32}, {"v_lshl_add_u64", k_lshl_add_u64},
        {"v_add_f32 literal", k_add_f32_lit}, {"v_add_f32 sgpr", k_add_f32_sgpr}, {"v_and_b32 literal", k_and_b32_lit},
        {"v_cndmask_b32 sgpr", k_cndmask_b32_sgpr}, {"v_max_f32", k_max_f32}, {"v_fmac_f32 literal", k_fmac_f32_lit},
        {"v_sub_f32", k_sub_f32},
    };
    for (int w : {2, 5, 8})
        for (const auto &o : ops) run(o.n, o.k, out, prop.multiProcessorCount, w);
    CK(hipFree(out));
    return 0;
}
