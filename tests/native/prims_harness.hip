// prims_harness.hip - test-only C entry points around the primitives every pipeline shares: the flat exclusive scan, the rank
// of a texel set and the radix sort of th_sort.hip, and block_scan (th_math.hpp).  This file holds no copy of them: it is linked against the object
// the product library is linked from (tendrils_amd/lib/obj/th_sort.o), so the device code under test is the bytes that ship;
// block_scan is a header template and is instantiated here at the product's (N, T) pairs.
//
// Every entry point takes and returns HOST arrays: allocation, copies, the launch on a stream of its own, the synchronisation
// and every HIP status check live here.  They return 0, or a code (kHip, kGuard, kArgument, kTouched) and leave thp_last_error().
//
// Guard words: every device buffer a primitive may write is allocated with kGuardBytes of a known pattern behind its stated
// size; a changed guard is reported as kGuard.  That is how a write past a stated scratch size is caught.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "th_kernels.hpp"
#include "th_math.hpp"

namespace {

enum { kOk = 0, kHip = 1, kGuard = 2, kArgument = 3, kTouched = 4 };
constexpr size_t kGuardBytes = 256;
constexpr int kGuardByte = 0xA5;       // behind every buffer
constexpr int kFillByte = 0xCD;        // what a buffer the caller does not fill holds before the launch

thread_local std::string g_error;

int fail(int code, const std::string &why) { g_error = why; return code; }

#define THP_HIP(expr)                                                                                              \
    do {                                                                                                           \
        const hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return fail(kHip, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)
#define THP_TRY(expr) do { if (const int s_ = (expr)) return s_; } while (0)

// a device buffer of `bytes` bytes with the guard behind it; freed with the Job that owns it
struct Guarded {
    const char *name = "";
    char *p = nullptr;
    size_t bytes = 0;
};

struct Job {
    hipStream_t stream = nullptr;
    std::vector<Guarded *> buffers;
    ~Job()
    {
        for (Guarded *g : buffers) if (g->p) (void)hipFree(g->p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int start() { THP_HIP(hipStreamCreate(&stream)); return kOk; }
    int alloc(Guarded &g, const char *name, size_t bytes, bool fill)
    {
        g.name = name; g.bytes = bytes;
        THP_HIP(hipMalloc((void **)&g.p, bytes + kGuardBytes));
        buffers.push_back(&g);
        if (fill && bytes) THP_HIP(hipMemsetAsync(g.p, kFillByte, bytes, stream));
        THP_HIP(hipMemsetAsync(g.p + bytes, kGuardByte, kGuardBytes, stream));
        return kOk;
    }
    int upload(Guarded &g, const void *src, size_t bytes)
    {
        if (bytes) THP_HIP(hipMemcpyAsync(g.p, src, bytes, hipMemcpyHostToDevice, stream));
        return kOk;
    }
    int download(void *dst, const Guarded &g, size_t bytes)
    {
        if (bytes) THP_HIP(hipMemcpyAsync(dst, g.p, bytes, hipMemcpyDeviceToHost, stream));
        return kOk;
    }
    int finish()
    {
        THP_HIP(hipGetLastError());
        THP_HIP(hipStreamSynchronize(stream));
        return kOk;
    }
    // after finish(): every buffer's guard still holds the pattern
    int guards()
    {
        unsigned char host[kGuardBytes];
        for (const Guarded *g : buffers) {
            THP_HIP(hipMemcpy(host, g->p + g->bytes, kGuardBytes, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < kGuardBytes; ++k)
                if (host[k] != (unsigned char)kGuardByte) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "guard behind %s (%zu bytes) changed at byte +%zu: 0x%02x", g->name, g->bytes, k, host[k]);
                    return fail(kGuard, msg);
                }
        }
        return kOk;
    }
    // (n = 0) a buffer the primitive must not touch still holds the fill pattern
    int untouched(const Guarded &g)
    {
        std::vector<unsigned char> host(g.bytes);
        if (g.bytes) THP_HIP(hipMemcpy(host.data(), g.p, g.bytes, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < g.bytes; ++k)
            if (host[k] != (unsigned char)kFillByte) {
                char msg[160];
                snprintf(msg, sizeof msg, "%s was written at byte %zu: 0x%02x", g.name, k, host[k]);
                return fail(kTouched, msg);
            }
        return kOk;
    }
};

int launch_sort(uint32_t *ka, uint32_t *va, uint32_t *kb, uint32_t *vb, uint32_t n, int b, int e, void *temp, bool iota, hipStream_t s)
{
    return th::launch_radix_sort_u32(ka, va, kb, vb, n, b, e, temp, iota, s);
}
int launch_sort(unsigned long long *ka, uint32_t *va, unsigned long long *kb, uint32_t *vb, uint32_t n, int b, int e, void *temp,
                bool iota, hipStream_t s)
{
    return th::launch_radix_sort_u64(ka, va, kb, vb, n, b, e, temp, iota, s);
}

template <typename K>
int radix_sort(const K *keys_in, const uint32_t *vals_in, uint32_t n, int begin_bit, int end_bit, K *keys_out, uint32_t *vals_out,
               int *in_b_out)
{
    if (begin_bit < 0 || end_bit <= begin_bit || end_bit > (int)(8 * sizeof(K))) return fail(kArgument, "bit range outside the contract");
    if (n == 0 || !(keys_in && keys_out && vals_out)) return fail(kArgument, "null array or n = 0 (thp_radix_sort_empty)");
    Job job;
    THP_TRY(job.start());
    Guarded ka, va, kb, vb, temp;
    THP_TRY(job.alloc(ka, "keys (a)", (size_t)n * sizeof(K), false));
    THP_TRY(job.alloc(va, "values (a)", (size_t)n * sizeof(uint32_t), vals_in == nullptr));
    THP_TRY(job.alloc(kb, "keys (b)", (size_t)n * sizeof(K), true));
    THP_TRY(job.alloc(vb, "values (b)", (size_t)n * sizeof(uint32_t), true));
    THP_TRY(job.alloc(temp, "temp", th::radix_sort_temp_bytes(n, begin_bit, end_bit), true));
    THP_TRY(job.upload(ka, keys_in, ka.bytes));
    if (vals_in) THP_TRY(job.upload(va, vals_in, va.bytes));
    const int in_b = launch_sort(reinterpret_cast<K *>(ka.p), reinterpret_cast<uint32_t *>(va.p), reinterpret_cast<K *>(kb.p),
                                 reinterpret_cast<uint32_t *>(vb.p), n, begin_bit, end_bit, temp.p, vals_in == nullptr, job.stream);
    THP_TRY(job.download(keys_out, in_b ? kb : ka, ka.bytes));
    THP_TRY(job.download(vals_out, in_b ? vb : va, va.bytes));
    THP_TRY(job.finish());
    if (in_b_out) *in_b_out = in_b;
    return job.guards();
}

// n = 0 with buffers of `cap` elements behind the pointers: nothing may be written
template <typename K>
int radix_sort_empty(uint32_t cap, int begin_bit, int end_bit, int *in_b_out)
{
    if (begin_bit < 0 || end_bit <= begin_bit || end_bit > (int)(8 * sizeof(K))) return fail(kArgument, "bit range outside the contract");
    Job job;
    THP_TRY(job.start());
    Guarded ka, va, kb, vb, temp;
    THP_TRY(job.alloc(ka, "keys (a)", (size_t)cap * sizeof(K), true));
    THP_TRY(job.alloc(va, "values (a)", (size_t)cap * sizeof(uint32_t), true));
    THP_TRY(job.alloc(kb, "keys (b)", (size_t)cap * sizeof(K), true));
    THP_TRY(job.alloc(vb, "values (b)", (size_t)cap * sizeof(uint32_t), true));
    THP_TRY(job.alloc(temp, "temp", th::radix_sort_temp_bytes(cap, begin_bit, end_bit), true));
    const int in_b = launch_sort(reinterpret_cast<K *>(ka.p), reinterpret_cast<uint32_t *>(va.p), reinterpret_cast<K *>(kb.p),
                                 reinterpret_cast<uint32_t *>(vb.p), 0u, begin_bit, end_bit, temp.p, true, job.stream);
    THP_TRY(job.finish());
    if (in_b_out) *in_b_out = in_b;
    for (const Guarded *g : job.buffers) THP_TRY(job.untouched(*g));
    return job.guards();
}

// One workgroup of N threads: `rounds` calls of block_scan in a loop over consecutive N-element slices, on ONE LDS array,
// with nothing between two calls but the loads and stores of the values (no barrier of the harness's own).  Every thread
// stores the total it was handed.
template <uint32_t N, typename T>
__global__ __launch_bounds__(N) void block_scan_kernel(const T *in, T *out, T *totals, uint32_t rounds)
{
    __shared__ T lds[N];
    for (uint32_t r = 0; r < rounds; ++r) {
        T total;
        const T before = th::block_scan<N, T>(lds, in[(size_t)r * N + threadIdx.x], total);
        out[(size_t)r * N + threadIdx.x] = before;
        totals[(size_t)r * N + threadIdx.x] = total;
    }
}

template <uint32_t N, typename T>
int block_scan(const void *in, void *out, void *totals, uint32_t rounds)
{
    Job job;
    THP_TRY(job.start());
    const size_t bytes = (size_t)rounds * N * sizeof(T);
    Guarded din, dout, dtot;
    THP_TRY(job.alloc(din, "in", bytes, false));
    THP_TRY(job.alloc(dout, "out", bytes, true));
    THP_TRY(job.alloc(dtot, "totals", bytes, true));
    THP_TRY(job.upload(din, in, bytes));
    hipLaunchKernelGGL((block_scan_kernel<N, T>), dim3(1), dim3(N), 0, job.stream, reinterpret_cast<const T *>(din.p),
                       reinterpret_cast<T *>(dout.p), reinterpret_cast<T *>(dtot.p), rounds);
    THP_TRY(job.download(out, dout, bytes));
    THP_TRY(job.download(totals, dtot, bytes));
    THP_TRY(job.finish());
    return job.guards();
}

}  // namespace

extern "C" {

const char *thp_last_error(void) { return g_error.c_str(); }

// exclusive scan of n u32 words in place (launch_exclusive_scan_u32), n >= 1
int thp_exclusive_scan_u32(uint32_t *data_inout, uint32_t n)
{
    if (!data_inout || n == 0) return fail(kArgument, "null array or n = 0");
    Job job;
    THP_TRY(job.start());
    Guarded data, sums;
    THP_TRY(job.alloc(data, "data", (size_t)n * sizeof(uint32_t), false));
    THP_TRY(job.alloc(sums, "block_sums", (size_t)th::exclusive_scan_sum_words(n) * sizeof(uint32_t), true));
    THP_TRY(job.upload(data, data_inout, data.bytes));
    th::launch_exclusive_scan_u32(reinterpret_cast<uint32_t *>(data.p), reinterpret_cast<uint32_t *>(sums.p), n, job.stream);
    THP_TRY(job.download(data_inout, data, data.bytes));
    THP_TRY(job.finish());
    return job.guards();
}

// the members of a texel set before each of its nwords >= 1 mask words (launch_texel_set_rank), and how many there are: the last
// word's count before and after.  counts_in: what a caller's kernel has left in the counts buffer (counted = true: the launcher
// must scan THESE, whatever the mask says), or NULL: the buffer holds the fill pattern and the launcher counts the mask's bits.
int thp_texel_set_rank(const unsigned long long *mask_in, uint32_t nwords, const uint32_t *counts_in, uint32_t *counts_out, unsigned long long *total_out)
{
    if (!mask_in || !counts_out || !total_out || nwords == 0) return fail(kArgument, "null array or no words");
    const bool counted = counts_in != nullptr;
    Job job;
    THP_TRY(job.start());
    Guarded mask, counts, sums;
    THP_TRY(job.alloc(mask, "mask", (size_t)nwords * sizeof(unsigned long long), false));
    THP_TRY(job.alloc(counts, "counts", (size_t)nwords * sizeof(uint32_t), !counted));
    THP_TRY(job.alloc(sums, "block_sums", (size_t)th::exclusive_scan_sum_words(nwords) * sizeof(uint32_t), true));
    THP_TRY(job.upload(mask, mask_in, mask.bytes));
    if (counted) THP_TRY(job.upload(counts, counts_in, counts.bytes));
    th::launch_texel_set_rank(reinterpret_cast<const unsigned long long *>(mask.p), reinterpret_cast<uint32_t *>(counts.p),
                              reinterpret_cast<uint32_t *>(sums.p), nwords, counted, job.stream);
    THP_TRY(job.download(counts_out, counts, counts.bytes));
    THP_TRY(job.finish());
    *total_out = (unsigned long long)counts_out[nwords - 1u] + (counted ? counts_in[nwords - 1u] : (uint32_t)__builtin_popcountll(mask_in[nwords - 1u]));
    return job.guards();
}

// stable sort by key bits [begin_bit, end_bit), n >= 1; vals_in == NULL: the values are the positions 0..n-1 (iota = true).
// in_b_out: what the launcher returned (0: result in (a), 1: in (b)); keys_out / vals_out are read from that buffer.
int thp_radix_sort_u32(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t n, int begin_bit, int end_bit, uint32_t *keys_out,
                       uint32_t *vals_out, int *in_b_out)
{
    return radix_sort<uint32_t>(keys_in, vals_in, n, begin_bit, end_bit, keys_out, vals_out, in_b_out);
}

int thp_radix_sort_u64(const unsigned long long *keys_in, const uint32_t *vals_in, uint32_t n, int begin_bit, int end_bit,
                       unsigned long long *keys_out, uint32_t *vals_out, int *in_b_out)
{
    return radix_sort<unsigned long long>(keys_in, vals_in, n, begin_bit, end_bit, keys_out, vals_out, in_b_out);
}

// n = 0 on buffers of `cap` elements of key_bytes (4 / 8): non-zero when any of the five buffers was written
int thp_radix_sort_empty(int key_bytes, uint32_t cap, int begin_bit, int end_bit, int *in_b_out)
{
    if (key_bytes == 4) return radix_sort_empty<uint32_t>(cap, begin_bit, end_bit, in_b_out);
    if (key_bytes == 8) return radix_sort_empty<unsigned long long>(cap, begin_bit, end_bit, in_b_out);
    return fail(kArgument, "key_bytes is 4 or 8");
}

// in / out / totals: rounds * N elements of elem_bytes each (totals: the total every thread was handed)
int thp_block_scan(uint32_t N, int elem_bytes, const void *in, void *out, void *totals, uint32_t rounds)
{
    if (!in || !out || !totals || rounds == 0) return fail(kArgument, "null array or no rounds");
    if (N == 256 && elem_bytes == 4) return block_scan<256, uint32_t>(in, out, totals, rounds);
    if (N == 256 && elem_bytes == 8) return block_scan<256, unsigned long long>(in, out, totals, rounds);
    if (N == 1024 && elem_bytes == 4) return block_scan<1024, uint32_t>(in, out, totals, rounds);
    if (N == 1024 && elem_bytes == 8) return block_scan<1024, unsigned long long>(in, out, totals, rounds);
    return fail(kArgument, "N is 256 or 1024, elem_bytes 4 or 8");
}

}  // extern "C"
