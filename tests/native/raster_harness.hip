// raster_harness.hip - test-only C entry points around the integer routines of th_raster.hpp: the scan conversions of a
// snapped polygon and the interpolation parameter of a fragment.  They are header functions: this file instantiates them,
// as the product's kernels do, and holds no copy of any of them (tests/test_raster_build.py reads this source for that).
//
// Every entry point takes and returns HOST arrays: allocation, copies, the launch on a stream of its own, the synchronisation
// and every HIP status check live here.  They return 0, or a code (kHip, kGuard, kArgument) and leave thr_last_error().
// Every device buffer is allocated with kGuardBytes of a known pattern behind its stated size; a changed guard is kGuard.
//
// The routines read fw and fh of DepositParams and nothing else of it.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "th_raster.hpp"

namespace {

enum { kOk = 0, kHip = 1, kGuard = 2, kArgument = 3 };
constexpr size_t kGuardBytes = 256;
constexpr int kGuardByte = 0xA5;

thread_local std::string g_error;

int fail(int code, const std::string &why) { g_error = why; return code; }

#define THR_HIP(expr)                                                                                              \
    do {                                                                                                           \
        const hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return fail(kHip, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)
#define THR_TRY(expr) do { if (const int s_ = (expr)) return s_; } while (0)

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
    int start() { THR_HIP(hipStreamCreate(&stream)); return kOk; }
    int alloc(Guarded &g, const char *name, size_t bytes, bool zero)
    {
        g.name = name; g.bytes = bytes;
        THR_HIP(hipMalloc((void **)&g.p, bytes + kGuardBytes));
        buffers.push_back(&g);
        if (zero && bytes) THR_HIP(hipMemsetAsync(g.p, 0, bytes, stream));
        THR_HIP(hipMemsetAsync(g.p + bytes, kGuardByte, kGuardBytes, stream));
        return kOk;
    }
    int upload(Guarded &g, const void *src)
    {
        if (g.bytes) THR_HIP(hipMemcpyAsync(g.p, src, g.bytes, hipMemcpyHostToDevice, stream));
        return kOk;
    }
    int download(void *dst, const Guarded &g)
    {
        if (g.bytes) THR_HIP(hipMemcpyAsync(dst, g.p, g.bytes, hipMemcpyDeviceToHost, stream));
        return kOk;
    }
    int finish()
    {
        THR_HIP(hipGetLastError());
        THR_HIP(hipStreamSynchronize(stream));
        return kOk;
    }
    int guards()
    {
        unsigned char host[kGuardBytes];
        for (const Guarded *g : buffers) {
            THR_HIP(hipMemcpy(host, g->p + g->bytes, kGuardBytes, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < kGuardBytes; ++k)
                if (host[k] != (unsigned char)kGuardByte) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "guard behind %s (%zu bytes) changed at byte +%zu: 0x%02x", g->name, g->bytes, k, host[k]);
                    return fail(kGuard, msg);
                }
        }
        return kOk;
    }
};

// ---- spans ------------------------------------------------------------------------------------------------------------------
enum { kPoly6 = 0, kPoly0 = 1, kSmallHexagon = 2, kSmallHexagon2 = 3, kRowSpan = 4, kTriSpan = 5, kVariants = 6 };
constexpr int kMaxVertices = 12;       // the stride of X and Y: the clipper's lists hold up to 12 points
constexpr int kHeadWords = 8, kRowWords = 4;
// head: { verdict (-1: the variant asks none), ymin, ymax, first row of the window, texels, strays, rows out of order, rows asked }
// row:  { texels, least x, greatest x, texels that did not come after their predecessor }

// What a polygon's lane keeps of the texels it is handed: the row in hand in registers, merged into the polygon's window of
// `cap` rows when another row begins.  A texel outside the window or outside [0, fw) is a stray: counted, stored nowhere.
struct Tally {
    int *head, *rows;
    int base, cap, fw;
    int y, n, lo, hi, back, last;
    bool open;
    int texels, strays, again, asked;          // (head[4..7]: in registers until finish())
    __device__ void flush()
    {
        if (!open) return;
        int *r = rows + (size_t)(y - base) * kRowWords;
        if (r[0] == 0) { r[1] = lo; r[2] = hi; }
        else { r[1] = lo < r[1] ? lo : r[1]; r[2] = hi > r[2] ? hi : r[2]; again += 1; }       // (the row came a second time)
        r[0] += n; r[3] += back;
        open = false;
    }
    __device__ void add(int x, int yy)
    {
        texels += 1;
        if (yy < base || yy >= base + cap || x < 0 || x >= fw) { strays += 1; return; }
        if (!open || yy != y) {
            if (open && yy < y) again += 1;
            flush();
            open = true; y = yy; n = 0; lo = x; hi = x; back = 0; last = x - 1;
        }
        back += x > last ? 0 : 1;
        last = x;
        lo = x < lo ? x : lo; hi = x > hi ? x : hi;
        ++n;
    }
    __device__ void span(int yy, int left, int right)          // (a routine that hands a row's span over, not its texels)
    {
        asked += 1;
        for (int x = left; x < right; ++x) add(x, yy);
    }
    __device__ void finish() { flush(); head[4] = texels; head[5] = strays; head[6] = again; head[7] = asked; }
};

__global__ __launch_bounds__(256) void spans_kernel(int variant, int fw, int fh, int count, int cap, const int *nv, const int *X,
                                                    const int *Y, int *head, int *rows)
{
    __shared__ float lds[48 * 256];                         // (kPoly0: the polygon where the slow kernels hold it)
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= count) return;
    th::DepositParams p{};
    p.fw = fw; p.fh = fh;
    const int n = nv[t];
    const int *x = X + (size_t)t * kMaxVertices, *y = Y + (size_t)t * kMaxVertices;
    int ymin = y[0], ymax = y[0];
    for (int k = 1; k < n; ++k) { ymin = y[k] < ymin ? y[k] : ymin; ymax = y[k] > ymax ? y[k] : ymax; }
    int r0 = (ymin + 15) >> 4, r1 = (ymax + 15) >> 4;
    r0 = r0 < 0 ? 0 : r0; r1 = r1 > fh ? fh : r1;
    Tally tally{head + (size_t)t * kHeadWords, rows + (size_t)t * cap * kRowWords, r0, cap, fw, 0, 0, 0, 0, 0, 0, false, 0, 0, 0, 0};
    int *h = tally.head;
    h[0] = -1; h[1] = ymin; h[2] = ymax; h[3] = r0;
    auto emit = [&](int ex, int ey) { tally.add(ex, ey); };
    int PX[6], PY[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { PX[k] = x[k]; PY[k] = y[k]; }
    if (variant == kPoly6) th::dep_raster_poly<6>(p, PX, PY, 6, emit);
    else if (variant == kPoly0) {
        th::LdsWords<256> w{lds + threadIdx.x};
        for (int k = 0; k < n; ++k) { w.i(24 + k) = x[k]; w.i(36 + k) = y[k]; }
        th::dep_raster_poly<0>(p, th::PolygonX<th::LdsWords<256>>{w}, th::PolygonY<th::LdsWords<256>>{w}, n, emit);
    } else if (variant == kTriSpan) {
        // every row of the target the polygon can reach, and one to either side: tri_span is asked about rows it does not cover
        for (int row = r0 > 0 ? r0 - 1 : 0; row < (r1 < fh ? r1 + 1 : fh); ++row) {
            int left, right;
            th::tri_span(n, x, y, row, fw, left, right);
            tally.span(row, left, right);
        }
    } else {
        int hmin, hmax;
        const bool small = th::dep_hexagon_is_small(PX, PY, hmin, hmax);
        h[0] = small ? 1 : 0; h[1] = hmin; h[2] = hmax;
        if (small) {
            if (variant == kSmallHexagon) th::dep_raster_small_hexagon(p, PX, PY, hmin, hmax, emit);
            else if (variant == kSmallHexagon2) th::dep_raster_small_hexagon2(p, PX, PY, hmin, hmax, emit);
            else {
                // (th_bins.hip bins_fused_kernel: the rows of a small hexagon, dealt one by one)
                int q0 = (hmin + 15) >> 4, q1 = (hmax + 15) >> 4;
                q0 = q0 < 0 ? 0 : q0; q1 = q1 > p.fh ? p.fh : q1;
                for (int row = q0; row < q1; ++row) {
                    int left, right;
                    th::dep_hexagon_row_span(p, PX, PY, row, left, right);
                    tally.span(row, left, right);
                }
            }
        }
    }
    tally.finish();
}

// ---- dep_param --------------------------------------------------------------------------------------------------------------
// The line is set up by dep_setup itself, from vertex records as a caller's draw program leaves them (dep_vertex_read: W lines of
// one row, two records of two float4 per line), on a kParamView x kParamView target; `short32` is what dep_setup left.
// out: { short32, dep_param's verdict, bits of t, verdict and bits of t with short32 forced false, the snapped endpoints }
constexpr int kParamView = 4096, kParamWords = 9;
__global__ __launch_bounds__(256) void param_kernel(int count, const float4 *vertices, const int *x, const int *y, uint32_t *out)
{
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= count) return;
    th::DepositParams p{};
    p.fw = kParamView; p.fh = kParamView;
    p.W = (uint32_t)count; p.H = 1u; p.row0 = 0u; p.rows = 1u;
    p.vertices = vertices;
    th::DepositLine L;
    L.sx[0] = L.sx[1] = L.sy[0] = L.sy[1] = 0x7fffffff;
    th::dep_setup<false, true>(p, (uint32_t)t, 0u, L, (size_t)t, th::OwnTexels{}, false);
    uint32_t *o = out + (size_t)t * kParamWords;
    o[5] = (uint32_t)L.sx[0]; o[6] = (uint32_t)L.sy[0]; o[7] = (uint32_t)L.sx[1]; o[8] = (uint32_t)L.sy[1];
    float v = 0.0f;
    o[0] = L.short32 ? 1u : 0u;
    o[1] = th::dep_param(L, x[t], y[t], v) ? 1u : 0u;
    o[2] = __float_as_uint(v);
    o[3] = o[1]; o[4] = o[2];
    if (L.short32) {
        L.short32 = false;
        float wide = 0.0f;
        o[3] = th::dep_param(L, x[t], y[t], wide) ? 1u : 0u;
        o[4] = __float_as_uint(wide);
    }
}

}  // namespace

extern "C" {

const char *thr_last_error(void) { return g_error.c_str(); }

// count polygons, vertex k of polygon t at X / Y[t * 12 + k], nv[t] vertices (6 for every variant but 1 and 5).  head: count * 8
// words, rows: count * cap * 4 words (the layouts above); a polygon's window starts at its first row inside the target.
int thr_spans(int variant, int fw, int fh, int count, int cap, const int *nv, const int *X, const int *Y, int *head, int *rows)
{
    if (variant < 0 || variant >= kVariants || fw < 1 || fh < 1 || count < 1 || cap < 1 || !nv || !X || !Y || !head || !rows)
        return fail(kArgument, "variant 0..5, a target, polygons, a window and five arrays");
    for (int t = 0; t < count; ++t) {
        const bool general = variant == kPoly0 || variant == kTriSpan;
        if (general ? (nv[t] < 3 || nv[t] > kMaxVertices) : nv[t] != 6) return fail(kArgument, "vertex count outside the variant's contract");
    }
    Job job;
    THR_TRY(job.start());
    Guarded dn, dx, dy, dh, dr;
    THR_TRY(job.alloc(dn, "nv", (size_t)count * sizeof(int), false));
    THR_TRY(job.alloc(dx, "X", (size_t)count * kMaxVertices * sizeof(int), false));
    THR_TRY(job.alloc(dy, "Y", (size_t)count * kMaxVertices * sizeof(int), false));
    THR_TRY(job.alloc(dh, "head", (size_t)count * kHeadWords * sizeof(int), true));
    THR_TRY(job.alloc(dr, "rows", (size_t)count * cap * kRowWords * sizeof(int), true));
    THR_TRY(job.upload(dn, nv));
    THR_TRY(job.upload(dx, X));
    THR_TRY(job.upload(dy, Y));
    hipLaunchKernelGGL(spans_kernel, dim3(((uint32_t)count + 255u) / 256u), dim3(256), 0, job.stream, variant, fw, fh, count, cap,
                       reinterpret_cast<const int *>(dn.p), reinterpret_cast<const int *>(dx.p), reinterpret_cast<const int *>(dy.p),
                       reinterpret_cast<int *>(dh.p), reinterpret_cast<int *>(dr.p));
    THR_TRY(job.download(head, dh));
    THR_TRY(job.download(rows, dr));
    THR_TRY(job.finish());
    return job.guards();
}

// count lines (snapped endpoints, sixteenths) with a fragment (texel) each; out: count * 9 words.  The endpoints reach dep_setup
// as the clip-space positions that snap to them on the kParamView target: (s - 32760) / 32768, exact in a float for the
// |s - 32760| < 2^24 this takes, and snapped back without a rounding.  Two equal endpoints a little off the centre are given
// positions 2^-20 apart (a thirty-second of a sixteenth), so that dep_setup draws the line and both snap to the one point.
int thr_param(int count, const int *sx0, const int *sy0, const int *sx1, const int *sy1, const int *x, const int *y, uint32_t *out)
{
    if (count < 1 || !sx0 || !sy0 || !sx1 || !sy1 || !x || !y || !out) return fail(kArgument, "lines, fragments and seven arrays");
    const int off = 8 * kParamView - 8;
    const float scale = 8.0f * (float)kParamView;
    std::vector<float> rec((size_t)count * 16u, 0.0f);
    const uint32_t one = 1u;
    for (int t = 0; t < count; ++t) {
        const int s[4] = {sx0[t], sy0[t], sx1[t], sy1[t]};
        for (int k = 0; k < 4; ++k)
            if (s[k] - off <= -(1 << 24) || s[k] - off >= (1 << 24)) return fail(kArgument, "an endpoint more than 2^24 sixteenths off the centre");
        float *a = &rec[(size_t)t * 16u], *b = a + 8;
        a[0] = (float)(s[0] - off) / scale; a[1] = (float)(s[1] - off) / scale;
        b[0] = (float)(s[2] - off) / scale; b[1] = (float)(s[3] - off) / scale;
        if (s[0] == s[2] && s[1] == s[3] && a[0] > -4.0f && a[0] < 4.0f) b[0] = a[0] + 0x1p-20f;
        memcpy(&a[2], &one, 4); memcpy(&b[2], &one, 4);                   // live
    }
    Job job;
    THR_TRY(job.start());
    Guarded dv, dx, dy, dout;
    THR_TRY(job.alloc(dv, "vertices", rec.size() * sizeof(float), false));
    THR_TRY(job.alloc(dx, "x", (size_t)count * sizeof(int), false));
    THR_TRY(job.alloc(dy, "y", (size_t)count * sizeof(int), false));
    THR_TRY(job.alloc(dout, "out", (size_t)count * kParamWords * sizeof(uint32_t), true));
    THR_TRY(job.upload(dv, rec.data()));
    THR_TRY(job.upload(dx, x));
    THR_TRY(job.upload(dy, y));
    hipLaunchKernelGGL(param_kernel, dim3(((uint32_t)count + 255u) / 256u), dim3(256), 0, job.stream, count,
                       reinterpret_cast<const float4 *>(dv.p), reinterpret_cast<const int *>(dx.p), reinterpret_cast<const int *>(dy.p),
                       reinterpret_cast<uint32_t *>(dout.p));
    THR_TRY(job.download(out, dout));
    THR_TRY(job.finish());
    return job.guards();
}

}  // extern "C"
