// th_fragline.hip - the fragment's line: what a caller's fragment stage sees of the line a fragment belongs to (th_line(f) in
// th_fragment_prelude.inc: stream index, the parameter along the line, the signed distance across it, its length).
//
// The stream-ordered pipeline drops these numbers: dep_put (th_deposit.hip) mixes the varying with dep_param's t and keeps
// neither t nor - in a local pass's 32-bit keys - the line's index.  For a pass whose stage reads the line (th_fragprog.hip:
// the program's source names th_line; every other pass launches nothing of this file) one kernel behind the scatter and in front
// of the stage sets every drawing line up again, exactly as the emit did (dep_setup: the built-in and a caller's vertex stage,
// halo rows, packed texels), and writes one 16-byte record per fragment beside the fragment's key and varying: lines[at] for the
// fragment at keys[at] / colors[at].  The texels come from the line's record (lines of up to kRecordTexels fragments) or, for
// the lines on the long list, from the keys the scatter has just written - nothing is rasterised again.
//
// Arithmetic (fp32, no contraction; the integers are dep_param's, in 1/16 texel - 32-bit where short32 proves they fit, 64-bit
// otherwise: both convert the exact integer, so both give the same floats):
//   ex = sx1 - sx0, ey = sy1 - sy0, qx = 16 x - sx0, qy = 16 y - sy0, den = ex^2 + ey^2, crs = qy ex - qx ey
//   along  = dep_param's own result (num / den)
//   len16  = sqrtf((float)den);  across = ((float)crs / len16) * 0.0625f;  length = len16 * 0.0625f
//   den == 0: along = across = length = 0
#include "th_kernels.hpp"
#include "th_raster.hpp"

namespace th {
namespace {

static_assert(sizeof(FragmentLine) == 16, "FragmentLine: th_fragment_line of th_fragment_prelude.inc, one 16-byte store a fragment");

TH_D FragmentLine line_record(const DepositLine &L, uint32_t id, int x, int y)
{
    FragmentLine r{id, 0.0f, 0.0f, 0.0f};
    float t = 0.0f;
    if (!dep_param(L, x, y, t)) return r;               // both endpoints snap to one point
    float crs, den;
    if (L.short32) {        // (dep_param's bounds: 24-bit factors, 30-bit sums)
        const int ex = L.sx[1] - L.sx[0], ey = L.sy[1] - L.sy[0];
        den = (float)(__mul24(ex, ex) + __mul24(ey, ey));
        crs = (float)(__mul24((y << 4) - L.sy[0], ex) - __mul24((x << 4) - L.sx[0], ey));
    } else {
        const long long ex = L.sx[1] - L.sx[0], ey = L.sy[1] - L.sy[0];
        den = (float)(ex * ex + ey * ey);
        crs = (float)(((long long)(y << 4) - L.sy[0]) * ex - ((long long)(x << 4) - L.sx[0]) * ey);
    }
    const float len16 = __builtin_sqrtf(den);
    r.along = t;
    r.across = (crs / len16) * 0.0625f;
    r.length = len16 * 0.0625f;
    return r;
}

// The lines of up to kRecordTexels fragments, walked as deposit_emit_kernel walks them (th_deposit.hip: patches of kPatchCols x
// kPatchRows lines, one stream column per wave, patches in column-major order): a wave's lines are 64 consecutive positions of
// the stream, so its records form ONE contiguous run of `lines` (the row-major walk cost the emit 1.2 ms against 0.3).
constexpr uint32_t kPatchCols = 8, kPatchRows = 64;

template <bool PROGRAM>
__global__ __launch_bounds__(kPatchCols * 64) void fragment_lines_kernel(const DepositParams p, FragmentLine *lines)
{
    const uint32_t patches_x = (p.W + kPatchCols - 1) / kPatchCols, patches_y = (p.rows + kPatchRows - 1) / kPatchRows;
    const uint32_t patches = patches_x * patches_y;
    for (uint32_t patch = blockIdx.x; patch < patches; patch += gridDim.x) {
        const uint32_t px = patch / patches_y, py = patch - px * patches_y;
        const uint32_t col = px * kPatchCols + (threadIdx.x >> 6), row = py * kPatchRows + (threadIdx.x & 63u);
        if (col >= p.W || row >= p.rows) continue;
        const uint32_t t = row * p.W + col;
        const uint32_t n = p.count[t];
        if (n == 0 || n > kRecordTexels) continue;
        const uint32_t id = col * p.H + p.row0 + row;
        const uint32_t at = p.offset[t];
        DepositLine L;
        dep_setup<false, PROGRAM>(p, col, p.row0 + row, L, (size_t)row * p.W + col, OwnTexels{}, false);      // (no varyings: the geometry alone)
        const uint4 ra = p.record[2u * t];
        uint4 rb = make_uint4(0u, 0u, 0u, 0u);
        if (n > 4u) rb = p.record[2u * t + 1u];
        const uint32_t xy[kRecordTexels] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
#pragma unroll
        for (uint32_t k = 0; k < kRecordTexels; ++k)
            if (k < n) lines[at + k] = line_record(L, id, (int)(xy[k] & 0xffffu), (int)(xy[k] >> 16));
    }
}

// ... and the lines of more fragments than a record holds, from the kListLong lists as deposit_emit_long_kernel takes them: a
// lane per line, the texel of fragment k from the key the scatter wrote at offset + k (the 32-bit key IS the texel; a 64-bit
// key holds it in bits 32 .. 55)
template <bool PROGRAM>
__global__ __launch_bounds__(256) void fragment_lines_long_kernel(const DepositParams p, FragmentLine *lines)
{
    dep_list_work(p, kListLong, [&](bool have, uint32_t t, uint32_t) {
        if (!have) return;
        const uint32_t row = t / p.W, col = t - row * p.W;
        const uint32_t id = col * p.H + p.row0 + row;
        const uint32_t at = p.offset[t], n = p.count[t];
        DepositLine L;
        dep_setup<false, PROGRAM>(p, col, p.row0 + row, L, (size_t)row * p.W + col, OwnTexels{}, false);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t texel = p.keys64 ? (uint32_t)(p.keys64[at + k] >> 32) & kTexelMask : p.keys[at + k];
            const uint32_t y = texel / (uint32_t)p.fw, x = texel - y * (uint32_t)p.fw;
            lines[at + k] = line_record(L, id, (int)x, (int)y);
        }
    });
}

}  // namespace

// behind launch_deposit_scatter(p), which left p.keys / p.keys64 (one of them: not a pass that reuses a sorted order); `lines`
// holds a record for every fragment of the pass
void launch_fragment_lines(const DepositParams &p, FragmentLine *lines, hipStream_t s)
{
    const uint32_t patches = ((p.W + kPatchCols - 1) / kPatchCols) * ((p.rows + kPatchRows - 1) / kPatchRows);
    const dim3 grid(patches < 65536u * 16u ? (patches ? patches : 1u) : 65536u * 16u);
    if (p.vertices) {
        hipLaunchKernelGGL(fragment_lines_kernel<true>, grid, dim3(kPatchCols * 64u), 0, s, p, lines);
        hipLaunchKernelGGL(fragment_lines_long_kernel<true>, dim3(kDepLists * 8u), dim3(256), 0, s, p, lines);
        return;
    }
    hipLaunchKernelGGL(fragment_lines_kernel<false>, grid, dim3(kPatchCols * 64u), 0, s, p, lines);
    hipLaunchKernelGGL(fragment_lines_long_kernel<false>, dim3(kDepLists * 8u), dim3(256), 0, s, p, lines);
}

}  // namespace th
