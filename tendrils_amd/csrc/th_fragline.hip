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
//
// The binned pipeline (th_bins.hip) keeps no stream-ordered array: between its emit and its blends a fragment lies at a PLACE of
// the page store, under a key that holds its texel and its line's stream index.  Under TH_OPT_LINE_BINS a stage that reads the
// line runs there too, over records written by the two kernels at the end of this file: fragment_line_ends_kernel walks the slots
// as the emit walked them and leaves every drawing line's four snapped integers in a table by stream index; fragment_lines_bins_kernel
// walks the places by the walk the stage's own kernel is compiled from (th_bins_walk.inc), looks a place's line up by the key's low word and writes line_record()'s
// result beside the key.  The numbers are line_record's from dep_setup's integers: the stream-ordered records, bit for bit.
#include "th_kernels.hpp"
#include "th_raster.hpp"
#include "th_bins_places.hpp"

namespace th {
namespace {

// the walk over a binned pass's page store: the text th_fragprog.hip hands to hiprtc in front of a fragment program, here as code
#define TH_BINS_WALK(...) __VA_ARGS__
#include "th_bins_walk.inc"
#undef TH_BINS_WALK
static_assert(th_bins_replicas == kBinReplicas && th_bins_page_shift == kPageShift && th_bins_tot_oob == kTotOob && th_bins_tot_flags == kTotFlags &&
              kBinsMaxExtent == 1 << 12, "th_bins_walk.inc holds the bins' constants, and a key's x and y are 12-bit fields");

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

// ---- the records of a BINNED pass ----------------------------------------------------------------------------------------------
// Kernel A: the snapped endpoints of every line that draws, by stream index.  The walk is bins_fused_kernel's: a workgroup of 256
// per listed block of slots, the blocks the step saw leave the view skipped, slot s's particle by slot_particle, its line by
// dep_setup - the geometry alone (the built-in stage over `perm`, LineSources tables and packed texels; a vertex program's
// records in texel order).  A line that does not draw has no fragment and its entry is never read: the table is not cleared.
// Two 16-byte state loads (or the records) and one 16-byte store a lane; no LDS, no atomics; *p.oob only where the emit set it
// (the same dep_fetch).
template <bool PROGRAM>
__global__ __launch_bounds__(256) void fragment_line_ends_kernel(const DepositParams p, int4 *ends)
{
    if (blockIdx.x >= p.draw_nblocks) return;
    const uint32_t block = p.draw_blocks[blockIdx.x];
    if (p.block_seen && p.block_seen[block] == 0u) return;
    const uint32_t s = block * 256u + threadIdx.x;
    uint32_t col = 0, row = 0;
    if (!(s < p.W * p.rows && slot_particle<PROGRAM>(p, s, col, row))) return;
    DepositLine L;
    dep_setup<false, PROGRAM>(p, col, p.row0 + row, L, s, OwnTexels{}, false);
    if (L.draws) ends[(size_t)col * p.H + p.row0 + row] = make_int4(L.sx[0], L.sy[0], L.sx[1], L.sy[1]);
}

// Kernel B: lines[place] for every live place of the store, by th_bins_walk - the places the stage's kernel will visit - less a
// key whose low word is no line of this texture (none is written: the table's bound, checked where it is indexed).  Per lane: the
// 8-byte key (x, y, line: its fields), the dependent 16-byte load of the line's endpoints, line_record, one 16-byte store.
// Nothing is written but lines[place] of live places.
__global__ __launch_bounds__(256) void fragment_lines_bins_kernel(const DepositParams p, const int4 *ends, FragmentLine *lines)
{
    const th_bins_store store{p.frag_keys, p.bin_cursor, p.page_table, p.totals, p.bin_stride, p.max_pages, p.nbins, p.nbins * kBinReplicas + p.pool_pages};
    const uint32_t nlines = p.W * p.H;
    th_bins_walk(store, [&](unsigned long long key, uint32_t at) {
        const uint32_t id = (uint32_t)key;
        if (id >= nlines) return;
        const int4 e = ends[id];
        DepositLine L;
        L.sx[0] = e.x; L.sy[0] = e.y; L.sx[1] = e.z; L.sy[1] = e.w;
        const int ex = L.sx[1] - L.sx[0], ey = L.sy[1] - L.sy[0];       // (dep_setup's own expression: either branch converts the exact integers)
        L.short32 = ex > -(1 << 14) && ex < (1 << 14) && ey > -(1 << 14) && ey < (1 << 14);
        lines[at] = line_record(L, id, (int)((uint32_t)(key >> 32) & 0xfffu), (int)((uint32_t)(key >> 44) & 0xfffu));
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

// behind launch_bins_fused(p, s, program) on the same stream: `ends` holds p.W * p.H entries
void launch_fragment_line_ends(const DepositParams &p, int4 *ends, hipStream_t s, bool program)
{
    const dim3 grid(p.draw_nblocks ? p.draw_nblocks : 1u);
    if (program) hipLaunchKernelGGL(fragment_line_ends_kernel<true>, grid, dim3(256), 0, s, p, ends);
    else hipLaunchKernelGGL(fragment_line_ends_kernel<false>, grid, dim3(256), 0, s, p, ends);
}

// ... and behind that: `lines` holds a record for every place of the store p.frag_keys names
void launch_fragment_lines_bins(const DepositParams &p, const int4 *ends, FragmentLine *lines, int deal, hipStream_t s)
{
    hipLaunchKernelGGL(fragment_lines_bins_kernel, dim3(p.nbins ? p.nbins : 1u, (uint32_t)deal), dim3(256), 0, s, p, ends, lines);
}

}  // namespace th
