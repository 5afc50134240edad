// th_flowline.hip - flow lines: the reference's FlowLine / FlowLines (src/flow-line/index.js, multi.js) drawn into the
// context's flow texture.
//
// Host side: th_flow_line_attributes restates Line.update() + FlowLine.setAttributes (polyline-normals in double, as the
// reference's JS computes it, stored as f32 attributes).  th_flow_lines packs one record per drawn path point (a strip
// vertex pair shares it) and uploads them through a pinned staging buffer.
//
// Device side, all on the context's stream:
//   fl_setup_kernel   one thread per strip triangle: the vertex stage of src/flow-line/index.vert in fp32 for its three
//                     vertices, clip / snap / orient as the GeometrySpawner triangles (th_raster.hpp:tri_clip_snap),
//                     the barycentric set-up of the varyings, the triangle's 16 x 16-texel tile box; counts its tiles
//                     per (tile, chunk of triangles)
//   (scan)            exclusive scan of those counts (th_sort.hip:launch_exclusive_scan_u32; tile-major, chunk-minor):
//                     where every chunk's run of a tile's list starts
//   fl_fill_kernel    one workgroup per chunk, one thread per (triangle, tile) pair: the triangle's rank among the chunk's
//                     earlier triangles on that tile, so that each tile's list is in primitive order
//   fl_raster_kernel  one workgroup per tile, one thread per texel: reads its texel once, walks the tile's list in order,
//                     64 triangles at a time staged in LDS (their row spans, th_raster.hpp:tri_span, and varying set-ups), shades
//                     (src/flow-line/index.frag) and blends SRC_ALPHA / ONE_MINUS_SRC_ALPHA in registers, writes back once
//                     if anything covered it.
#include "th_ctx.hpp"
#include "th_raster.hpp"

namespace {

constexpr int kTile = 16;                  // texels per tile side (one 256-thread workgroup per tile)
constexpr int kChunkMin = 64;              // triangles per chunk of the fill (widened for large calls)
constexpr int kStage = 64;                 // triangles staged in LDS per round of the raster kernel
constexpr uint32_t kMaxCountCells = 1u << 24;   // (tile, chunk) counters at most; chunks widen to stay under it

struct FlPoint {                           // one drawn path point: both strip vertices of it
    float px, py, nx, ny, miter, qx, qy, time, dt;
};

struct FlTri {                             // a set-up triangle
    // barycentrics from the SNAPPED unclipped vertices (what the captured rasteriser interpolates with), in double:
    // dx = 16 x - X0, dy = 16 y - Y0, l1 = (dx e2y - dy e2x) inv, l2 = (dy e1x - dx e1y) inv
    double X0, Y0, e1x, e1y, e2x, e2y, inv;
    float v0[7], d1[7], d2[7];             // varyings (values.rgba, crest.xy, sdf) at vertex 0 and their differences to 1 and 2
    th::TrianglePoly P;                    // the clipped, snapped polygon (P.n 0: draws nothing)
};

struct FlParams {
    const FlPoint *pts;
    const int32_t *line_tri;               // [nlines + 1] first triangle of every line
    const int32_t *line_pt;                // [nlines] first point record of every line
    int32_t nlines, ntri;
    float speed, rad, crest_shape, speed_limit, view_x, view_y;
    int32_t w, h, tiles_x, tiles_y;
    uint32_t nchunks, chunk;               // triangles per chunk
    FlTri *tris;
    uint32_t *box;                         // [ntri] tile box: x0 | x1 << 16, y0 | y1 << 16 (empty: x0 > x1)
    uint32_t *counts;                      // [ntiles * nchunks + 1] -> exclusive scan
    uint32_t *list;                        // triangles of every tile, in primitive order
    uint32_t list_cap;                     // its capacity (the host's bound; a write past it is dropped, never made)
    float4 *flow;
};

// src/flow-line/index.vert (+ src/flow/apply/state.glsl, src/geom/line/expand/index.glsl), in the shader's order
__device__ __forceinline__ void fl_vertex(const FlParams &p, const FlPoint &q, int side, float &cx, float &cy, float (&v)[7])
{
    const float miter = side ? q.miter : -q.miter;
    const float sdf = miter > 0.0f ? 1.0f : (miter < 0.0f ? -1.0f : 0.0f);
    const float rate = p.speed / __builtin_fmaxf(q.dt, 1.0f);
    const float vx = (q.px - q.qx) * rate, vy = (q.py - q.qy) * rate;
    const float len = __builtin_sqrtf(vx * vx + vy * vy);
    const float a = __builtin_fminf(len / p.speed_limit, 1.0f);
    const float r = p.rad * a;
    cx = (q.px + q.nx * r * miter) * p.view_x;
    cy = (q.py + q.ny * r * miter) * p.view_y;
    v[0] = vx; v[1] = vy; v[2] = q.time; v[3] = a;
    v[4] = q.nx * miter; v[5] = q.ny * miter; v[6] = sdf;
}

__global__ __launch_bounds__(256) void fl_setup_kernel(const FlParams p)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.ntri) return;
    int lo = 0, hi = p.nlines - 1;                         // the line of triangle t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.line_tri[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int j = t - p.line_tri[lo];                     // strip vertices j, j+1, j+2 of the line
    float cx[12], cy[12], v[3][7];
    for (int k = 0; k < 3; ++k) {
        const int vert = j + k;
        fl_vertex(p, p.pts[p.line_pt[lo] + (vert >> 1)], vert & 1, cx[k], cy[k], v[k]);
    }
    FlTri &T = p.tris[t];
    uint32_t bx = 0xffffu, by = 0xffffu;                   // (empty box: x0 = 0xffff > x1 = 0)
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && __builtin_isfinite(cx[k]) && __builtin_isfinite(cy[k]);
    const float wx16 = 8.0f * (float)p.w, wy16 = 8.0f * (float)p.h;
    const float ox = wx16 - 8.0f, oy = wy16 - 8.0f;
    // the snapped unclipped vertices: the varyings' barycentric set-up
    double SX[3], SY[3];
    for (int k = 0; k < 3; ++k) { SX[k] = (double)__builtin_rintf(cx[k] * wx16 + ox); SY[k] = (double)__builtin_rintf(cy[k] * wy16 + oy); }
    int X[7], Y[7];
    const int n = th::tri_clip_snap(cx, cy, finite ? 3 : 0, p.w, p.h, X, Y);
    T.P.n = 0;
    if (n) {
        int minx = X[0], maxx = X[0], miny = Y[0], maxy = Y[0];
        for (int k = 0; k < n; ++k) {
            T.P.x[k] = X[k]; T.P.y[k] = Y[k];
            minx = min(minx, X[k]); maxx = max(maxx, X[k]); miny = min(miny, Y[k]); maxy = max(maxy, Y[k]);
        }
        // texels the spans can reach: ceil(X / 16) <= x < ceil(maxX / 16), the same for rows
        const int x0 = max((minx + 15) >> 4, 0), x1 = min(((maxx + 15) >> 4) - 1, p.w - 1);
        const int y0 = max((miny + 15) >> 4, 0), y1 = min(((maxy + 15) >> 4) - 1, p.h - 1);
        if (x0 <= x1 && y0 <= y1) {
            T.P.n = n;
            bx = (uint32_t)(x0 / kTile) | ((uint32_t)(x1 / kTile) << 16);
            by = (uint32_t)(y0 / kTile) | ((uint32_t)(y1 / kTile) << 16);
        }
    }
    if (T.P.n) {
        const double e1x = SX[1] - SX[0], e1y = SY[1] - SY[0], e2x = SX[2] - SX[0], e2y = SY[2] - SY[0];
        const double det = e1x * e2y - e2x * e1y;
        T.X0 = SX[0]; T.Y0 = SY[0]; T.e1x = e1x; T.e1y = e1y; T.e2x = e2x; T.e2y = e2y;
        T.inv = det != 0.0 ? 1.0 / det : 0.0;
        for (int k = 0; k < 7; ++k) { T.v0[k] = v[0][k]; T.d1[k] = v[1][k] - v[0][k]; T.d2[k] = v[2][k] - v[0][k]; }
    }
    p.box[2 * t] = bx; p.box[2 * t + 1] = by;
    if (!T.P.n) return;
    const uint32_t chunk = (uint32_t)t / p.chunk;
    for (uint32_t ty = by & 0xffffu; ty <= (by >> 16); ++ty)
        for (uint32_t tx = bx & 0xffffu; tx <= (bx >> 16); ++tx)
            atomicAdd(&p.counts[((size_t)ty * p.tiles_x + tx) * p.nchunks + chunk], 1u);
}

// src/flow-line/index.frag at one texel (sx, sy: its centre in 1/16 texels) + the blend into d
__device__ __forceinline__ void fl_shade_blend(float4 &d, const double *g, const float *s, double sx, double sy, float crest_shape)
{
    const double dx = sx - g[0], dy = sy - g[1];
    const float l1 = (float)((dx * g[5] - dy * g[4]) * g[6]), l2 = (float)((dy * g[2] - dx * g[3]) * g[6]);
    float v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = s[c] + l1 * s[7 + c] + l2 * s[14 + c];
    const float dd = __builtin_fabsf(v[6]);
    const float speed = __builtin_sqrtf(v[0] * v[0] + v[1] * v[1]) * (1.0f - dd);
    const float t = dd * crest_shape;
    const float mx = v[0] * (1.0f - t) + v[4] * t, my = v[1] * (1.0f - t) + v[5] * t;
    const float inv = 1.0f / __builtin_sqrtf(mx * mx + my * my);
    const float ox = mx * inv * speed, oy = my * inv * speed, oz = v[2], ow = v[3] - dd;
    const float da = 1.0f - ow;
    d.x = ox * ow + d.x * da; d.y = oy * ow + d.y * da; d.z = oz * ow + d.z * da; d.w = ow * ow + d.w * da;
}

// The comparison arm of tools/flow_line_bench.py (TH_FLOWLINE_NAIVE=1): no bins, every texel walks every triangle in
// order, as the GeometrySpawner's triangle_fill_kernel does.  Same results as the binned path.
__global__ __launch_bounds__(256) void fl_naive_kernel(const FlParams p)
{
    const uint32_t texels = (uint32_t)p.w * (uint32_t)p.h;
    for (uint32_t texel = blockIdx.x * 256u + threadIdx.x; texel < texels; texel += gridDim.x * 256u) {
        const int y = (int)(texel / (uint32_t)p.w), x = (int)(texel - (uint32_t)y * (uint32_t)p.w);
        float4 d = p.flow[texel];
        bool touched = false;
        for (int t = 0; t < p.ntri; ++t) {
            const FlTri &T = p.tris[t];
            int left, right;
            th::tri_span(T.P.n, T.P.x, T.P.y, y, p.w, left, right);
            if (x < left || x >= right) continue;
            fl_shade_blend(d, &T.X0, T.v0, 16.0 * (double)x, 16.0 * (double)y, p.crest_shape);
            touched = true;
        }
        if (touched) p.flow[texel] = d;
    }
}

// ---- stable fill: a triangle's place on each of its tiles = the chunk's run start + its earlier chunk-mates there --------
// One workgroup per chunk; the chunk's (triangle, tile) pairs are spread over its threads (a scan of the boxes' areas in
// LDS finds a pair's triangle), each pair counting the earlier boxes of the chunk that hold its tile.
__global__ __launch_bounds__(256) void fl_fill_kernel(const FlParams p)
{
    extern __shared__ uint32_t sfill[];                    // [chunk][2] boxes | [chunk] inclusive scan of their areas
    __shared__ uint32_t part[256];
    const uint32_t chunk = blockIdx.x, first = chunk * p.chunk;
    const uint32_t m = min(p.chunk, (uint32_t)p.ntri - first);
    uint32_t *sbox = sfill, *sarea = sfill + 2 * p.chunk;
    const uint32_t per = (m + 255u) / 256u;                // boxes per thread in the scan
    uint32_t run = 0;
    for (uint32_t k = threadIdx.x * per; k < min(m, (threadIdx.x + 1u) * per); ++k) {
        const uint32_t bx = p.box[2 * (first + k)], by = p.box[2 * (first + k) + 1];
        sbox[2 * k] = bx; sbox[2 * k + 1] = by;
        const uint32_t x0 = bx & 0xffffu, x1 = bx >> 16, y0 = by & 0xffffu, y1 = by >> 16;
        run += x0 > x1 ? 0u : (x1 - x0 + 1u) * (y1 - y0 + 1u);
        sarea[k] = run;
    }
    uint32_t pairs;                                        // (the chunk's pairs: the sum of its boxes' areas)
    const uint32_t before = th::block_scan<256>(part, run, pairs);
    for (uint32_t k = threadIdx.x * per; k < min(m, (threadIdx.x + 1u) * per); ++k) sarea[k] += before;
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < pairs; q += 256u) {
        uint32_t lo = 0, hi = m - 1;                       // the first triangle whose inclusive area sum exceeds q
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sarea[mid] > q) hi = mid; else lo = mid + 1;
        }
        const uint32_t k = lo, j = q - (k ? sarea[k - 1] : 0u);
        const uint32_t bx = sbox[2 * k], by = sbox[2 * k + 1];
        const uint32_t x0 = bx & 0xffffu, x1 = bx >> 16, y0 = by & 0xffffu;
        const uint32_t bw = x1 - x0 + 1u;
        const uint32_t tx = x0 + j % bw, ty = y0 + j / bw;
        uint32_t rank = 0;
        for (uint32_t e = 0; e < k; ++e) {
            const uint32_t ex = sbox[2 * e], ey = sbox[2 * e + 1];
            rank += (tx >= (ex & 0xffffu)) & (tx <= (ex >> 16)) & (ty >= (ey & 0xffffu)) & (ty <= (ey >> 16));
        }
        const uint32_t at = p.counts[((size_t)ty * p.tiles_x + tx) * p.nchunks + chunk] + rank;
        if (at < p.list_cap) p.list[at] = first + k;
    }
}

// ---- raster, shade, blend: one workgroup per tile --------------------------------------------------------------------
__global__ __launch_bounds__(256) void fl_raster_kernel(const FlParams p)
{
    __shared__ int span_l[kStage][kTile], span_r[kStage][kTile];
    __shared__ double shd[kStage][7];
    __shared__ float shf[kStage][21];
    const uint32_t tile = blockIdx.x;
    const uint32_t begin = p.counts[(size_t)tile * p.nchunks], end = min(p.counts[(size_t)(tile + 1) * p.nchunks], p.list_cap);
    if (begin >= end) return;
    const int tx = (int)(tile % (uint32_t)p.tiles_x), ty = (int)(tile / (uint32_t)p.tiles_x);
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 4;
    const int x = tx * kTile + lx, y = ty * kTile + ly;
    const bool inside = x < p.w && y < p.h;
    float4 d = inside ? p.flow[(size_t)y * p.w + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool touched = false;
    const double sx = 16.0 * (double)x, sy = 16.0 * (double)y;
    for (uint32_t base = begin; base < end; base += kStage) {
        const uint32_t m = min((uint32_t)kStage, end - base);
        // row spans: (triangle, row) pairs, 4 per thread
        for (uint32_t q = threadIdx.x; q < m * kTile; q += 256u) {
            const uint32_t k = q >> 4;
            const int row = ty * kTile + (int)(q & 15u);
            const th::TrianglePoly &P = p.tris[p.list[base + k]].P;
            int left, right;
            th::tri_span(P.n, P.x, P.y, row, p.w, left, right);
            span_l[k][q & 15u] = left;
            span_r[k][q & 15u] = right;
        }
        for (uint32_t q = threadIdx.x; q < m * 28u; q += 256u) {
            const uint32_t k = q / 28u, f = q - k * 28u;
            const FlTri &T = p.tris[p.list[base + k]];
            if (f < 7u) shd[k][f] = (&T.X0)[f]; else shf[k][f - 7u] = (&T.v0[0])[f - 7u];
        }
        __syncthreads();
        if (inside)
            for (uint32_t k = 0; k < m; ++k) {
                if (x < span_l[k][ly] || x >= span_r[k][ly]) continue;
                fl_shade_blend(d, shd[k], shf[k], sx, sy, p.crest_shape);
                touched = true;
            }
        __syncthreads();
    }
    if (touched) p.flow[(size_t)y * p.w + x] = d;
}

// ---- host: polyline-normals (double) + Line.update / FlowLine.setAttributes --------------------------------------------
struct V2 { double x, y; };
inline V2 sub(V2 a, V2 b) { return {a.x - b.x, a.y - b.y}; }
inline V2 unit(V2 v)                           // gl-vec2 normalize: a zero vector stays zero
{
    double l2 = v.x * v.x + v.y * v.y;
    if (l2 > 0) { l2 = 1 / std::sqrt(l2); v.x = v.x * l2; v.y = v.y * l2; }
    return v;
}
inline V2 direction(V2 a, V2 b) { return unit(sub(a, b)); }
inline V2 perp(V2 d) { return {-d.y, d.x}; }
inline double miter_of(V2 A, V2 B, V2 &miter)
{
    const V2 t = unit({A.x + B.x, A.y + B.y});
    miter = {-t.y, t.x};
    const V2 tmp = {-A.y, A.x};
    return 1 / (miter.x * tmp.x + miter.y * tmp.y);
}

// polyline-normals(points, closed): per drawn point, the normal and the miter length (closed: the first repeated at the end)
void line_normals(const float *pts, int n, bool closed, std::vector<V2> &nrm, std::vector<double> &len)
{
    std::vector<V2> P(n);
    for (int i = 0; i < n; ++i) P[i] = {(double)pts[2 * i], (double)pts[2 * i + 1]};
    if (closed) P.push_back(P[0]);
    const int total = (int)P.size();
    nrm.clear(); len.clear();
    V2 cur{0, 0}, A{0, 0}, B{0, 0}, miter{0, 0};
    bool have = false;
    for (int i = 1; i < total; ++i) {
        A = direction(P[i], P[i - 1]);
        if (!have) { cur = perp(A); have = true; }
        if (i == 1) { nrm.push_back(cur); len.push_back(1); }
        if (i < total - 1) {
            B = direction(P[i + 1], P[i]);
            const double m = miter_of(A, B, miter);
            nrm.push_back(miter); len.push_back(m);
        } else {
            cur = perp(A);
            nrm.push_back(cur); len.push_back(1);
        }
    }
    if (total > 2 && closed) {
        A = direction(P[0], P[total - 2]);
        B = direction(P[1], P[0]);
        const double m = miter_of(A, B, miter);
        nrm[0] = miter; len[0] = m; nrm[total - 1] = miter; len[total - 1] = m;
        nrm.pop_back(); len.pop_back();
    }
    if (closed && n) { nrm.push_back(nrm[0]); len.push_back(len[0]); }
}

int32_t drawn_points(int32_t n, bool closed) { return n < 2 ? 0 : n + (closed ? 1 : 0); }

// One drawn point's record; `p` indexes the drawn path (closed: p == n is point 0 again).
FlPoint point_record(const float *pts, const double *times, int n, bool closed, int p, V2 nrm, double len)
{
    const int src = p == n ? 0 : p;
    const int prev = closed ? (p - 1 < 0 ? n + p - 1 : (p - 1) % n) : std::max(0, p - 1);
    const double time = times[src];
    FlPoint r;
    r.px = pts[2 * src]; r.py = pts[2 * src + 1];
    r.nx = (float)nrm.x; r.ny = (float)nrm.y;
    r.miter = (float)len;
    r.qx = pts[2 * prev]; r.qy = pts[2 * prev + 1];
    r.time = (float)time;
    r.dt = (float)(time - times[prev]);
    return r;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

namespace thi {
struct FlowLineScratch {
    DevBuf<char> dev;
    HostBuf<char> pinned;
    hipEvent_t uploaded = nullptr;             // the last copy out of `pinned`
    bool pending = false;
    std::vector<V2> nrm;
    std::vector<double> len;
};

void flow_lines_free(th_context *c)
{
    thi::FlowLineScratch *s = c->flow_lines;
    if (!s) return;
    if (s->uploaded) (void)hipEventDestroy(s->uploaded);
    delete s;
    c->flow_lines = nullptr;
}
}  // namespace thi

extern "C" {

th_status th_flow_line_attributes(const float *points, const double *times, int32_t n, int32_t closed, int32_t capacity,
                                  int32_t *nverts, float *position, float *normal, float *miter, float *previous,
                                  float *time, float *dt)
{
    TH_REQUIRE(n >= 0, "negative point count %d", n);
    TH_REQUIRE(nverts, "null vertex count");
    TH_REQUIRE(n == 0 || (points && times), "null points or times");
    const bool cl = closed != 0;
    const int32_t drawn = drawn_points(n, cl);
    *nverts = 2 * drawn;
    if (!drawn || capacity == 0) return TH_OK;                // (capacity 0: the count alone)
    TH_REQUIRE(capacity >= 2 * drawn, "capacity %d < %d vertices", capacity, 2 * drawn);
    TH_REQUIRE(position && normal && miter && previous && time && dt, "null attribute array");
    std::vector<V2> nrm;
    std::vector<double> len;
    line_normals(points, n, cl, nrm, len);
    for (int p = 0; p < drawn; ++p) {
        const FlPoint r = point_record(points, times, n, cl, p, nrm[p], len[p]);
        for (int s = 0; s < 2; ++s) {
            const int v = 2 * p + s;
            position[2 * v] = r.px; position[2 * v + 1] = r.py;
            normal[2 * v] = r.nx; normal[2 * v + 1] = r.ny;
            miter[v] = (float)(len[p] * (double)(s * 2 - 1));
            previous[2 * v] = r.qx; previous[2 * v + 1] = r.qy;
            time[v] = r.time;
            dt[v] = r.dt;
        }
    }
    return TH_OK;
}

th_status th_flow_lines(th_context *c, const th_flow_line_uniforms *u, const float *points, const double *times,
                        const int32_t *offsets, const int32_t *closed, int32_t nlines)
{
    if (th_status s = thi::use(c)) return s;
    TH_REQUIRE(u, "null uniforms");
    TH_REQUIRE(nlines >= 0, "negative line count %d", nlines);
    if (nlines == 0) return TH_OK;
    TH_REQUIRE(offsets && closed, "null offsets or closed flags");
    TH_REQUIRE(offsets[0] >= 0, "negative offset");
    for (int32_t i = 0; i < nlines; ++i) TH_REQUIRE(offsets[i + 1] >= offsets[i], "offsets decrease at line %d", i);
    TH_REQUIRE(offsets[nlines] == offsets[0] || (points && times), "null points or times");
    TH_REQUIRE(c->fw > 0 && c->fh > 0 && c->fw < 65536 * kTile && c->fh < 65536 * kTile, "no flow texture");

    // the strips: drawn points, triangles per line
    std::vector<int32_t> line_tri, line_pt;
    int64_t npts = 0, ntri = 0;
    for (int32_t i = 0; i < nlines; ++i) {
        const int32_t d = drawn_points(offsets[i + 1] - offsets[i], closed[i] != 0);
        if (!d) continue;
        line_tri.push_back((int32_t)ntri);
        line_pt.push_back((int32_t)npts);
        npts += d;
        ntri += 2 * (int64_t)d - 2;
    }
    TH_REQUIRE(ntri < (1 << 28), "%lld triangles: too many for one call", (long long)ntri);
    if (ntri == 0) return TH_OK;
    const int32_t nl = (int32_t)line_pt.size();
    line_tri.push_back((int32_t)ntri);

    thi::FlowLineScratch *s = c->flow_lines;
    if (!s) { s = new (std::nothrow) thi::FlowLineScratch; TH_REQUIRE(s, "out of host memory"); c->flow_lines = s; }

    // sizes: tiles, chunks (widened so that the (tile, chunk) counters stay bounded), the pair capacity (tile boxes bounded
    // from the attributes in double: |a| <= 1 when speedLimit > 0, else the whole view)
    const int tiles_x = (c->fw + kTile - 1) / kTile, tiles_y = (c->fh + kTile - 1) / kTile;
    const uint64_t ntiles = (uint64_t)tiles_x * tiles_y;
    uint32_t chunk = kChunkMin;
    while (ntiles * (((uint64_t)ntri + chunk - 1) / chunk) > kMaxCountCells && chunk < 4096u) chunk *= 2;
    const uint32_t nchunks = (uint32_t)(((uint64_t)ntri + chunk - 1) / chunk);
    TH_REQUIRE(ntiles * nchunks <= (uint64_t)kMaxCountCells * 4, "flow of %dx%d with %lld triangles: too large", c->fw, c->fh, (long long)ntri);

    const size_t rec_bytes = align256((size_t)npts * sizeof(FlPoint));
    const size_t tab_bytes = align256(sizeof(int32_t) * (size_t)(2 * nl + 1));
    const size_t up_bytes = rec_bytes + tab_bytes;
    if (s->pending) { TH_HIP(hipEventSynchronize(s->uploaded)); s->pending = false; }   // (the previous call's copy: long done)
    if (th_status st = s->pinned.reserve(up_bytes, up_bytes * 2)) return st;
    if (!s->uploaded) TH_HIP(hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming));

    FlPoint *rec = reinterpret_cast<FlPoint *>(s->pinned.get());
    const bool bounded = u->speedLimit > 0.0f;
    const double vx = (double)u->viewSize[0], vy = (double)u->viewSize[1], rad = std::fabs((double)u->rad);
    uint64_t pairs = 0;
    for (int32_t i = 0, li = 0; i < nlines; ++i) {
        const int32_t n = offsets[i + 1] - offsets[i];
        const bool cl = closed[i] != 0;
        const int32_t d = drawn_points(n, cl);
        if (!d) continue;
        const float *pts = points + 2 * (size_t)offsets[i];
        const double *tms = times + offsets[i];
        line_normals(pts, n, cl, s->nrm, s->len);
        FlPoint *r = rec + line_pt[li++];
        for (int p = 0; p < d; ++p) r[p] = point_record(pts, tms, n, cl, p, s->nrm[p], s->len[p]);
        for (int j = 0; j < 2 * d - 2; ++j) {              // tile box bound of triangle j: vertices j..j+2 (points j/2 .. (j+2)/2)
            double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
            bool ok = true;
            for (int k = j >> 1; k <= (j + 2) >> 1; ++k) {
                const double e = rad * std::fabs((double)r[k].miter);
                const double ex = std::fabs((double)r[k].nx) * e, ey = std::fabs((double)r[k].ny) * e;
                if (!std::isfinite(ex) || !std::isfinite(ey) || !std::isfinite((double)r[k].px) || !std::isfinite((double)r[k].py)) ok = false;
                const double xa = (r[k].px - ex) * vx, xb = (r[k].px + ex) * vx, ya = (r[k].py - ey) * vy, yb = (r[k].py + ey) * vy;
                x0 = std::min(x0, std::min(xa, xb)); x1 = std::max(x1, std::max(xa, xb));
                y0 = std::min(y0, std::min(ya, yb)); y1 = std::max(y1, std::max(ya, yb));
            }
            uint64_t here;
            if (!bounded) here = ntiles;
            else if (!ok) here = 0;                              // (a vertex that is not finite: the triangle is not drawn)
            else {
                auto tiles = [](double lo, double hi, int size, int ntile) -> uint64_t {
                    // texels [floor((lo+1)/2*size) - 1, ceil((hi+1)/2*size) + 1] clamped, in tiles
                    if (hi < -1.0 || lo > 1.0) return 0;
                    const double a = std::max(std::floor((std::max(lo, -1.0) + 1.0) * 0.5 * size) - 1.0, 0.0);
                    const double b = std::min(std::ceil((std::min(hi, 1.0) + 1.0) * 0.5 * size) + 1.0, (double)size - 1.0);
                    if (b < a) return 0;
                    return (uint64_t)std::min((double)ntile, std::floor(b / kTile) - std::floor(a / kTile) + 1.0);
                };
                here = tiles(x0, x1, c->fw, tiles_x) * tiles(y0, y1, c->fh, tiles_y);
            }
            pairs += here;
        }
    }
    TH_REQUIRE(pairs < (1ull << 31), "%llu tile entries: too many for one call", (unsigned long long)pairs);
    int32_t *tab = reinterpret_cast<int32_t *>(s->pinned + rec_bytes);
    std::copy(line_tri.begin(), line_tri.end(), tab);
    std::copy(line_pt.begin(), line_pt.end(), tab + nl + 1);

    // device scratch: records | table | triangles | boxes | counts | list
    const uint32_t ncount = (uint32_t)(ntiles * nchunks) + 1u;
    const size_t tri_bytes = align256((size_t)ntri * sizeof(FlTri)), box_bytes = align256((size_t)ntri * 8);
    const size_t cnt_bytes = align256((size_t)ncount * 4), sum_bytes = align256((size_t)th::exclusive_scan_sum_words(ncount) * 4);
    const size_t list_bytes = align256((size_t)std::max<uint64_t>(pairs, 1) * 4);
    const size_t need = up_bytes + tri_bytes + box_bytes + cnt_bytes + sum_bytes + list_bytes;
    if (s->dev.size() < need) {
        TH_HIP(hipStreamSynchronize(c->stream));              // (growing: the old scratch may still be in use)
        if (th_status st = s->dev.alloc(need + need / 2)) return st;
    }
    char *base = s->dev;
    TH_HIP(hipMemcpyAsync(base, s->pinned, up_bytes, hipMemcpyHostToDevice, c->stream));
    TH_HIP(hipEventRecord(s->uploaded, c->stream));
    s->pending = true;

    FlParams p{};
    p.pts = reinterpret_cast<const FlPoint *>(base);
    p.line_tri = reinterpret_cast<const int32_t *>(base + rec_bytes);
    p.line_pt = p.line_tri + nl + 1;
    p.nlines = nl; p.ntri = (int32_t)ntri;
    p.speed = u->speed; p.rad = u->rad; p.crest_shape = u->crestShape; p.speed_limit = u->speedLimit;
    p.view_x = u->viewSize[0]; p.view_y = u->viewSize[1];
    p.w = c->fw; p.h = c->fh; p.tiles_x = tiles_x; p.tiles_y = tiles_y;
    p.nchunks = nchunks; p.chunk = chunk;
    char *at = base + up_bytes;
    p.tris = reinterpret_cast<FlTri *>(at); at += tri_bytes;
    p.box = reinterpret_cast<uint32_t *>(at); at += box_bytes;
    p.counts = reinterpret_cast<uint32_t *>(at); at += cnt_bytes;
    uint32_t *sums = reinterpret_cast<uint32_t *>(at); at += sum_bytes;
    p.list = reinterpret_cast<uint32_t *>(at);
    p.list_cap = (uint32_t)std::max<uint64_t>(pairs, 1);
    p.flow = c->flow;

    TH_HIP(hipMemsetAsync(p.counts, 0, (size_t)ncount * 4, c->stream));
    hipLaunchKernelGGL(fl_setup_kernel, dim3((unsigned)((ntri + 255) / 256)), dim3(256), 0, c->stream, p);
    static const bool naive = [] { const char *e = getenv("TH_FLOWLINE_NAIVE"); return e && atoi(e) == 1; }();
    if (naive) {
        const uint32_t texels = (uint32_t)c->fw * (uint32_t)c->fh;
        hipLaunchKernelGGL(fl_naive_kernel, dim3(std::min<uint32_t>((texels + 255) / 256, 16384u)), dim3(256), 0, c->stream, p);
        TH_HIP(hipGetLastError());
        return TH_OK;
    }
    th::launch_exclusive_scan_u32(p.counts, sums, ncount, c->stream);
    hipLaunchKernelGGL(fl_fill_kernel, dim3(nchunks), dim3(256), (size_t)chunk * 12, c->stream, p);
    hipLaunchKernelGGL(fl_raster_kernel, dim3((unsigned)ntiles), dim3(256), 0, c->stream, p);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

}  // extern "C"
