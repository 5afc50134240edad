// th_draw.hip - Tendrils.draw() (src/index.js:278-337): the flow pass, the view pass, both in one call, the trail export;
// which pipeline draws (binned over sorted slots, th_bins.hip / stream-ordered in texel order, th_deposit.hip + th_sort.hip).
#include "th_ctx.hpp"
#include <chrono>

using namespace thi;

namespace thi {

// ---- flow deposit ------------------------------------------------------------------------------------------
int deposit_texel_bits(const th_context *c)
{
    const uint64_t texels = (uint64_t)c->fw * c->fh;
    int bits = 1;
    while (bits < 32 && (1ull << bits) < texels) ++bits;
    return bits;
}

// ---- which pipeline draws -------------------------------------------------------------------------------------
// The binned pipeline (th_bins.hip) walks the particles by slot, in whatever order the ring is held; the stream-ordered one
// (th_deposit.hip) needs texel order.  th_draw_pipeline (or TH_DRAW=bins / stream at th_create) forces one; by default the binned pipeline draws
// whenever the integrator would step over tile-sorted slots (sorting_possible): a step() + draw() frame loop then never
// leaves the sorted order.
// Which pipeline a draw pass takes.  auto: wherever the integrator steps over tile-sorted slots the frame loop - step(); draw() -
// stays on them: the binned pipeline takes particles in any order, and it is ahead of the stream-ordered one from the first
// frame (1.3 against 2.2 ms per draw with both passes at C3) to the crowded target the wake leaves after a thousand frames
// (70-77 % of all fragments in bins of more than 4096, in texels with thousands of them: 1.3-1.7 against 1.7-2.3 ms;
// profiles/r4_g_giants.txt).  (Round 3 handed a crowded target over to the stream-ordered pipeline for a spell: it was level
// then.)  A binned pass that cannot go on - no memory for its store - is repeated in stream order, and the ring then keeps
// texel order for opt.rebucket_steps steps (deposit_prepare): that many frames pass before the bins are tried again.

float drawn_line_width(const th_context *c, int pass)
{
    const float w = c->line_width[pass];
    return w < c->line_range[0] ? c->line_range[0] : (w > c->line_range[1] ? c->line_range[1] : w);
}

static int draw_policy(const th_context *c) { return c->draw_pipeline != TH_DRAW_AUTO ? c->draw_pipeline : c->opt.draw; }
// Both passes draw lines at most 2 wide.  (Wider lines cover more texels than a line's record holds: nearly all of them would
// leave the fused pass for the long list, one atomic per fragment - the stream-ordered pipeline counts and scans instead)
static bool lines_fit_records(const th_context *c) { return drawn_line_width(c, TH_PASS_FLOW) <= 2.0f && drawn_line_width(c, TH_PASS_VIEW) <= 2.0f; }

static bool draw_uses_bins(th_context *c)
{
    const int policy = draw_policy(c);
    if (policy == 0) return false;
    if (c->cfg.height != c->cfg.global_height || c->fw > th::kBinsMaxExtent || c->fh > th::kBinsMaxExtent) return false;
    if (policy == 1) return true;
    return lines_fit_records(c) && sorting_possible(c);
}

// How a prepared pass walks the lines: the stream-ordered pipeline in texel order; the bins by SLOT, in the order the ring is
// held in; or the bins in TEXEL order whatever that order is - the pass of a draw program, whose lines are the records its vertex
// stage left (texel-indexed) and read nothing of the ring.
enum class Walk { stream, slots, texels };
// per-line buffers + parameters
static th_status prepare_pass(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p, Walk walk);

// Draw programs and the auto policy: a program pass goes through the bins wherever the built-in pass of the same context would
// (and the gate in deposit_prepare holds) - the frame loop then keeps its sorted slots (DESIGN.md 3.10 has the measurement the
// default rests on).  false: only a forced policy (th_draw_pipeline / TH_DRAW = bins) sends a program pass there.
constexpr bool kAutoBinsPrograms = true;

// Does a sharded job draw through the bins?  Only what every rank sees alike may enter: the job's shapes, the lines' widths,
// the switches (set alike on all ranks) - not this band's size, not how crowded its last draw was.  (lines_local below
// IS rank-local - kept as it is here)
bool binned_shards(const th_context *c)
{
    const int policy = draw_policy(c);
    if (policy == 0 || (c->lines_local != 1 && c->lines_local != 0)) return false;      // (2: lookups off the line's own texel that no table holds)
    if (c->fw > th::kBinsMaxExtent || c->fh > th::kBinsMaxExtent) return false;
    if (!lines_fit_records(c)) return false;
    if (policy == 1 || c->opt.bucket == 1) return true;
    if (c->opt.bucket == 0) return false;
    // (sorting_possible's rule on the job's average band: the integrator steps over sorted slots there)
    const size_t flow_texels = (size_t)c->fw * c->fh, per_rank = (size_t)c->cfg.width * c->cfg.global_height / (size_t)std::max(c->comm_world, 1);
    return per_rank >= ((size_t)1 << 20) && per_rank >= 2 * flow_texels && flow_texels * sizeof(float2) > ((size_t)3 << 20);
}

// the binned pass over a band's slots in whatever order they are held (row-band shards: th_shard.hip)
th_status deposit_prepare_bins(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p)
{
    TH_REQUIRE(u, "null uniforms");
    TH_REQUIRE(c->ring.size() >= 2, "draw needs at least 2 state buffers (have %zu)", c->ring.size());
    if (any_sorted(c)) if (th_status s = align_slot_orders(c)) return s;
    c->last_binned_draw = c->total_steps;
    return prepare_pass(c, u, p, Walk::slots);
}

th_status deposit_prepare(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p, bool want_bins, bool *bins, bool program, const FragmentStage *stage)
{
    TH_REQUIRE(u, "null uniforms");
    TH_REQUIRE(c->ring.size() >= 2, "draw needs at least 2 state buffers (have %zu)", c->ring.size());
    if (program && !kAutoBinsPrograms && draw_policy(c) != 1) want_bins = false;
    // (a pass with a caller's fragment stage is stream-ordered, and no frame of the policy's count - unless TH_OPT_STAGE_BINS is on:
    // then it is the pass it would be without the stage, which runs over the bins' page store: deposit_run_bins.  A stage that
    // reads th_line stays stream-ordered under the option too - its line records lie beside the stream-ordered fragment array -
    // unless TH_OPT_LINE_BINS is on as well: then they lie beside the page store's places, bins_line_store)
    if (stage && (!c->opt.stage_bins || (stage_reads_line(stage) && !c->opt.line_bins))) want_bins = false;
    // The auto policy counts FRAMES, and the passes of one frame - th_flow_deposit then th_view_draw, or two widths - take one
    // pipeline: a view pass that left the slot order its flow pass had drawn over would throw the order away in mid-frame.
    if (want_bins && c->draw_frame_step != c->total_steps) { ++c->draws; c->draw_frame_step = c->total_steps; c->frame_bins = -1; }
    bool use_bins = want_bins && (c->frame_bins >= 0 && c->draw_pipeline == TH_DRAW_AUTO ? c->frame_bins == 1 : draw_uses_bins(c));
    if (use_bins) {
        // the binned pipeline reads a line's vertices from the line's own slot - or, for the shapes whose vertex lookup lands on
        // another particle, through the table of where those particles lie in the slot order (line_rows, th::LineSources); the
        // few shapes with more such rows / columns than the table holds keep to the stream-ordered pipeline in texel order
        if (th_status s = line_rows(c)) return s;
        // (a draw program's vertex stage over a slot order reads the slot's own f32 texels: shapes whose lookup drifts off the
        // line's texel, and packed rings - seen through an unpacked copy in texel order - keep to the stream-ordered path)
        if (program ? (c->lines_local != 1 || c->packed) : (c->lines_local != 1 && c->lines_local != 0)) use_bins = false;
        else if (any_sorted(c)) { if (th_status s = align_slot_orders(c)) return s; }
    }
    if (bins) *bins = use_bins;
    if (want_bins) c->frame_bins = use_bins ? 1 : 0;
    if (use_bins) c->last_binned_draw = c->total_steps;
    else {
        if (th_status s = ensure_identity(c)) return s;      // the vertex stream addresses particles in texel order
        c->hold_texel_order_until = c->total_steps + c->opt.rebucket_steps;   // a frame loop of step + draw stays in texel order
    }
    return prepare_pass(c, u, p, !use_bins ? Walk::stream : (program ? Walk::texels : Walk::slots));
}

// the five per-line buffers and the totals, all or nothing
static th_status line_buffers(th_context *c)
{
    const size_t lines = c->texels();
    if (c->dep_lines == lines) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    c->dep_lines = 0;                   // (all five per-line buffers and `lines`, or nothing: a failure below leaves the next call to start over)
    c->dep_count.reset(); c->dep_offset.reset(); c->dep_blocks.reset(); c->dep_record.reset(); c->dep_lists.reset();
    if (th_status s = c->dep_count.alloc(lines)) return s;
    if (th_status s = c->dep_offset.alloc(lines)) return s;
    if (th_status s = c->dep_record.alloc(2 * lines)) return s;
    if (th_status s = c->dep_lists.alloc(th::deposit_list_words((uint32_t)c->cfg.width, (uint32_t)c->cfg.height, &c->dep_list_cap))) return s;
    if (th_status s = c->dep_blocks.alloc(th::deposit_scan_words((uint32_t)c->cfg.width, (uint32_t)c->cfg.height))) return s;
    if (th_status s = c->dep_total.reserve(th::kTotWords, th::kTotWords)) return s;      // [0] total, [1] out-of-band flag, [2] largest bin, [3] large bins, [4] their blocks
    c->dep_lines = lines;
    return TH_OK;
}

// what every pass fills: the ring, the shapes, the uniforms, the per-line buffers
static void pass_fields(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p)
{
    p = th::DepositParams{};
    // a packed ring is read in place, texel by texel, as what the stored texels decode to (dep_state: no f32 copy of the ring
    // per draw - two passes over 10.7 GB at config 5's size)
    p.cur = c->ring[0]; p.prev = c->ring[1];
    p.packed = c->packed ? 1u : 0u;
    p.flow = c->flow;
    p.W = (uint32_t)c->cfg.width; p.H = (uint32_t)c->cfg.global_height;
    p.row0 = (uint32_t)c->cfg.row0; p.rows = (uint32_t)c->cfg.height;
    p.fw = c->fw; p.fh = c->fh;
    p.view_x = u->viewSize[0]; p.view_y = u->viewSize[1]; p.time = u->time; p.speed_limit = u->speedLimit;
    p.line_half = 0.5f * drawn_line_width(c, TH_PASS_FLOW);       // (view_params: the view pass's)
    {
        const int lw = c->cfg.width > 2 ? c->cfg.width : 2, lh = 2 * c->cfg.global_height > 2 ? 2 * c->cfg.global_height : 2;
        p.inv_x = 1.0 / (double)(lw - 1); p.inv_y = 1.0 / (double)(lh - 1);
    }
    p.count = c->dep_count; p.offset = c->dep_offset; p.record = c->dep_record; p.oob = c->dep_total + 1;
    p.list_n = c->dep_lists; p.list_cap = c->dep_list_cap;
    {
        uint32_t cap = 0;
        p.lists = c->dep_lists + (th::deposit_list_words((uint32_t)c->cfg.width, (uint32_t)c->cfg.height, &cap) - (size_t)3 * 64 * cap);      // (three kinds of list, 64 segments each: th_raster.hpp)
    }
    p.halo_lo = c->halo_lo; p.halo_hi = c->halo_hi;
}

// the bins' tables (grown when the target has more bins than ever before) and where they lie
static th_status bins_tables(th_context *c, th::DepositParams &p)
{
    p.bins_x = ((uint32_t)c->fw + (1u << th::kBinShift) - 1u) >> th::kBinShift;
    p.nbins = p.bins_x * (((uint32_t)c->fh + (1u << th::kBinShift) - 1u) >> th::kBinShift);
    if (c->bin_capacity < p.nbins) {
        TH_HIP(hipStreamSynchronize(c->stream));
        c->bin_capacity = 0; c->bin_mem.reset(); c->chunk_table.reset();
        const size_t stride = ((size_t)p.nbins + 255) / 256 * 256 + 64;      // (the lists' cursors of one bin on different memory channels)
        if (th_status s = c->bin_mem.alloc(th::kBinReplicas * stride + 2 * (size_t)p.nbins + 2)) return s;
        // (TH_OPT_BINS_PAGES: how far a list can grow at first - tests make it small to run the widening path)
        const int first = c->opt.bins_pages;
        c->bin_max_pages = first > 0 ? (uint32_t)first : (first < 0 ? (uint32_t)-first : th::kBinFirstPages);
        if (th_status s = c->chunk_table.alloc((size_t)p.nbins * th::kBinReplicas * c->bin_max_pages)) return s;
        TH_HIP(hipMemsetAsync(c->chunk_table, 0, c->chunk_table.bytes(), c->stream));        // (every reader of a list leaves its entries empty)
        c->bin_capacity = p.nbins;
    }
    p.bin_stride = (uint32_t)(((size_t)c->bin_capacity + 255) / 256 * 256 + 64);
    p.bin_cursor = c->bin_mem; p.large_bins = c->bin_mem + (size_t)th::kBinReplicas * p.bin_stride;
    p.large_key0 = p.large_bins + c->bin_capacity;
    p.page_table = c->chunk_table; p.max_pages = c->bin_max_pages;
    p.totals = c->dep_total; p.totals_host = nullptr; p.totals_seq = 0;       // (bins_expect, before the plan's kernels go out)
    return TH_OK;
}

// the blocks of 256 lines with something to draw into `list` (its count in front, read back into `n`): both caches below
static th_status list_blocks(th_context *c, const th::DepositParams &p, DevBuf<uint32_t> &list, uint32_t &n, uint32_t *src_slots)
{
    const size_t blocks = (c->texels() + 255) / 256;
    if (!c->draw_block_flags) if (th_status s = c->draw_block_flags.alloc(blocks)) return s;
    if (!list) if (th_status s = list.alloc(blocks + 1)) return s;          // (last: what goes with a list is there when the list is)
    th::launch_bins_block_list(p, c->draw_block_flags, list + 1, list, src_slots, c->stream);
    TH_HIP(hipGetLastError());
    return read_back(c, &n, list, sizeof(uint32_t));
}

// the walk of a binned pass: the slot order's perm, what the step saw of the lines, the block list - cached per slot order (one
// read-back per re-sort), or, by_texel, once per context
static th_status bins_walk(th_context *c, th::DepositParams &p, bool by_texel)
{
    // (by_texel: the walk is over texel indices - no perm, and nothing that describes the ring's slots below: what the step
    // saw of its lines is where the BUILT-IN stage puts them, not where a program does)
    const int o = by_texel ? -1 : order_of(c, c->ring[0]);
    p.perm = o >= 0 ? c->orders[(size_t)o].perm : nullptr;
    const unsigned long long stamp = o >= 0 ? c->orders[(size_t)o].stamp : 0ull;
    // what the step that wrote these two buffers saw of their lines (th_step.hip): only for exactly this pair, order and view
    // (... and only where a line's two ends ARE the slot's own particle, now and a step ago: lines_local)
    if (!by_texel && c->opt.skip_unseen && c->lines_local == 1 && c->seen.bytes && c->seen.cur == c->ring[0] && c->seen.prev == c->ring[1] && p.cur == c->ring[0] && p.prev == c->ring[1] &&
        c->seen.order == o && c->seen.stamp == stamp && c->seen.view_x == p.view_x && c->seen.view_y == p.view_y && c->seen.fw == c->fw && c->seen.fh == c->fh &&
        lines_fit_records(c))
        p.block_seen = reinterpret_cast<const uint32_t *>(c->seen.bytes.get());
    if (by_texel) {
        if (!c->texel_blocks_listed) {
            if (th_status s = list_blocks(c, p, c->texel_blocks, c->texel_nblocks, nullptr)) return s;
            c->texel_blocks_listed = true;
        }
        p.draw_blocks = c->texel_blocks + 1; p.draw_nblocks = c->texel_nblocks;
        return TH_OK;
    }
    if (!c->draw_blocks || c->draw_blocks_order != o || c->draw_blocks_stamp != stamp) {
        if (!c->draw_blocks && c->lines_local == 0)
            if (th_status s = c->src_slots.alloc((size_t)c->src_nrows * c->cfg.width + (size_t)c->src_ncols * c->cfg.height + 1)) return s;
        if (th_status s = list_blocks(c, p, c->draw_blocks, c->draw_nblocks, o >= 0 ? c->src_slots.get() : nullptr)) return s;
        c->draw_blocks_order = o; c->draw_blocks_stamp = stamp;
    }
    p.draw_blocks = c->draw_blocks + 1; p.draw_nblocks = c->draw_nblocks;
    if (c->lines_local == 0 && o >= 0) p.src.slot = c->src_slots;
    return TH_OK;
}

// per-line buffers + parameters of a pass whose pipeline is decided
static th_status prepare_pass(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p, Walk walk)
{
    TH_REQUIRE((size_t)c->fw * c->fh > 0 && (uint64_t)c->cfg.width * c->cfg.global_height < (1ull << 32), "bad shapes");
    if (th_status s = line_buffers(c)) return s;
    pass_fields(c, u, p);
    if (walk == Walk::stream) TH_HIP(hipMemsetAsync(c->dep_total, 0, th::kTotWords * sizeof(uint32_t), c->stream));      // (bins: launch_bins_fused)
    if (th_status s = line_rows(c)) return s;
    p.row_draws = c->d_row_draws;
    if (c->lines_local == 0) {          // (the tables; `slot` stays null in texel order: a texel's slot is its index)
        p.src.row_index = c->src_row_index; p.src.col_index = c->src_col_index; p.src.nrows = c->src_nrows; p.src.ncols = c->src_ncols;
    }
    if (walk == Walk::stream) return TH_OK;
    if (th_status s = bins_tables(c, p)) return s;
    return bins_walk(c, p, walk == Walk::texels);
}

th_status missing_halo(const th_context *c)
{
    return fail(TH_ERR_UNSUPPORTED, "a line of this row band looks up a particle row outside the band (rows %d..%d of %d) and no halo row was supplied (th_deposit_set_halo)", c->cfg.row0, c->cfg.row0 + c->cfg.height, c->cfg.global_height);
}

// scan of p.count (filled by the caller's marking pass) -> p.offset, total (one sync); reports band violations
th_status deposit_scan_total(th_context *c, const th::DepositParams &p, uint32_t *total)
{
    th::launch_deposit_scan(p, c->dep_blocks, c->dep_total, c->stream);
    uint32_t host[2] = {0, 0};
    if (th_status s = read_back(c, host, c->dep_total, sizeof host)) return s;
    if (host[1]) return missing_halo(c);
    if (host[0] >= (1u << 31)) return fail(TH_ERR_UNSUPPORTED, "too many fragments for one draw (2^31 or more)");
    *total = host[0];
    return TH_OK;
}

// per-fragment buffers for `total` fragments (grow-only)
th_status deposit_reserve(th_context *c, uint32_t total, bool wide, bool pairs, bool lines)
{
    if (pairs && !c->dep_pairs) {                 // two varyings per fragment: the colour buffers at twice the size
        c->dep_colors.reset(); c->dep_colors_sorted.reset();
        c->dep_pairs = true;
        if (c->dep_capacity) if (th_status s = c->dep_colors.alloc(2 * c->dep_capacity)) { c->dep_capacity = 0; return s; }
    }
    if (c->dep_capacity < total) {
        for (DevBuf<uint32_t> &q : c->dep_u32) q.reset();
        for (DevBuf<unsigned long long> &q : c->dep_u64) q.reset();
        c->dep_colors.reset(); c->dep_colors_sorted.reset(); c->dep_fraglines.reset();
        c->dep_capacity = 0; c->dep_wide = false;
        const size_t cap = (size_t)total + (size_t)total / 4 + 1024;
        for (DevBuf<uint32_t> &q : c->dep_u32) if (th_status s = q.alloc(cap)) return s;
        if (th_status s = c->dep_colors.alloc((c->dep_pairs ? 2 : 1) * cap)) return s;
        c->dep_capacity = cap;
    }
    if (!c->dep_colors_sorted) if (th_status s = c->dep_colors_sorted.alloc((c->dep_pairs ? 2 : 1) * c->dep_capacity)) return s;
    if (wide && !c->dep_wide) {
        for (DevBuf<unsigned long long> &q : c->dep_u64) if (th_status s = q.alloc(c->dep_capacity)) return s;
        c->dep_wide = true;
    }
    if (lines && !c->dep_fraglines) if (th_status s = c->dep_fraglines.alloc(c->dep_capacity)) return s;      // (a stage that reads th_line: fragment_stage_run)
    return TH_OK;
}

th_status deposit_temp(th_context *c, size_t need) { return c->dep_temp.reserve(need, need + need / 4); }

// ---- view pass ---------------------------------------------------------------------------------------------
// The screen image and Tendrils.buffers at the target's shape (Tendrils.resize gives every buffer viewRes, src/index.js:404:
// a resized FBO starts empty); c->view = the bound one.
th_status view_storage(th_context *c)
{
    const bool shaped = c->view_w == c->fw && c->view_h == c->fh;
    if (c->view && shaped && (int32_t)c->view_ring.size() == c->view_buffers) return TH_OK;
    const size_t bytes = (size_t)c->fw * c->fh * sizeof(uchar4);
    auto fresh = [&](uchar4 **img) -> th_status {            // (a view_ring element: raw, like the particle ring's)
        TH_HIP(hipMalloc((void **)img, bytes));
        TH_HIP(hipMemsetAsync(*img, 0, bytes, c->stream));       // a fresh drawing buffer is transparent black
        return TH_OK;
    };
    const uchar4 *was = c->view;
    int32_t bound = was && was != c->view_screen ? -2 : -1;      // (-2: a buffer that may be gone in a moment)
    for (size_t k = 0; k < c->view_ring.size(); ++k) if (c->view_ring[k] == was) bound = (int32_t)k;
    TH_HIP(hipStreamSynchronize(c->stream));
    c->view = nullptr;
    if (!shaped) {
        c->view_screen.reset();
        for (uchar4 *&b : c->view_ring) { (void)hipFree(b); b = nullptr; }
        c->view_w = c->view_h = 0;
    }
    while ((int32_t)c->view_ring.size() > c->view_buffers) { (void)hipFree(c->view_ring.back()); c->view_ring.pop_back(); }
    while ((int32_t)c->view_ring.size() < c->view_buffers) c->view_ring.push_back(nullptr);
    if (!c->view_screen) {
        if (th_status s = c->view_screen.alloc((size_t)c->fw * c->fh)) return s;
        TH_HIP(hipMemsetAsync(c->view_screen, 0, bytes, c->stream));
    }
    for (uchar4 *&b : c->view_ring) if (!b) if (th_status s = fresh(&b)) return s;
    c->view_w = c->fw; c->view_h = c->fh;
    c->view = bound >= 0 && bound < (int32_t)c->view_ring.size() ? c->view_ring[(size_t)bound] : c->view_screen;   // (a bound buffer that was removed: the screen)
    return TH_OK;
}

void view_fields(th_context *c, const th_render_uniforms *u, th::DepositParams &p)
{
    p.flow_decay = u->flowDecay; p.speed_alpha = u->speedAlpha; p.colormap_alpha = u->colorMapAlpha; p.sin_term = u->sinTerm;
    for (int k = 0; k < 4; ++k) { p.base_color[k] = u->baseColor[k]; p.flow_color[k] = u->flowColor[k]; }
    p.colormap = c->colormap; p.cw = c->cmap_w; p.ch = c->cmap_h;
}

// what the vertex stage takes of a view pass's uniforms
th_deposit_uniforms deposit_uniforms_of(const th_render_uniforms &u)
{
    th_deposit_uniforms d{};
    d.viewSize[0] = u.viewSize[0]; d.viewSize[1] = u.viewSize[1]; d.time = u.time; d.speedLimit = u.speedLimit;
    return d;
}

th_status view_params(th_context *c, const th_render_uniforms *u, th::DepositParams &p, bool want_bins, bool *bins, const FragmentStage *stage)
{
    TH_REQUIRE(u, "null uniforms");
    const th_deposit_uniforms d = deposit_uniforms_of(*u);
    if (th_status s = deposit_prepare(c, &d, p, want_bins, bins, false, stage)) return s;
    p.mode = 1;
    p.line_half = 0.5f * drawn_line_width(c, TH_PASS_VIEW);
    view_fields(c, u, p);
    return TH_OK;
}

// ---- what the entry points of a draw say alike --------------------------------------------------------------------------------
void draw_moves_nothing(th_context *c) { c->last_draw.sent_bytes = c->last_draw.received_bytes = 0; }

// a local entry point on a row band: `what` it is and where a band's pass goes `instead`, in the entry point's own words
th_status refuse_band(const th_context *c, const char *what, const char *instead)
{
    if (c->cfg.height == c->cfg.global_height) return TH_OK;
    return fail(TH_ERR_UNSUPPORTED, "%s on a row-band shard (%d of %d rows): %s", what, c->cfg.height, c->cfg.global_height, instead);
}

th_status shared_uniforms(const th_deposit_uniforms *du, const th_render_uniforms *ru)
{
    TH_REQUIRE(memcmp(du->viewSize, ru->viewSize, sizeof du->viewSize) == 0 && memcmp(&du->time, &ru->time, sizeof du->time) == 0 &&
               memcmp(&du->speedLimit, &ru->speedLimit, sizeof du->speedLimit) == 0,
               "the two passes of one draw share viewSize, time and speedLimit");
    return TH_OK;
}

}  // namespace thi

static th_status export_run(th_context *c, th::DepositParams &p, float *lines, uint64_t capacity, uint64_t *count)
{
    th::launch_export_mark(p, c->stream);
    uint32_t total = 0;
    if (th_status s = deposit_scan_total(c, p, &total)) return s;
    *count = total;
    if (!lines || total == 0) return TH_OK;                  // size query
    TH_REQUIRE(capacity >= total, "line buffer holds %llu of %u lines", (unsigned long long)capacity, total);
    DevBuf<float> d_out;                     // (every way out frees it; the one that launched waits for the stream first)
    if (th_status s = d_out.alloc((size_t)total * 12)) return s;
    th::launch_export_write(p, d_out, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(lines, d_out, (size_t)total * 12 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    (void)hipStreamSynchronize(c->stream);
    TH_HIP(e);
    return TH_OK;
}

// the fragments of the (prepared) pass `p`: count, emit, sort by texel, blend
th_status thi::deposit_run(th_context *c, th::DepositParams &p, const FragmentStage *stage, uint64_t *fragments)
{
    // Same state, same view, same resolution as the pass before (the view pass after the flow pass of one draw()): the
    // lines cover the same texels in the same order - counts, offsets, records and the sorted order of the fragments are
    // still there, only the varyings differ.  (TH_DRAW_REUSE=0: every pass on its own.)
    // (A caller's fragment stage runs over the array the scatter writes, key beside varying: such a pass reuses nothing.)
    const bool reuse = c->opt.draw_reuse && !stage && p.mode != 2 && c->drawn.valid && !c->drawn.binned && c->drawn.view_x == p.view_x && c->drawn.view_y == p.view_y &&
                       c->drawn.line_half == p.line_half;
    uint32_t total = 0;
    if (reuse) total = c->drawn.total;
    else {
        c->drawn.valid = false;
        th::launch_deposit_count(p, c->stream);
        if (th_status s = deposit_scan_total(c, p, &total)) return s;
    }
    if (fragments) *fragments = total;
    draw_streamed(c, total);
    if (total == 0) return TH_OK;
    if (!reuse) if (th_status s = deposit_reserve(c, total, false, p.mode == 2, stage_reads_line(stage))) return s;
    p.keys = c->dep_u32[0]; p.slots = c->dep_u32[1]; p.keys_sorted = c->dep_u32[2]; p.slots_sorted = c->dep_u32[3];
    p.colors = c->dep_colors; p.colors_sorted = c->dep_colors_sorted;
    if (reuse) {
        p.keys = nullptr;                        // (the keys are where the sort left them: only the varyings are written)
        if (c->drawn.sorted_in_a) { p.keys_sorted = c->dep_u32[0]; p.slots_sorted = c->dep_u32[1]; }
        th::launch_deposit_scatter(p, c->stream);
    } else {
        const int bits = th::deposit_key_bits(p);
        if (th_status s = deposit_temp(c, th::radix_sort_temp_bytes(total, 0, bits))) return s;
        th::launch_deposit_scatter(p, c->stream);
        if (stage) if (th_status s = fragment_stage_run(c, *stage, p, total)) return s;
        const bool in_a = th::launch_radix_sort_u32(p.keys, p.slots, p.keys_sorted, p.slots_sorted, total, 0, bits, c->dep_temp, true, c->stream) == 0;
        if (in_a) { p.keys_sorted = c->dep_u32[0]; p.slots_sorted = c->dep_u32[1]; }        // an even number of passes ends in the (a) buffers
        c->drawn.valid = true; c->drawn.binned = false; c->drawn.view_x = p.view_x; c->drawn.view_y = p.view_y; c->drawn.line_half = p.line_half; c->drawn.total = total; c->drawn.sorted_in_a = in_a;
    }
    th::launch_deposit_blend(p, total, c->stream);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

// the chunk store of the binned pipeline: nbins + pool chunks of keys (all empty) and varyings
// The varyings are sized by the pass that needs them (one float4 per place; two once a th_draw has run) and the pool starts
// at a quarter of the bins' first pages: the growth path is there (deposit_run_bins repeats a pass whose pool ran dry), and
// at 1920 x 1080 the store is 0.9 GB for a flow-only host, 1.4 GB with both passes - not 2.7 GB up front.  A store that
// cannot be allocated (a small device, many contexts) leaves the draw to the stream-ordered pipeline.
static size_t bins_places(uint32_t bins, uint32_t pool) { return ((size_t)bins * th::kBinReplicas + pool) * th::kBinPage; }

// the store as every blend leaves it: keys to "empty", the lists' page tables to "no page"
static th_status bins_wipe(th_context *c)
{
    if (c->bins_keys) TH_HIP(hipMemsetAsync(c->bins_keys, 0xff, bins_places(c->bins_store_bins, c->bins_pool) * sizeof(unsigned long long), c->stream));
    if (c->chunk_table) TH_HIP(hipMemsetAsync(c->chunk_table, 0, (size_t)c->bin_capacity * th::kBinReplicas * c->bin_max_pages * sizeof(uint32_t), c->stream));
    return TH_OK;
}

static th_status bins_store(th_context *c, uint32_t nbins, uint32_t pool, bool pairs)
{
    if (c->bins_keys && c->bins_store_bins == nbins && c->bins_pool >= pool && (c->bins_pairs || !pairs)) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    c->bins_keys.reset(); c->bins_colors.reset();
    c->bins_lines.reset(); c->bins_lines_places = 0;         // (the places' line records follow the store: bins_line_store)
    pool = pool > c->bins_pool ? pool : c->bins_pool;
    pairs = pairs || c->bins_pairs;
    c->bins_pool = 0; c->bins_store_bins = 0;
    const size_t places = bins_places(nbins, pool);
    TH_REQUIRE(places < ((size_t)1 << 32), "the binned draw's chunk store would hold 2^32 places or more");
    const std::string said = last_error();          // (a store that cannot be had is no error: th_last_error() keeps what it said)
    if (c->bins_colors.alloc(places * (pairs ? 2 : 1)) != TH_OK || c->bins_keys.alloc(places) != TH_OK) {      // (the keys last: the store is there when they are)
        (void)hipGetLastError();
        last_error() = said;
        c->bins_colors.reset();
        return kRetryInStreamOrder;
    }
    TH_HIP(hipMemsetAsync(c->bins_keys, 0xff, places * sizeof(unsigned long long), c->stream));
    c->bins_pool = pool; c->bins_store_bins = nbins; c->bins_pairs = pairs;
    return TH_OK;
}

// What a binned pass whose fragment stage reads th_line holds beside the store (TH_OPT_LINE_BINS; th_fragline.hip): the lines'
// snapped endpoints by stream index - 16 bytes a particle, 268 MB at 4096^2 - and a line record per place of the store - 16
// bytes a place, the size of bins_colors with one varying a place -, reserved by the first pass that needs them;
// the records are as long as the store and go when it is laid out anew (bins_store).  Memory that cannot be had is no error: the
// pass goes stream-ordered, as for a store that cannot be had, and th_last_error() keeps what it said.
static th_status bins_line_store(th_context *c)
{
    const size_t places = bins_places(c->bins_store_bins, c->bins_pool);
    if (c->bins_line_ends && c->bins_lines && c->bins_lines_places >= places) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    const std::string said = last_error();
    c->bins_lines.reset(); c->bins_lines_places = 0;
    if ((!c->bins_line_ends && c->bins_line_ends.alloc((size_t)c->cfg.width * c->cfg.global_height) != TH_OK) || c->bins_lines.alloc(places) != TH_OK) {
        (void)hipGetLastError();
        last_error() = said;
        c->bins_line_ends.reset(); c->bins_lines.reset();
        return kRetryInStreamOrder;
    }
    c->bins_lines_places = places;
    return TH_OK;
}

constexpr double kEarlyBlendShare = 0.5;            // (of a draw's fragments in crowded bins: see deposit_run_bins)
// ---- the binned pipeline (th_bins.hip) over the (prepared) pass `p`, in three parts ------------------------------------------
namespace thi {

th_status bins_streams(th_context *c)
{
    if (c->side) return TH_OK;
    TH_HIP(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    TH_HIP(hipEventCreateWithFlags(&c->forked, hipEventDisableTiming));
    TH_HIP(hipEventCreateWithFlags(&c->joined, hipEventDisableTiming));
    TH_HIP(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
    TH_HIP(hipEventCreateWithFlags(&c->joined2, hipEventDisableTiming));
    TH_HIP(hipEventCreateWithFlags(&c->regrouped, hipEventDisableTiming));
    if (th_status s = c->bins_totals_host.alloc(th::kTotWords + 1, hipHostMallocCoherent | hipHostMallocMapped)) return s;
    memset(c->bins_totals_host, 0, (th::kTotWords + 1) * sizeof(uint32_t));
    TH_HIP(hipHostGetDevicePointer((void **)&c->bins_totals_dev, c->bins_totals_host, 0));
    return TH_OK;
}

// the pass's totals to the host over the side stream (behind `forked`, recorded by the caller on the main stream)
// crowd_plan_kernel, the last kernel of a pass's plan, has been launched with p.totals_host / p.totals_seq (bins_expect): wait
// for the sequence number to arrive behind the totals.  (Polled: the device writes host memory; a copy on the side stream had
// to be scheduled behind an event, run and be signalled before the host woke up - 43 us in which nothing ran.)
static void bins_expect(th_context *c, th::DepositParams &p)
{
    p.totals_host = c->bins_totals_dev; p.totals_seq = ++c->totals_seq;
    if (p.totals_seq == 0u) p.totals_seq = ++c->totals_seq;          // (0: what the word holds before the first pass)
}
static th_status bins_totals(th_context *c, const th::DepositParams &p)
{
    volatile uint32_t *seq = c->bins_totals_host + th::kTotWords;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; __atomic_load_n(seq, __ATOMIC_ACQUIRE) != p.totals_seq; ++spins) {
        if ((spins & 1023u) == 1023u) {
            // a kernel that faulted never writes the word: ask the runtime now and then, give up after a long while
            const hipError_t e = hipStreamQuery(c->stream);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(TH_ERR_HIP, "the binned pass failed: %s", hipGetErrorString(e));
            if (e == hipSuccess && __atomic_load_n(seq, __ATOMIC_ACQUIRE) != p.totals_seq) {
                // (the stream is done and the word is not there: read the totals the slow way)
                TH_HIP(hipMemcpy(c->bins_totals_host, c->dep_total, th::kTotWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
                return TH_OK;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) return fail(TH_ERR_HIP, "the binned pass's totals did not arrive");
        }
    }
    return TH_OK;
}

th_status bins_store_for(th_context *c, th::DepositParams &p, uint32_t at_least)
{
    // (TH_OPT_BINS_POOL: the first pool's size in pages - tests make it small to run the growth path)
    const uint32_t pool0 = c->opt.bins_pool;
    uint32_t pool = c->bins_pool ? c->bins_pool : (pool0 ? pool0 : (p.nbins * 4u > 4096u ? p.nbins * 4u : 4096u));
    if (pool < at_least) pool = at_least;
    if (th_status s = bins_store(c, p.nbins, pool, p.mode == 2)) return s;
    p.frag_keys = c->bins_keys; p.colors = c->bins_colors; p.pool_pages = c->bins_pool;
    return TH_OK;
}

// every list's page table four times as wide (`keep`: with its entries - row-band shards: the owner's own bins are laid out
// already; otherwise the table is empty, as every pass leaves it)
th_status bins_table_widen(th_context *c, th::DepositParams &p, bool keep)
{
    const uint32_t had = c->bin_max_pages, wide = had * 4u < th::kBinPagesLimit ? had * 4u : th::kBinPagesLimit;
    if (c->opt.bins_pages < 0 || wide <= had) return kRetryInStreamOrder;
    const size_t lists = (size_t)c->bin_capacity * th::kBinReplicas;
    DevBuf<uint32_t> table;
    const std::string said = last_error();          // (no memory for it is no error: th_last_error() keeps what it said)
    if (table.alloc(lists * wide) != TH_OK) { (void)hipGetLastError(); last_error() = said; return kRetryInStreamOrder; }
    TH_HIP(hipMemsetAsync(table, 0, table.bytes(), c->stream));
    if (keep) TH_HIP(hipMemcpy2DAsync(table, (size_t)wide * sizeof(uint32_t), c->chunk_table, (size_t)had * sizeof(uint32_t), (size_t)had * sizeof(uint32_t), lists, hipMemcpyDeviceToDevice, c->stream));
    TH_HIP(hipStreamSynchronize(c->stream));
    c->chunk_table.swap(table); c->bin_max_pages = wide;          // (the narrow one goes with `table`)
    p.page_table = c->chunk_table; p.max_pages = wide;
    return TH_OK;
}

// a larger pool behind the same bins WITH what the store holds (row-band shards: the owner's own bins wait in it for the
// other ranks' fragments); page ids stay what they are
th_status bins_store_grow_keep(th_context *c, th::DepositParams &p, uint32_t pool)
{
    if (pool <= c->bins_pool) return TH_OK;
    const size_t had = bins_places(c->bins_store_bins, c->bins_pool), places = bins_places(c->bins_store_bins, pool), per = c->bins_pairs ? 2 : 1;
    TH_REQUIRE(places < ((size_t)1 << 32), "the binned draw's chunk store would hold 2^32 places or more");
    DevBuf<unsigned long long> keys;
    DevBuf<float4> colors;
    if (th_status s = keys.alloc(places)) return s;
    if (colors.alloc(places * per) != TH_OK) { (void)hipGetLastError(); return fail(TH_ERR_HIP, "the binned store could not grow to %zu places", places); }
    TH_HIP(hipMemcpyAsync(keys, c->bins_keys, had * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    TH_HIP(hipMemcpyAsync(colors, c->bins_colors, had * per * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    TH_HIP(hipStreamSynchronize(c->stream));
    c->bins_keys.swap(keys); c->bins_colors.swap(colors); c->bins_pool = pool;      // (the smaller ones go with the locals)
    p.frag_keys = c->bins_keys; p.colors = c->bins_colors; p.pool_pages = pool;
    return TH_OK;
}

// Part 1: rasterise + emit into the bins, the plan; repeated with a larger pool when the pool ran dry (nothing has been
// blended).  blend_early: the ordinary bins' blend goes out right behind the pass and covers the totals' read-back.
// Leaves the totals in c->bins_totals_host.  kRetryInStreamOrder: a bin outgrew its lists (or the store cannot be had).
th_status bins_pass_emit(th_context *c, th::DepositParams &p, bool blend_early, bool program, const FragmentStage *stage)
{
    c->drawn.valid = false;
    if (th_status s = bins_streams(c)) return s;
    uint32_t *host = c->bins_totals_host;
    // A pass that emitted and was never blended (th_shard.hip: a peer gave up or failed after this rank's own emit had
    // succeeded) left keys in its places and page ids in its lists' tables: a page id found there before this pass publishes
    // its own would send fragments to pages another list owns now, and stale keys would blend as fragments nobody drew.
    if (c->bins_dirty) {
        if (th_status s = bins_wipe(c)) return s;
        c->bins_dirty = false;
    }
    for (int attempt = 0;; ++attempt) {
        if (th_status s = bins_store_for(c, p, 0)) return s;
        // (a stage that reads th_line: room for this attempt's store's line records before anything is emitted - a pass that
        // cannot have it has touched nothing)
        if (stage_reads_line(stage)) if (th_status s = bins_line_store(c)) return s;
        bins_expect(c, p);
        th::launch_bins_fused(p, c->stream, program);
        // A caller's fragment stage: over every place the attempt handed out, in place, before the fork - so before the early blend
        // and both topologies of bins_pass_blend: every fragment has run before anything blends (th_flow inside a stage reads the
        // field as it was before the pass).  On an attempt the host then turns down it is harmless: the kernel leaves a flagged
        // pass alone, a repeated pass writes every varying again and an abandoned one is wiped.
        // (one that reads th_line: the two line kernels first, on this stream, then its sixth entry point - fragment_stage_run_bins)
        if (stage) if (th_status s = fragment_stage_run_bins(c, *stage, p, !blend_early, program)) return s;
        // the totals come back over the side stream while the ordinary bins are already being blended (the kernel looks at the
        // pass's flags itself): the host's round trip - it sizes the crowded bins' launches - costs the GPU nothing
        TH_HIP(hipEventRecord(c->forked, c->stream));
        if (blend_early) th::launch_bins_blend(p, c->stream);
        if (th_status s = bins_totals(c, p)) return s;
        const uint32_t flags = host[th::kTotFlags];
        if (host[th::kTotOob]) {          // (a store nobody will blend: wiped by the next pass)
            c->bins_dirty = true;
            return missing_halo(c);
        }
        if (flags == 0) { c->bins_dirty = true; return TH_OK; }        // (until bins_pass_finish has sent the blends after it)
        // nothing has been blended yet: the store is wiped, and the pass is repeated with a larger pool - or, when a bin
        // outgrew its chunk table or a line its reservation, left to the stream-ordered pipeline
        if (th_status s = bins_wipe(c)) return s;
        if (bins_flags_final(flags, attempt)) return kRetryInStreamOrder;
        // (a bin that outgrew its lists - the wake of a long-running loop draws half a million fragments into 16 x 16 texels -
        // gets a wider page table: a list's pages x 4, up to kBinPagesLimit)
        if (flags & th::kBinsBinFull) { if (th_status s = bins_table_widen(c, p, false)) return s; }
        if (flags & th::kBinsPoolExhausted) {
            const uint32_t want = 2u * host[th::kTotPool] + 64;      // (generously: growing the store costs a frame's worth of time)
            if (th_status s = bins_store(c, p.nbins, want, p.mode == 2)) return s;
        }
    }
}

// Part 2: with the totals in c->bins_totals_host.  First, room for the crowded bins: `nlarge` of them holding `crowd_keys` of the
// pass's `total` fragments (both buffers grow-only), and where their arrays lie.
static th_status crowd_room(th_context *c, th::DepositParams &p, uint32_t nlarge, uint32_t crowd_keys, uint32_t total)
{
    if (c->crowd_capacity < nlarge) {
        c->crowd_capacity = 0;
        const uint32_t cap = std::min(p.nbins, std::max(2u * nlarge + 256u, p.nbins / 4u));      // (a quarter of the bins at once: no growth step by step)
        if (th_status s = c->crowd_mem.alloc((size_t)cap * th::crowd_words_per_bin())) return s;
        // (the fragment counts per texel - the first of the arrays - start from zero; crowd_scan_kernel leaves them so)
        TH_HIP(hipMemsetAsync(c->crowd_mem, 0, th::crowd_count_words(cap) * sizeof(uint32_t), c->stream));
        TH_HIP(hipStreamSynchronize(c->stream));         // (whichever stream the regroup runs on: a new buffer is rare)
        c->crowd_capacity = cap;
    }
    if (c->crowd_keys_cap < crowd_keys) {
        c->crowd_keys.reset(); c->crowd_sorted.reset(); c->crowd_parted.reset(); c->crowd_windows.reset(); c->crowd_keys_cap = 0;
        // (room for every fragment of a pass like this one and a quarter more: the share of the crowded bins grows from a third
        // to three quarters over the first hundred frames of a loop - sized by what it is now, the four buffers were freed and
        // allocated again every few frames on the way, milliseconds each time)
        const size_t cap = std::max(2 * (size_t)crowd_keys, (size_t)total + total / 4) + ((size_t)1 << 20);
        if (th_status s = c->crowd_keys.alloc(cap)) return s;
        if (th_status s = c->crowd_sorted.alloc(cap)) return s;
        if (th_status s = c->crowd_parted.alloc(cap)) return s;
        if (th_status s = c->crowd_windows.alloc((cap / 512 + 2) * 3)) return s;      // (th_bins.hip: giant_part_kernel)
        c->crowd_keys_cap = cap;
    }
    p.nlarge = nlarge;
    th::crowd_carve(p, c->crowd_mem, c->crowd_capacity);
    p.crowd_keys = c->crowd_keys; p.crowd_sorted = c->crowd_sorted; p.crowd_parted = c->crowd_parted;
    p.crowd_windows = c->crowd_windows; p.crowd_windows_cap = (uint32_t)(c->crowd_keys_cap / 512 + 2);
    return TH_OK;
}

// ... then the launches: the crowded bins regrouped and blended on the side streams, the ordinary bins' blend unless it went
// out early.  The two topologies are written out in full: they are what was measured.
static th_status bins_pass_blend(th_context *c, th::DepositParams &p, bool blended_early)
{
    const uint32_t nlarge = p.nlarge;
    if (nlarge && !blended_early) {
        // A crowded target: the crowded bins' short runs - regroup, sort, walk: the longest chain of the draw - stay on the MAIN
        // stream, right behind the plan (no event to wait for) and right in front of whatever the host sends next (a frame
        // loop's next step: behind a chain that ends on a side stream it waited 17-26 us for the join); beside them, on the
        // side streams, the ordinary bins' blend (disjoint texels, kernels that wait on chains and loads rather than fill the
        // chip) and the long runs - the walk of the longest run, one fragment after the other, overlaps with everything else.
        th::launch_bins_regroup(p, c->stream);
        th::launch_bins_part_giants(p, c->stream);          // (the long runs' stream is the longer one: its first kernel here)
        TH_HIP(hipEventRecord(c->regrouped, c->stream));
        TH_HIP(hipStreamWaitEvent(c->side2, c->forked, 0));       // (recorded behind the emitting pass and its plan)
        th::launch_bins_blend(p, c->side2);
        TH_HIP(hipEventRecord(c->joined2, c->side2));
        TH_HIP(hipStreamWaitEvent(c->side, c->regrouped, 0));
        th::launch_bins_blend_giants(p, c->side);
        th::launch_bins_sort_long(p, c->side);
        th::launch_bins_walk_long(p, c->side);
        TH_HIP(hipEventRecord(c->joined, c->side));
        th::launch_bins_blend_crowd(p, c->stream);
        // (both side streams waited for by the main stream: a wait costs it ~9 us even when the event has long been signalled, but
        // with the crowded bins' sort at 140 us the ordinary bins' blend ends LAST as often as not - the long runs' last kernel
        // waiting for it, so that the main stream had one event to wait for, stood idle in half of the frames)
        TH_HIP(hipStreamWaitEvent(c->stream, c->joined, 0)); TH_HIP(hipStreamWaitEvent(c->stream, c->joined2, 0));
    } else if (nlarge) {
        // The ordinary bins' blend went out early on the main stream (few fragments in crowded bins last time): the crowded
        // bins on two streams of their own beside it - their fragments regrouped by texel, then the long runs on one stream
        // and the short runs on the other.
        TH_HIP(hipStreamWaitEvent(c->side2, c->forked, 0));       // (recorded behind the emitting pass and its plan: the ordinary bins' blend need not be waited for)
        th::launch_bins_regroup(p, c->side2);
        th::launch_bins_part_giants(p, c->side2);
        TH_HIP(hipEventRecord(c->regrouped, c->side2));
        TH_HIP(hipStreamWaitEvent(c->side, c->regrouped, 0));
        th::launch_bins_blend_giants(p, c->side);
        // ... and the runs in between behind them.  (A stream of their own shares a hardware queue with one of the others -
        // four per process by default - and holds that one's kernels back; behind the ordinary bins' blend on the main stream,
        // or ordered behind the short runs and walked on the main stream: the same within 1-3 % one way or the other, by the
        // phase of the loop - the blend phase of a crowded draw is bound by the chip's throughput, not by one stream's chain:
        // profiles/r4_g_giants.txt)
        th::launch_bins_sort_long(p, c->side);
        th::launch_bins_walk_long(p, c->side);
        TH_HIP(hipEventRecord(c->joined, c->side));
        th::launch_bins_blend_crowd(p, c->side2);
        TH_HIP(hipEventRecord(c->joined2, c->side2));
        TH_HIP(hipStreamWaitEvent(c->stream, c->joined, 0)); TH_HIP(hipStreamWaitEvent(c->stream, c->joined2, 0));
    } else if (!blended_early) th::launch_bins_blend(p, c->stream);
    TH_HIP(hipGetLastError());
    c->bins_dirty = false;          // (every reader of a list leaves its places and its table entries empty)
    return TH_OK;
}

th_status bins_pass_finish(th_context *c, th::DepositParams &p, uint64_t *fragments, bool blended_early)
{
    const uint32_t *host = c->bins_totals_host;
    const uint32_t total = host[th::kTotFragments], nlarge = host[th::kTotLarge];
    if (fragments) *fragments = total;
    c->last_draw.pipeline = TH_DRAW_BINS; c->last_draw.fragments = total; c->last_draw.crowded_fragments = host[th::kTotCrowdKeys];
    if (host[th::kTotCrowdKeys] == 0xffffffffu) return fail(TH_ERR_UNSUPPORTED, "too many fragments in crowded bins for one draw (2^32 or more places)");
    if (th_status s = crowd_room(c, p, nlarge, host[th::kTotCrowdKeys], total)) return s;
    return bins_pass_blend(c, p, blended_early);
}

// (row-band shards, th_shard.hip) the received bins are in the store, laid out by launch_bins_owner_insert: the totals of its
// plan to the host
void bins_pass_expect(th_context *c, th::DepositParams &p) { bins_expect(c, p); }
th_status bins_pass_totals(th_context *c, const th::DepositParams &p)
{
    TH_HIP(hipEventRecord(c->forked, c->stream));
    return bins_totals(c, p);
}

}  // namespace thi

th_status thi::deposit_run_bins(th_context *c, th::DepositParams &p, uint64_t *fragments, bool program, const FragmentStage *stage)
{
    if (th_status s = bins_streams(c)) return s;
    // Which comes first behind the emitting pass: the ordinary bins' blend - it needs nothing from the host and covers the
    // read-back - or, on a crowded target, the crowded bins' kernels: their long runs (walked by one thread each, on the
    // side stream) are then the longest chain of the draw and must start as early as they can.  Decided by the last draw.
    const bool early = !(c->last_draw.pipeline == TH_DRAW_BINS && (double)c->last_draw.crowded_fragments > kEarlyBlendShare * (double)c->last_draw.fragments);
    if (th_status s = bins_pass_emit(c, p, early, program, stage)) return s;
    return bins_pass_finish(c, p, fragments, early);
}

// ---- one pass, as its entry point describes it (PassSpec) ------------------------------------------------------------------------
// `p` readied for the pass, in front of its vertex kernel (want_bins, bins: as draw_pass hands them; an emit has neither)
static th_status pass_prepare(th_context *c, const PassSpec &s, th::DepositParams &p, bool want_bins, bool *bins)
{
    if (s.vertex) {
        const th_deposit_uniforms none{};                   // (viewSize, time, speedLimit are the program's own business)
        return deposit_prepare(c, &none, p, want_bins, bins, true, s.fragment);
    }
    if (s.pass == TH_PASS_VIEW) return view_params(c, static_cast<const th_render_uniforms *>(s.builtin), p, want_bins, bins, s.fragment);
    return deposit_prepare(c, static_cast<const th_deposit_uniforms *>(s.builtin), p, want_bins, bins, false, s.fragment);
}

// Through the pipeline the built-in pass of this context would take (deposit_prepare: the policy, the frame's one-pipeline rule, the
// gate; a fragment stage: stream-ordered, or under TH_OPT_STAGE_BINS the same pipeline with the stage over the page store).  With a vertex program, binned: the ring stays in the order it is held in, the vertex
// kernel fills the texel-indexed vertex buffer - over a sorted ring one lane per SLOT, the state read where it lies - and the bins
// walk the records in texel order; stream: the ring goes to texel order (held for a while), one lane per vertex - every attempt runs the vertex kernel.  A caller's stage
// made or coloured the lines: what a built-in pass left of its own (c->drawn) is not such a pass's, nor such a pass's a built-in's.
th_status thi::pass_run(th_context *c, const PassSpec &s, uint64_t *fragments)
{
    const bool view = s.pass == TH_PASS_VIEW, own_lines = s.vertex || s.fragment;
    if (own_lines) c->drawn.valid = false;
    if (view) if (th_status st = view_storage(c)) return st;
    const th_status ran = draw_pass(c, fragments, s.vertex != nullptr, s.fragment, [&](th::DepositParams &p, bool first, bool *bins) -> th_status {
        if (th_status st = pass_prepare(c, s, p, first, bins)) return st;
        if (view) p.view = c->view;
        return s.vertex ? vertex_stage_run(c, s, p, *bins) : TH_OK;
    });
    if (own_lines) c->drawn.valid = false;          // (deposit_run has said what it left: true of a built-in pass alone)
    return ran;
}

// always stream-ordered: the ring goes to texel order (deposit_prepare clears the out-of-band word), a vertex program fills the vertex buffer by local row, the tail of every emit
// keys and parts the fragments.  A row that neither the band nor a halo row holds - asked for by the vertex kernel or by the raster stage, on the same word - is one error, and nothing is handed out.
th_status thi::pass_emit(th_context *c, const PassSpec &s, uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (s.vertex || s.fragment) c->drawn.valid = false;
    if (th_status st = texels_fit_keys(c, s.pass == TH_PASS_VIEW ? "view" : "flow")) return st;
    if (s.vertex) { *count = 0; *keys_dev = nullptr; *colors_dev = nullptr; }        // (what a failure of the vertex stage hands out)
    th::DepositParams p;
    if (th_status st = pass_prepare(c, s, p, false, nullptr)) return st;
    if (s.vertex) if (th_status st = vertex_stage_band(c, s, p)) return st;
    return emit_parted(c, p, s.fragment, count, keys_dev, colors_dev);
}

extern "C" {

th_status th_export_lines(th_context *c, const th_deposit_uniforms *u, float *lines, uint64_t capacity, uint64_t *count)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(count, "null count");
    th::DepositParams p;
    if (th_status s = deposit_prepare(c, u, p)) return s;
    return export_run(c, p, lines, capacity, count);
}

th_status th_flow_deposit(th_context *c, const th_deposit_uniforms *u, uint64_t *fragments)
{
    if (th_status s = use(c)) return s;
    draw_moves_nothing(c);
    if (th_status s = refuse_band(c, "flow deposit", "use th_deposit_emit / th_deposit_merge with the exchange of tendrils_amd/sharding.py")) return s;
    return pass_run(c, builtin_pass(TH_PASS_FLOW, u), fragments);
}

// Both passes of Tendrils.draw() (src/index.js:278-337) in one: the lines are rasterised, scanned, emitted and sorted once,
// every fragment carries the flow pass's varying and the view pass's colour side by side, one gather brings both into
// the sorted order and each target is blended from its half.  The two passes must agree on what they draw: the same
// viewSize, time and speedLimit (what Tendrils.draw() hands to both); results are those of th_flow_deposit followed
// by th_view_draw.
th_status th_draw(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *fragments)
{
    if (th_status s = use(c)) return s;
    draw_moves_nothing(c);
    TH_REQUIRE(du && ru, "null uniforms");
    if (th_status s = refuse_band(c, "draw", "the passes go through th_deposit_emit / th_deposit_merge and th_view_emit / th_view_merge with the owners' exchange in between")) return s;
    if (th_status s = shared_uniforms(du, ru)) return s;
    if (drawn_line_width(c, TH_PASS_FLOW) != drawn_line_width(c, TH_PASS_VIEW)) {       // two widths: two rasterisations
        if (th_status s = pass_run(c, builtin_pass(TH_PASS_FLOW, du), fragments)) return s;
        return pass_run(c, builtin_pass(TH_PASS_VIEW, ru), nullptr);
    }
    if (th_status s = view_storage(c)) return s;
    return draw_pass(c, fragments, false, nullptr, [&](th::DepositParams &p, bool first, bool *bins) -> th_status {
        if (th_status s = deposit_prepare(c, du, p, first, bins)) return s;
        p.mode = 2;
        view_fields(c, ru, p);
        p.view = c->view;
        return TH_OK;
    });
}

th_status th_view_draw(th_context *c, const th_render_uniforms *u, uint64_t *fragments)
{
    if (th_status s = use(c, true)) return s;
    draw_moves_nothing(c);
    if (th_status s = refuse_band(c, "view pass", "use th_view_emit / th_view_merge with the owners' exchange in between")) return s;
    return pass_run(c, builtin_pass(TH_PASS_VIEW, u), fragments);
}

th_status th_view_fill(th_context *c, const float rgba[4])
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(rgba, "null colour");
    if (th_status s = view_storage(c)) return s;
    th::launch_view_fill(c->view, (size_t)c->view_w * c->view_h, make_float4(rgba[0], rgba[1], rgba[2], rgba[3]), c->stream);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

th_status th_view_clear(th_context *c)
{
    if (th_status s = use(c, true)) return s;
    if (th_status s = view_storage(c)) return s;
    TH_HIP(hipMemsetAsync(c->view, 0, (size_t)c->view_w * c->view_h * sizeof(uchar4), c->stream));
    return TH_OK;
}

// Tendrils.buffers (src/index.js:172-184, 359-391)
th_status th_view_buffers(th_context *c, int32_t count)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(count >= 0 && count <= 64, "bad number of view buffers %d", count);
    c->view_buffers = count;
    return view_storage(c);
}

th_status th_view_bind(th_context *c, int32_t index)
{
    if (th_status s = use(c, true)) return s;
    if (th_status s = view_storage(c)) return s;
    TH_REQUIRE(index >= -1 && index < (int32_t)c->view_ring.size(), "no view buffer %d (there are %zu)", index, c->view_ring.size());
    c->view = index < 0 ? c->view_screen : c->view_ring[(size_t)index];
    c->view_bound = index;
    return TH_OK;
}

th_status th_view_copy(th_context *c, int32_t index)
{
    if (th_status s = use(c, true)) return s;
    if (th_status s = view_storage(c)) return s;
    if (index < 0 || index >= (int32_t)c->view_ring.size()) return TH_OK;       // src/index.js:371: `if(index < this.buffers.length)`
    th::launch_view_copy(c->view, c->view_ring[(size_t)index], (size_t)c->view_w * c->view_h, c->stream);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

th_status th_view_step_buffers(th_context *c)
{
    if (th_status s = use(c, true)) return s;
    if (th_status s = view_storage(c)) return s;
    if (c->view_ring.size() > 1) {               // src/utils/index.js:1-7: array.unshift(array.pop())
        uchar4 *last = c->view_ring.back();
        c->view_ring.pop_back();
        c->view_ring.insert(c->view_ring.begin(), last);
    }
    return TH_OK;
}

th_status th_view_download(th_context *c, uint8_t *rgba8)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(rgba8, "null pixels");
    if (th_status s = view_storage(c)) return s;
    return image_download(c, rgba8, c->view, (size_t)c->view_w * c->view_h * sizeof(uchar4));
}

th_status th_colormap_upload(th_context *c, const float *rgba, int32_t w, int32_t h)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(rgba && w > 0 && h > 0 && (uint64_t)w * h < (1ull << 28), "bad colour map %dx%d", w, h);
    if (w != c->cmap_w || h != c->cmap_h) if (th_status s = image_reshape(c, c->colormap, c->cmap_w, c->cmap_h, w, h)) return s;
    return image_upload(c, c->colormap, rgba, (size_t)w * h * sizeof(float4));
}

th_status th_export_view_lines(th_context *c, const th_render_uniforms *u, float *lines, uint64_t capacity, uint64_t *count)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(count, "null count");
    th::DepositParams p;
    if (th_status s = view_params(c, u, p)) return s;
    return export_run(c, p, lines, capacity, count);
}

th_status th_draw_query(th_context *c, th_draw_info *out)
{
    TH_REQUIRE(c && out, "null argument");
    *out = c->last_draw;
    return TH_OK;
}

th_status th_line_width(th_context *c, int32_t pass, float width)
{
    TH_REQUIRE(c, "null context");
    TH_REQUIRE(pass == TH_PASS_FLOW || pass == TH_PASS_VIEW, "unknown pass %d", pass);
    TH_REQUIRE(width > 0.0f, "line width %g (gl.lineWidth: INVALID_VALUE, the width stays %g)", (double)width, (double)c->line_width[pass]);
    c->line_width[pass] = width;
    return TH_OK;
}

th_status th_line_width_range(th_context *c, float lo, float hi)
{
    TH_REQUIRE(c, "null context");
    TH_REQUIRE(lo > 0.0f && lo <= 1.0f && hi >= 1.0f && hi <= th::kMaxLineWidth, "line width range [%g, %g]: need 0 < lo <= 1 <= hi <= %g",
               (double)lo, (double)hi, (double)th::kMaxLineWidth);
    c->line_range[0] = lo; c->line_range[1] = hi;
    return TH_OK;
}

th_status th_line_width_query(th_context *c, int32_t pass, float *width, float *drawn, float *range)
{
    TH_REQUIRE(c, "null context");
    TH_REQUIRE(pass == TH_PASS_FLOW || pass == TH_PASS_VIEW, "unknown pass %d", pass);
    if (width) *width = c->line_width[pass];
    if (drawn) *drawn = drawn_line_width(c, pass);
    if (range) { range[0] = c->line_range[0]; range[1] = c->line_range[1]; }
    return TH_OK;
}

th_status th_draw_pipeline(th_context *c, int32_t which)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(which == TH_DRAW_AUTO || which == TH_DRAW_STREAM || which == TH_DRAW_BINS, "unknown draw pipeline %d", which);
    c->draw_pipeline = which;
    return TH_OK;
}

}  // extern "C"
