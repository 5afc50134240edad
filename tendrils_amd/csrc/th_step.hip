// th_step.hip - Particles.step (src/particles.js:123-145) = one integrator pass over the state ring: th_step, and th_step_n =
// n fixed-step passes as one fused launch per <= 32 steps or a captured hipGraph.
#include "th_ctx.hpp"

using namespace thi;

namespace {

// Largest s2 with sqrt_rn(s2) <= limit (sqrt_rn monotonic), so that
// `0 < s2 <= cap` <=> `0 < speed <= speedLimit` <=> min(speed,limit)/speed == 1.
float s2_cap_for(float limit)
{
    if (!(limit > 0.0f)) return -1.0f;                       // never take the shortcut
    if (std::isinf(limit)) return std::numeric_limits<float>::max();
    double sq = (double)limit * (double)limit;
    if (sq >= (double)std::numeric_limits<float>::max()) return std::numeric_limits<float>::max();
    float c = (float)sq;
    while (sqrtf(c) > limit) c = nextafterf(c, 0.0f);
    for (;;) {
        float n = nextafterf(c, std::numeric_limits<float>::infinity());
        if (std::isinf(n) || sqrtf(n) > limit) break;
        c = n;
    }
    return c;
}

bool finite_uniforms(const th_logic_uniforms &u)
{
    const float *f = reinterpret_cast<const float *>(&u);
    for (size_t k = 0; k < sizeof(u) / sizeof(float); ++k)
        if (!std::isfinite(f[k])) return false;
    return true;
}

// The window of the noise lattice that one fused launch of m steps stays in (th_logic.hpp "over a window"):
// the bound on |pos| that goes with it and the bias constants of both evaluations.  In double; hulls over the index i in
// [0, 1] (vary() is linear in it) and uv in [0, 1]; every lattice range 2 cells wider each way than its hull, for the
// kernel's fp32 rounding (below 0.01 cell at these magnitudes).  false: a range is wider than a window, or reaches beyond
// the cells whose mod289_int is the true residue, or - a huge noiseScale - the bound on |pos| does not reach twice the view's
// half-extent (pos * viewSize in [-1, 1] is in sight): particles in and near plain sight would take the reference-order
// branch.  The launch then runs the kernel without the window, as every launch in fast mode does (th_logic.hpp: integrate, WIN).
constexpr double kWinNoiseUnits = 64.0;      // N: |pos * noiseScale'| <= N inside win_bound
constexpr double kWinMinViews = 2.0;         // win_bound * min|viewSize| at least this
bool hash_window(const th_logic_uniforms &u, float pos_bound, const float *times, int32_t m, float *win_bound, float (*win_k)[3])
{
    const double N = kWinNoiseUnits;
    const double scale0 = u.noiseScale, scale1 = scale0 + (double)u.varyNoiseScale * scale0;
    const double scale = std::fmax(std::fabs(scale0), std::fabs(scale1));
    *win_bound = (float)(scale > 0.0 ? std::fmin((double)pos_bound, N / scale) : (double)pos_bound);
    if (!((double)*win_bound * std::fmin(std::fabs((double)u.viewSize[0]), std::fabs((double)u.viewSize[1])) >= kWinMinViews)) return false;
    const double speed0 = u.noiseSpeed, speed1 = speed0 + (double)u.varyNoiseSpeed * speed0;
    double tlo = std::numeric_limits<double>::infinity(), thi = -tlo;
    for (int32_t k = 0; k < m; ++k)
        for (double speed : {speed0, speed1}) {
            const double nt = (double)times[k] * speed;
            tlo = std::fmin(tlo, nt); thi = std::fmax(thi, nt);
        }
    for (int e = 0; e < 2; ++e) {
        const double zlo = tlo + (e ? 1234.5678 : 0.0), zhi = thi + 1.0 + (e ? 1234.5678 : 0.0);    // z = uv + ntime (+ 1234.5678)
        const double slo = zlo / 3.0 - 2.0 * N / 3.0, shi = zhi / 3.0 + 2.0 * N / 3.0;                // s = (nx + ny + z) / 3
        const double lo[2] = {std::floor(-N + slo) - 2.0, std::floor(zlo + slo) - 2.0};               // ix, iy | iz
        const double hi[2] = {std::floor(N + shi) + 2.0, std::floor(zhi + shi) + 2.0};
        double c[2];
        for (int a = 0; a < 2; ++a) {
            if (!(hi[a] - lo[a] <= (double)th::kWinSpan)) return false;
            if (!(std::fmax(std::fabs(lo[a]), std::fabs(hi[a])) + 1.0 <= (double)th::kWinMaxCell)) return false;
            c[a] = 289.0 * std::floor(lo[a] / 289.0);
        }
        win_k[e][0] = (float)(2097152.0 - c[1]);      // 2^21 - cz
        win_k[e][1] = (float)(2097152.0 - c[0]);      // 2^21 - cxy
        win_k[e][2] = (float)(524288.0 - c[0]);       // 2^19 - cxy
    }
    return true;
}

}  // namespace

// ---- one integrator pass = plan (host decisions, may synchronise) + enqueue (launches only) -------
struct StepPlan {
    th::LogicParams p{};         // everything except in / out / perm / time_dev
    th::LogicVariant v;          // the specialised kernel's variant ...
    bool generic = false;        // ... unless the pass runs the generic kernel
    bool may_sort = false;       // this pass may run on (and produce) tile-sorted slots
};

// Pick the kernel variant and bring the slot layout up to date.  `u.time` must be the time of
// largest magnitude the plan will be used with (it only enters the domain checks here).
static th_status plan_step(th_context *c, const th_logic_uniforms &u, int32_t target, StepPlan &plan)
{
    const uint32_t W = (uint32_t)c->cfg.width, H = (uint32_t)c->cfg.global_height;
    th::LogicParams &p = plan.p;
    p = th::LogicParams{};
    p.flow = c->flow; p.flow_dec = c->flow_dec; p.targets = c->targets; p.lut = c->lut;
    p.count = (uint32_t)c->texels();
    p.width = W;
    p.row0 = (uint32_t)c->cfg.row0;
    p.wf = (float)W; p.hf = (float)H;
    th::LogicVariant &v = plan.v;
    v = th::LogicVariant{};
    v.mode = c->cfg.mode;
    v.pow2 = is_pow2(W) && is_pow2(H);
    p.log2w = v.pow2 ? ilog2(W) : 0;
    p.inv_w = 1.0f / p.wf; p.inv_h = 1.0f / p.hf; p.inv_wh = 1.0f / (p.wf * p.hf);
    p.fw = c->fw; p.fh = c->fh;
    p.fwf = (float)c->fw; p.fhf = (float)c->fh;
    p.half_fw = 0.5f * p.fwf; p.half_fh = 0.5f * p.fhf;
    p.fwm1 = (float)(c->fw - 1); p.fhm1 = (float)(c->fh - 1);
    p.u = u;
    p.s2_cap = s2_cap_for(u.speedLimit);

    // Preconditions of the specialised path (DESIGN.md "fast-path domain").
    plan.generic = c->opt.force_generic || !finite_uniforms(u);
    v.noise = u.noiseWeight != 0.0f;
    v.target = u.target != 0.0f;
    if (!plan.generic) {
        // i = (x+.5 + (y+.5)W)/(WH) lies in (0, 1]; bound |vary(base, i, v)| <= |base|(1+|v|)
        double nscale = std::fabs((double)u.noiseScale) * (1.0 + std::fabs((double)u.varyNoiseScale)) * 1.001;
        double ntime = std::fabs((double)u.time) * std::fabs((double)u.noiseSpeed) *
                       (1.0 + std::fabs((double)u.varyNoiseSpeed)) * 1.001;
        if (ntime + 1237.0 >= (double)th::kNoiseDomain) plan.generic = true;  // z = uv + noiseTime (+1234.5678)
        double bound = nscale > 0.0 ? (double)th::kNoiseDomain / nscale : 3.0e38;
        // capped below |inert| = 1e6: a lane inside the bound cannot be inert, so the specialised path tests
        // the bound only and the inert pass-through lives on the (reference-order) fallback path
        p.pos_bound = (float)std::fmin(bound * 0.999, 999999.0);
        if (!(p.pos_bound > 0.0f)) plan.generic = true;
    }
    if (!plan.generic && !v.target) {
        // target == 0 multiplies (targets - pos) by an exact zero; dropping the read is only
        // value-preserving when the texture holds no NaN/Inf.
        if (!c->targets_checked) {
            unsigned int flag = 0;
            TH_HIP(hipMemsetAsync(c->d_flag, 0, sizeof(unsigned int), c->stream));
            th::launch_finite_check(c->targets, c->texels(), c->d_flag, c->stream);
            TH_HIP(hipMemcpyAsync(&flag, c->d_flag, sizeof flag, hipMemcpyDeviceToHost, c->stream));
            TH_HIP(hipStreamSynchronize(c->stream));
            c->targets_nonfinite = flag != 0;
            c->targets_checked = true;
        }
        v.target = c->targets_nonfinite;
    }
    // Decode the flow once per step when that is cheaper than decoding per particle: it shrinks the
    // random-gather footprint (the L2/Infinity-Fabric miss traffic is what bounds this kernel).
    const size_t flow_texels = (size_t)c->fw * c->fh;
    v.decoded = !plan.generic && c->texels() >= 2 * flow_texels;
    // A packed (TH_STATE_F16) ring runs the packed kernel on the default path (ring -> ring, specialised kernel); explicit
    // targets and the generic kernel go through f32 staging.
    v.format = c->packed && target == TH_TARGET_RING && !plan.generic ? th::StateFormat::packed : th::StateFormat::f32;

    // Slot layout (texel order or a tile-sorted order): only ring -> ring passes of the specialised f32 kernels run on
    // sorted slots; the callers bring the layout up to date.
    plan.may_sort = v.decoded && target == TH_TARGET_RING && sorting_possible(c) &&
                    c->total_steps >= c->hold_texel_order_until;
    return TH_OK;
}

// what a captured th_step_n sequence depends on besides the ring order and the kernel flags (`time` excluded: it lives in
// device memory); an explicit field list - the struct has padding and fields the captured launches never read
static bool same_key(const th::LogicParams &a, const th::LogicParams &b)
{
    th_logic_uniforms ua = a.u, ub = b.u;
    ua.time = ub.time = 0.0f;
    return a.flow == b.flow && a.flow_dec == b.flow_dec && a.targets == b.targets && a.lut == b.lut &&
           a.count == b.count && a.width == b.width && a.log2w == b.log2w && a.row0 == b.row0 &&
           a.wf == b.wf && a.hf == b.hf && a.fw == b.fw && a.fh == b.fh &&
           memcmp(&ua, &ub, sizeof ua) == 0 && a.s2_cap == b.s2_cap && a.pos_bound == b.pos_bound;
}

th_status thi::LaunchTimer::begin(th_context *c, bool on)
{
    if (!on || !c->kernel_timing) return TH_OK;
    if (c->kt_used + 2 > c->kt_events.size()) {          // (timing_events: the next pair, made on first use)
        hipEvent_t a = nullptr, b = nullptr;
        TH_HIP(hipEventCreate(&a)); TH_HIP(hipEventCreate(&b));
        c->kt_events.push_back(a); c->kt_events.push_back(b);
    }
    hipEvent_t k0 = c->kt_events[c->kt_used]; k1 = c->kt_events[c->kt_used + 1];
    c->kt_used += 2;
    TH_HIP(hipEventRecord(k0, c->stream));
    return TH_OK;
}
th_status thi::LaunchTimer::end(th_context *c)
{
    if (k1) TH_HIP(hipEventRecord(k1, c->stream));
    return TH_OK;
}

// a lane only ever touches its own texel, so one of the two outputs may overwrite the input;
// after m rotations of [cur, other]: m even -> [cur, other], m odd -> [other, cur]
thi::FusedRoute thi::fused_route(th_context *c, int32_t m)
{
    float4 *cur = c->ring[0], *other = c->ring[1];
    state_written(c, cur); state_written(c, other);
    return {cur, (m & 1) ? other : cur, (m & 1) ? cur : other, other};
}
void thi::fused_routed(th_context *c, int32_t m)
{
    if (m & 1) std::swap(c->ring[0], c->ring[1]);
    c->steps_since_sort += m; c->total_steps += m;
}

// ---- one pass, stage by stage (enqueue_step) ----------------------------------------------------
struct StepSlots {               // what the stages hand on: the pass's buffers and what its slot plan decided
    float4 *in = nullptr, *out = nullptr, *rt = nullptr;     // the input, the target, where the pass writes it (staging when packed)
    int in_order = -1, out_order = -1;                       // the slot orders they are held in (-1: texel order)
    // the sorted pass - first sort (in_order < 0), re-sort (scatter) or count in place - or the plain kernel over the slots (gather)
    bool use_sorted = false, scatter = false, count = false, gather = false;
    bool async = false, seeing = false;      // the re-sort runs beside the draws (asort_start); the pass notes what may touch the view
};

// Buffers and staging: the target (the ring rotated for TH_TARGET_RING) and the input - Particles.step binds buffers[1] as
// `particles` (src/particles.js:139); a packed ring under an f32 kernel goes through f32 staging on both sides.
static th_status step_buffers(th_context *c, bool packed_kernel, int32_t target, StepSlots &s)
{
    if (th_status st = resolve_target(c, target, true, &s.out)) return st;
    s.in = c->ring[1]; s.rt = s.out;
    if (c->packed && !packed_kernel) {
        if (th_status st = unpacked_view(c, c->ring[1], 1, &s.in)) return st;
        if (th_status st = render_target(c, s.out, 0, &s.rt)) return st;
    }
    return TH_OK;
}

// The slot plan of a packed ring: the plain grid-stride kernel over the sorted slots; a re-sort is a plain move of the input
// (tile_hist, scan, tile_scatter into the spare buffer, which then takes the input's place in the ring).
static th_status plan_packed_slots(th_context *c, th::LogicParams &p, StepSlots &s)
{
    const th::TileGeom g = tile_geom(c, p.u);
    if (s.in_order < 0 || order_stale(c, s.in_order, g) || c->steps_since_sort >= c->opt.resort_steps) {
        int fresh = -1;
        th::TileSortParams b;
        if (th_status st = begin_sort(c, g, s.in, s.in_order >= 0 ? c->orders[(size_t)s.in_order].perm : nullptr, &fresh, &b)) return st;
        b.state_out = c->spare;
        th::launch_tile_scatter(b, c->stream);
        TH_HIP(hipGetLastError());
        clear_graphs(c);               // captured sequences name the ring buffers: one of them changes places with the spare
        // (a packed kernel's input is ring[1] itself, and no other ring element is that allocation)
        ring_trade(c, c->ring[1], c->spare, fresh);
        s.in = c->ring[1]; s.in_order = fresh;
    }
    p.perm = c->orders[(size_t)s.in_order].perm;
    s.out_order = s.in_order;
    return TH_OK;
}

// The slot plan of an f32 pass.  The input keeps its order; the output is written either at the same slots or - every
// c->opt.resort_steps steps, and when the input is not sorted yet or was sorted for another view / field shape - at
// the slots of a new sort keyed on the input positions (counted just before the launch).
static th_status plan_f32_slots(th_context *c, const StepPlan &plan, int32_t target, th::LogicParams &p, StepSlots &s)
{
    const th::TileGeom g = tile_geom(c, p.u);
    if (order_stale(c, s.in_order, g)) {   // the chunk table no longer describes the field: start over from texel order
        if (th_status st = ensure_identity(c)) return st;
        s.in = c->ring[1]; s.out = s.rt = c->ring[0];
        s.in_order = -1;
    }
    // The re-sort of a frame loop (th_order.hip: asort_start): while draws over the slot order are going on, no step counts
    // or scatters - the order laid out beside the last draw is taken up here, its copy of this step's input in the input's
    // place - and the next one is started behind the step that is `resort_steps` launches on.
    const bool drawing = c->total_steps - c->last_binned_draw <= 2ll * c->opt.resort_steps;
    s.async = c->opt.async_sort && s.in_order >= 0 && plan.v.decoded && c->side && s.in == c->ring[1] && target == TH_TARGET_RING && drawing;
    if (c->asort.pending) {
        const bool take = s.async && c->asort.valid && c->asort.src == s.in && c->asort.src_order == s.in_order && c->asort.at_step == c->total_steps &&
                          same_geom(c->orders[(size_t)c->asort.order].geom, g);
        if (th_status st = take ? asort_take(c) : asort_drop(c)) return st;
        if (take) { s.in = c->ring[1]; s.in_order = c->asort.order; }
    }
    s.scatter = !s.async && (s.in_order < 0 || c->steps_since_sort >= c->opt.resort_steps);
    s.use_sorted = true;
    // between two sorts the pass is the plain grid-stride kernel over the sorted slots (taps gathered from the
    // decoded plane: a wave's taps fall into one neighbourhood); the chunk kernel counts and scatters around a re-sort
    s.gather = !s.scatter && plan.v.decoded && (s.async || c->steps_since_sort + 1 < c->opt.resort_steps);
    p.geom = g;
    if (s.in_order >= 0) {
        const th_context::SlotOrder &o = c->orders[(size_t)s.in_order];
        p.perm = o.perm; p.chunks = o.chunks; p.nchunks = o.nchunks; p.records = o.records;
    }
    if (s.scatter) {
        // counted by the pass that wrote `in`?  Then the histogram is complete and every chunk has its table.
        const bool counted = s.in_order >= 0 && c->counted.buf == s.in && c->counted.order == s.in_order &&
                             same_geom(c->counted.geom, g) && c->counted.at_step == c->total_steps;
        set_order(c, s.out, -1);       // the output buffer's old content (and order) dies here
        th::TileSortParams b;
        if (th_status st = begin_sort(c, g, s.in, s.in_order >= 0 ? c->orders[(size_t)s.in_order].perm : nullptr, &s.out_order, &b, counted)) return st;
        p.cursor = b.cursor; p.perm_out = b.perm_out;
        p.use_records = counted ? 1u : 0u;
        // draws over the slot order are going on (th_bins.hip): the pass moves its INPUT along to the new slots, so
        // that buffers[0] and buffers[1] - the two ends of every line - stay in one order
        if (s.in == c->ring[1] && drawing) p.in_moved = c->spare;
    } else {
        s.out_order = s.in_order;
        s.count = !s.gather && c->steps_since_sort + 1 >= c->opt.resort_steps;      // the next pass will re-sort: count for it
        if (s.count) {
            if (th_status st = sort_storage(c)) return st;
            p.hist = c->tile_mem;
            TH_HIP(hipMemsetAsync(p.hist, 0, kTileWords / 2 * sizeof(uint32_t), c->stream));
        }
    }
    return TH_OK;
}

// A frame loop: the plain kernel notes per 64 slots whether any of their lines - input position to output position - may
// touch the view (LogicParams::seen); the draw that follows skips the blocks of 256 slots of which none may (44 % of the
// bench's particles live outside the view, and the tile order keeps them together).  Hidden for sure = both ends beyond one
// edge by more than 2 texels: more than a line of width <= 2 reaches (its diamonds: one texel) and its snapping moves.
// Never inside a stream capture (th_step_n's graphs: time_dev set): the bytes would be allocated on a capturing thread, the
// captured launch would keep writing them at every replay, and `seen` would describe a launch that has not run.
static th_status step_sees(th_context *c, const StepPlan &plan, int32_t target, th::LogicParams &p, StepSlots &s)
{
    const float vx = p.u.viewSize[0], vy = p.u.viewSize[1];
    if (!(c->opt.skip_unseen && !p.time_dev && target == TH_TARGET_RING && !c->packed && !plan.generic && (s.gather || !s.use_sorted) && s.rt == s.out &&
          c->total_steps - c->last_binned_draw <= 2ll * c->opt.resort_steps && vx > 0.0f && vy > 0.0f && std::isfinite(vx) && std::isfinite(vy)))
        return TH_OK;
    if (!c->seen.bytes) {
        const size_t bytes = ((c->texels() + 63) / 64 + 7) & ~(size_t)3;
        if (th_status st = c->seen.bytes.alloc(bytes)) return st;
        TH_HIP(hipMemsetAsync(c->seen.bytes, 0, bytes, c->stream));
    }
    const float mx = 4.0f / (float)c->fw, my = 4.0f / (float)c->fh;
    p.seen = c->seen.bytes;
    p.seen_xlo = (-1.0f - mx) / vx; p.seen_xhi = (1.0f + mx) / vx;
    p.seen_ylo = (-1.0f - my) / vy; p.seen_yhi = (1.0f + my) / vy;
    s.seeing = true;
    return TH_OK;
}

// the kernel the plan asks for, between the th_kernel_timing events (`timing`: never inside a capture)
static th_status launch_step(th_context *c, const StepPlan &plan, bool timing, const th::LogicParams &p, const StepSlots &s)
{
    LaunchTimer timer;
    if (th_status st = timer.begin(c, timing)) return st;
    if (s.use_sorted && !s.gather) {
        const th::SortedPass pass = s.in_order < 0 ? th::SortedPass::first_sort : s.scatter ? th::SortedPass::resort : th::SortedPass::count_in_place;
        th::launch_logic_sorted(p, plan.v, pass, c->max_chunks, c->stream);
    } else if (plan.generic)
        th::launch_logic_generic(p, c->stream);
    else
        th::launch_logic(p, plan.v, c->stream);
    if (th_status st = timer.end(c)) return st;
    TH_HIP(hipGetLastError());
    return TH_OK;
}

// behind the launch: the output's order, the moved input, the packed commit, what the pass saw and counted, the next re-sort
static th_status step_done(th_context *c, bool packed_kernel, int32_t target, const th::LogicParams &p, const StepSlots &s)
{
    if (target == TH_TARGET_RING || (target >= 0 && target < (int32_t)c->ring.size())) set_order(c, s.out, s.out_order);
    if (p.in_moved) {                       // the moved copy takes the input's place in the ring
        clear_graphs(c);
        ring_trade(c, c->ring[1], c->spare, s.out_order);
    }
    if (c->packed && !packed_kernel)
        if (th_status st = commit_target(c, s.out, s.rt)) return st;
    if (s.seeing) {
        c->seen.cur = s.out; c->seen.prev = s.in; c->seen.order = s.out_order;
        c->seen.stamp = s.out_order >= 0 ? c->orders[(size_t)s.out_order].stamp : 0ull;
        c->seen.view_x = p.u.viewSize[0]; c->seen.view_y = p.u.viewSize[1]; c->seen.fw = c->fw; c->seen.fh = c->fh;
    }
    ++c->steps_since_sort; ++c->total_steps;
    if (s.count) { c->counted.buf = s.out; c->counted.order = s.out_order; c->counted.geom = p.geom; c->counted.at_step = c->total_steps; }
    else c->counted.buf = nullptr;
    if (s.async && !c->asort.pending && s.out_order >= 0 && c->steps_since_sort >= c->opt.resort_steps)
        return asort_start(c, p.geom, s.out, s.out_order);
    return TH_OK;
}

// Rotate / resolve the render target and launch (flow decode +) the integrator.  Launches only:
// safe inside a stream capture.  `time_dev` (optional) overrides plan.p.u.time on the device.
// `sorted`: the pass may read and write tile-sorted slots (else every ring buffer is in texel order already).
static th_status enqueue_step(th_context *c, const StepPlan &plan, int32_t target, float time, const float *time_dev,
                              bool timing, bool sorted = false)
{
    th::LogicParams p = plan.p;
    const bool packed_kernel = plan.v.format == th::StateFormat::packed;      // (else a packed ring goes through f32 staging)
    StepSlots s;
    if (th_status st = step_buffers(c, packed_kernel, target, s)) return st;
    p.u.time = time;
    p.time_dev = time_dev;
    s.in_order = sorted ? order_of(c, s.in) : -1;
    if (c->asort.pending && (!sorted || packed_kernel)) if (th_status st = asort_drop(c)) return st;
    if (sorted)
        if (th_status st = packed_kernel ? plan_packed_slots(c, p, s) : plan_f32_slots(c, plan, target, p, s)) return st;
    p.in = s.in;
    p.out = s.rt;
    if (plan.v.decoded)
        th::launch_flow_decode(c->flow, c->flow_dec, (size_t)c->fw * c->fh, time, time_dev, p.u.flowDecay, c->stream);
    if (th_status st = step_sees(c, plan, target, p, s)) return st;
    if (th_status st = launch_step(c, plan, timing, p, s)) return st;
    return step_done(c, packed_kernel, target, p, s);
}

// ---- th_step_n's three paths --------------------------------------------------------------------
// Temporal fusion (logic_fused_kernel): all n steps of a particle in one pass, <= kMaxFusedSteps per launch.
static th_status step_n_fused(th_context *c, const StepPlan &plan, const std::vector<float> &times, int32_t n)
{
    if (th_status s = fused_slots(c, plan.may_sort, tile_geom(c, plan.p.u))) return s;
    // The field does not change inside the call.  Without the noise the pass waits for its taps (a dependent gather per
    // step): the field's x, y, z packed 12 B apart once per call - three quarters of the footprint, and the band one
    // XCD taps fits its L2 (0.574 -> 0.546 ms per 20-step launch at C3; with the noise on the pass is bound by its
    // arithmetic and the packing pass only costs: 1.829 against 1.818 + 0.01)
    const bool pack3 = th::fused_taps_flow3(plan.v);
    if (pack3) {
        if (!c->flow3) if (th_status s = c->flow3.alloc((size_t)c->fw * c->fh * 3)) return s;
        th::launch_flow_pack3(c->flow, c->flow3, (size_t)c->fw * c->fh, c->stream);
    }
    for (int32_t done = 0; done < n;) {
        const int32_t m = std::min<int32_t>(n - done, (int32_t)th::kMaxFusedSteps);
        th::LogicParams p = plan.p;
        p.flow3 = pack3 ? c->flow3 : nullptr;
        const int order = order_of(c, c->ring[0]);
        const FusedRoute r = fused_route(c, m);
        p.in = r.in;
        p.out = r.out;                             // state m     (ends up in buffers[0])
        p.out_prev = r.out_prev;                   // state m - 1 (ends up in buffers[1]; m == 1: state 0 back into its own buffer)
        p.perm = order >= 0 ? c->orders[(size_t)order].perm : nullptr;
        p.nsteps = (uint32_t)m;
        for (int32_t k = 0; k < m; ++k) p.times[k] = times[(size_t)(done + k)];
        const bool window = plan.v.noise && plan.v.mode != TH_MODE_FAST && c->opt.hash_window && hash_window(p.u, p.pos_bound, p.times, m, &p.win_bound, p.win_k);
        if (window) p.win = c->win_block;
        // the last launch of the call takes the statistics of the state it leaves in buffers[0] (a packed ring's: of
        // what the stored texels decode to)
        const bool takes_stats = done + m == n;
        if (takes_stats) {
            const uint32_t parts = th::fused_stats_parts(p.count, p.perm != nullptr), need = parts + (parts + 255u) / 256u + 16u;
            if (c->fused_parts.size() < need) {
                TH_HIP(hipStreamSynchronize(c->stream));
                // (no memset, here or in front of a launch: every wave writes its partial - an empty one where it met no particle)
                if (th_status s = c->fused_parts.alloc(need)) return s;
            }
            p.stats_part = c->fused_parts;
            c->fused_stats.nparts = parts; c->fused_stats.limit = p.u.speedLimit;
        }
        LaunchTimer timer;
        if (th_status s = timer.begin(c)) return s;
        th::launch_logic_fused(p, plan.v, c->stream);
        if (th_status s = timer.end(c)) return s;
        TH_HIP(hipGetLastError());
        if (window) ++c->hash_window_launches;
        set_order(c, r.other, order);              // both outputs sit at the input's slots
        c->counted.buf = nullptr;
        fused_routed(c, m);
        done += m;
        if (takes_stats) { c->fused_stats.valid = true; c->fused_stats.buf = c->ring[0]; }
    }
    return TH_OK;
}

// step by step, in texel order: one plan per step (the domain checks see every step's time)
static th_status step_n_single(th_context *c, th_logic_uniforms v, StepPlan &plan, const std::vector<float> &times, int32_t n)
{
    for (int32_t k = 0; k < n; ++k) {
        if (k) { v.time = times[(size_t)k]; if (th_status s = plan_step(c, v, TH_TARGET_RING, plan)) return s; }
        if (th_status s = enqueue_step(c, plan, TH_TARGET_RING, times[(size_t)k], nullptr, true)) return s;
    }
    return TH_OK;
}

// The launch sequence (2 kernels per step) is captured once into a hipGraph per (n, uniforms, ring order, layout) and
// replayed; the per-step `time` values live in a small device array refreshed before every replay, so replays need no
// node updates.
static th_status step_n_graph(th_context *c, const StepPlan &plan, const std::vector<float> &times, int32_t n)
{
    // cache lookup: same n, same parameters (time excluded), same ring order and layout
    th::LogicParams key = plan.p;
    key.u.time = 0.0f;
    GraphEntry *hit = nullptr;
    for (GraphEntry &g : c->graphs)
        if (g.n == n && g.variant == plan.v && g.generic == plan.generic && g.ring == c->ring && same_key(g.key, key)) { hit = &g; break; }
    if (!hit) {
        if (c->graphs.size() >= 8) { destroy_graph(c->graphs.front()); c->graphs.erase(c->graphs.begin()); }
        GraphEntry g;
        g.n = n; g.variant = plan.v; g.generic = plan.generic; g.ring = c->ring; g.key = key;
        if (th_status s = g.times_dev.alloc((size_t)n)) return s;
        if (th_status s = g.times_host.alloc((size_t)n)) return s;
        TH_HIP(hipEventCreate(&g.copied));
        const std::vector<float4 *> ring_before = c->ring;
        const int since_before = c->steps_since_sort;
        const long long total_before = c->total_steps;
        hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
        th_status st = TH_OK;
        if (e == hipSuccess) {
            for (int32_t k = 0; k < n && st == TH_OK; ++k)
                st = enqueue_step(c, plan, TH_TARGET_RING, 0.0f, g.times_dev + k, false);
            hipGraph_t graph = nullptr;
            e = hipStreamEndCapture(c->stream, &graph);
            if (e == hipSuccess && st == TH_OK) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
        }
        c->ring = ring_before;                         // the capture only recorded; nothing ran yet
        c->steps_since_sort = since_before;
        c->total_steps = total_before;
        if (e != hipSuccess || st != TH_OK) {
            destroy_graph(g);
            return st != TH_OK ? st : fail(TH_ERR_HIP, "graph capture failed: %s", hipGetErrorString(e));
        }
        c->graphs.push_back(std::move(g));
        hit = &c->graphs.back();
    }
    TH_HIP(hipEventSynchronize(hit->copied));          // previous replay's copy out of times_host is done
    memcpy(hit->times_host, times.data(), (size_t)n * sizeof(float));
    TH_HIP(hipMemcpyAsync(hit->times_dev, hit->times_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    TH_HIP(hipGraphLaunch(hit->exec, c->stream));
    for (int32_t k = 0; k < n; ++k) (void)ring_rotate(c);      // host-side ring bookkeeping of the n rotations
    // the replay wrote the buffers the capture's resolve_target() calls named - at capture time only: what is remembered of
    // their content (a step's `seen` bytes, a gathered copy, a re-sort's copy) ends here, as it does behind a plain step
    for (float4 *r : c->ring) state_written(c, r);
    c->steps_since_sort += n; c->total_steps += n;
    // times_host must stay untouched until the copy has run; a later replay of this entry waits here
    TH_HIP(hipEventRecord(hit->copied, c->stream));
    return TH_OK;
}

extern "C" {

th_status th_step(th_context *c, const th_logic_uniforms *u, int32_t target)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(u, "null uniforms");
    // Particles.step reads this.buffers[1] (src/particles.js:139): needs >= 2 buffers
    TH_REQUIRE(c->ring.size() >= 2, "step needs at least 2 state buffers (have %zu)", c->ring.size());
    StepPlan plan;
    if (th_status s = plan_step(c, *u, target, plan)) return s;
    const bool sorted = plan.may_sort && !plan.generic;
    if (!sorted) { if (th_status s = asort_drop(c)) return s; if (th_status s = ensure_identity(c)) return s; }
    return enqueue_step(c, plan, target, u->time, nullptr, true, sorted);
}

// n fixed-step Tendrils.step() calls: fused launches, or single steps - replayed from a captured graph where that is on.
th_status th_step_n(th_context *c, const th_logic_uniforms *u, double time0, double dt_ms, int32_t n)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(u && n >= 0, "bad arguments");
    TH_REQUIRE(c->ring.size() >= 2, "step needs at least 2 state buffers (have %zu)", c->ring.size());
    if (n == 0) return TH_OK;
    if (th_status s = asort_drop(c)) return s;          // (a frame loop's re-sort under way: these launches lay their own orders out)
    th_logic_uniforms v = *u;
    v.dt = (float)dt_ms;
    std::vector<float> times((size_t)n);
    double t = time0, tmax = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        t += dt_ms;                                   // src/timer.js:28-31: time accumulates in double
        times[(size_t)k] = (float)t;
        if (std::fabs(t) > std::fabs(tmax)) tmax = t;
    }
    v.time = (float)tmax;
    StepPlan plan;
    if (th_status s = plan_step(c, v, TH_TARGET_RING, plan)) return s;
    // Fusion needs the plain 2-buffer ring (only the last two states survive n rotations) and the specialised kernel;
    // both ring formats.  th_options::fuse = 0 turns it off (the tests compare both paths).
    if (c->opt.fuse && n >= 2 && c->ring.size() == 2 && !plan.generic) return step_n_fused(c, plan, times, n);
    if (th_status s = ensure_identity(c)) return s;     // everything else runs in texel order
    if (!c->opt.graph || n < 2 || (c->packed && plan.generic)) return step_n_single(c, v, plan, times, n);
    return step_n_graph(c, plan, times, n);
}

}  // extern "C"
