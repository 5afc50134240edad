// th_stepprog.hip - step programs: n steps of a caller's integrator in one launch.  new Tendrils(gl, { logicShader }) takes a
// caller's integrator (src/index.js:70, 107-113); as a state program (th_program.hip) it runs one launch per step and moves the
// ring through memory every time.  An integrator reads nothing of the ring but its own texel - the built-in one, src/logic.frag
// and the reference's Euler and Verlet bodies alike - and a step program is a state program whose contract is that restriction
// (th_step_prelude.inc: no th_particles).  Everything else a pass may read does not change inside a run of steps, so the steps
// of one particle run back to back with its state in registers, as th_step_n's fused launch runs the built-in integrator
// (th_step.hip): the ring is read once and written twice per launch of up to kMaxFusedSteps steps.
#include "th_ctx.hpp"

using namespace thi;

namespace {

// the tap rule and the packed-state codec as text (th_taps.inc, th_packed.inc: the library's kernels compile the same lines),
// then the prelude
#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#undef TH_TAPS
#define TH_PACKED(...) #__VA_ARGS__
const char kPacked[] =
#include "th_packed.inc"
    ;
#undef TH_PACKED
const char kPrelude[] =
#include "th_step_prelude.inc"
    ;

// the launch record (th_step_prelude.inc: th_step_args, th_program_uniform_block - the same layout)
struct StepArgs {
    const float4 *in;
    float4 *out, *out_prev;
    const float4 *data, *flow, *targets;
    const uint32_t *perm;
    uint32_t count, width, rows, row0, global_height;
    int32_t dw, dh, fw, fh;
    uint32_t nsteps, step0;
    float dt;
    float times[th::kMaxFusedSteps];
};
using KernArgs = ProgramKernArgs<StepArgs>;
static_assert(th::kMaxFusedSteps == 32 && sizeof(StepArgs) == 232 && offsetof(StepArgs, times) == 104 && offsetof(KernArgs, u) == 240 &&
                  sizeof(KernArgs) == 240 + kUniformBytes,
              "launch record: layout shared with th_step_prelude.inc");

// one launch of th_step_kernel or, on a packed ring, th_step_packed_kernel (th_kernel_timing: an event pair around it, as around every logic launch): in texel order on the
// grid of the streaming passes, over tile-sorted slots (k.a.perm) on the built-in fused launch's - 8 groups of workgroups, one
// per eighth of the slots (th::fused_grid)
th_status step_launch(th_context *c, hipFunction_t fn, KernArgs &k)
{
    LaunchTimer timer;
    if (th_status s = timer.begin(c)) return s;
    const int grid = k.a.perm ? th::fused_grid(k.a.count, true) : th::grid_for(c->texels(), 8);
    if (th_status s = program_launch_grid(c, fn, grid, &k, sizeof k)) return s;
    return timer.end(c);
}

}  // namespace

extern "C" {

th_status th_step_program_compile(const char *source, const char *name, th_program **out)
{
    return program_compile(kStepProgram, std::string(kTaps) + "\nnamespace th {\n" + kPacked + "\n}\n" + kPrelude, source, name, out);
}

th_status th_step_program_view_size(th_context *c, const float viewSize[2])
{
    if (th_status s = use(c, true)) return s;
    if (viewSize)
        for (int k = 0; k < 2; ++k)
            TH_REQUIRE(std::isfinite(viewSize[k]) && viewSize[k] > 0.0f, "viewSize[%d] = %g: a step program's sort key needs a finite, positive view size", k, (double)viewSize[k]);
    c->step_keyed = viewSize != nullptr;
    if (viewSize) { c->step_view[0] = viewSize[0]; c->step_view[1] = viewSize[1]; }
    return TH_OK;
}

// n passes with the ring semantics of TH_TARGET_RING: buffers[0] is state n afterwards, buffers[1] state n - 1.
//   fused:  the two-buffer ring with th_options::fuse on, f32 or packed - at most kMaxFusedSteps steps per launch, both outputs
//           routed as th_step_n routes them (a lane touches its own slot alone: one output may be the input buffer).
//           f32: the launches run over the slot order buffers[0] is held in (perm) and leave both buffers in it: a tile-sorted
//           ring stays sorted, stale or not (a stale order is still a permutation).  With a key (th_step_program_view_size) the
//           call first lays an order out or refreshes it, as th_step_n does (fused_slots); without one it never creates an order.
//           packed: texel order first (ensure_identity), key or no key, then th_step_packed_kernel in place on the 8-byte
//           texels - no f32 staging; the state is quantised after every step inside the launch, as the ring would hold it.
//   single: every other ring (more buffers: all of them rotate; fuse off) - texel order first (ensure_identity), then
//           th_step_kernel with nsteps = 1 between RingPass::begin and commit, once per step (a packed ring: through f32
//           staging, unpacked before and packed after every step)
// The state between the steps of a fused launch is exactly what a single pass stores: a call with n steps leaves the bits and
// the ring order of n calls with one.
th_status th_step_program_run(th_context *c, th_program *prog, const void *uniforms, uint32_t uniform_bytes, int32_t source,
                              const float *times, float dt, int32_t n)
{
    if (th_status s = use(c)) return s;
    if (th_status s = program_run_args(prog, kStepProgram, "th_step_program_run", uniforms, uniform_bytes)) return s;
    TH_REQUIRE(n >= 0, "%d steps", n);
    TH_REQUIRE(times || n == 0, "null times");
    TH_REQUIRE(!(source >= 0 && source < (int32_t)c->ring.size()),
               "state buffer %d as a step program's spawnData: the ring is what the call writes (a fused launch overwrites its input)", source);
    TH_REQUIRE(source == TH_SOURCE_NONE || source == TH_SOURCE_FLOW || source == TH_SOURCE_IMAGE, "bad spawnData source %d", source);
    TH_REQUIRE(c->ring.size() >= 2, "a pass needs at least 2 state buffers (have %zu)", c->ring.size());
    KernArgs k{};
    StepArgs &a = k.a;
    if (th_status s = spawn_data(c, source, nullptr, true, &a.data, &a.dw, &a.dh)) return s;
    if (n == 0) return TH_OK;
    ProgramModule *m = nullptr;
    if (th_status s = program_loaded(c, prog, &m)) return s;
    if (th_status s = asort_drop(c)) return s;
    const bool fused = c->opt.fuse && c->ring.size() == 2;
    if (!fused || c->packed) {
        if (th_status s = ensure_identity(c)) return s;  // these rings step in texel order, like every other program pass
    } else if (c->step_keyed) {
        const bool may_sort = sorting_possible(c) && c->total_steps >= c->hold_texel_order_until;
        if (th_status s = fused_slots(c, may_sort, tile_geom(c, c->step_view))) return s;
    }
    a.flow = c->flow; a.fw = c->fw; a.fh = c->fh;
    a.targets = c->targets;
    a.count = (uint32_t)c->texels(); a.width = (uint32_t)c->cfg.width; a.rows = (uint32_t)c->cfg.height;
    a.row0 = (uint32_t)c->cfg.row0; a.global_height = (uint32_t)c->cfg.global_height;
    a.dt = dt;
    k.set_uniforms(uniforms, uniform_bytes);

    if (fused) {
        for (int32_t done = 0; done < n;) {
            const int32_t steps = std::min<int32_t>(n - done, (int32_t)th::kMaxFusedSteps);
            const int order = order_of(c, c->ring[0]);
            const FusedRoute r = fused_route(c, steps);
            a.perm = order >= 0 ? c->orders[(size_t)order].perm : nullptr;
            a.in = r.in;
            a.out = r.out;                                           // state `steps`     (ends up in buffers[0])
            // state `steps` - 1 (ends up in buffers[1]) - of a single step it is the input, where it lies: a step program
            // stores none (the built-in kernel always does)
            a.out_prev = steps == 1 ? nullptr : r.out_prev;
            a.nsteps = (uint32_t)steps; a.step0 = (uint32_t)done;
            for (int32_t j = 0; j < steps; ++j) a.times[j] = times[(size_t)(done + j)];
            if (th_status s = step_launch(c, m->entry[c->packed ? kStepPacked : kStepF32], k)) return s;
            set_order(c, r.other, order);                            // both outputs sit at the input's slots (a single step's input stays)
            fused_routed(c, steps);
            done += steps;
        }
    } else {
        a.nsteps = 1; a.out_prev = nullptr; a.perm = nullptr;
        for (int32_t done = 0; done < n; ++done) {
            RingPass pass;
            if (th_status s = pass.begin(c, TH_TARGET_RING)) return s;
            a.in = pass.particles; a.out = pass.rt;
            a.step0 = (uint32_t)done; a.times[0] = times[(size_t)done];
            if (th_status s = step_launch(c, m->entry[kStepF32], k)) return s;
            if (th_status s = pass.commit(c)) return s;
            ++c->steps_since_sort; ++c->total_steps;
        }
    }
    // what is remembered of the buffers' content ended with use() and state_written(); the ring stays in the order it was stepped in, and
    // no pass of this call has counted tiles or taken statistics of what it wrote
    c->counted.buf = nullptr;
    c->fused_stats.valid = false;
    c->drawn.valid = false;
    return TH_OK;
}

}  // extern "C"
