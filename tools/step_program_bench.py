"""GPU time of n fused steps of a step program (tendrils_amd/csrc/th_stepprog.hip) against the ways to run the same steps, on one
MI355X.

Workload: 4096 x 4096 particles (a 256 MiB RGBA32F ring buffer), flow 1920 x 1080, 20 steps per call, two programs - the drift
program (pos += vel * dt) and this repository's flow-only integrator (a flow tap, decay, force, damping, speed clamp, Euler).
Arms, all in this process (one library), each on a context of its own:
  fused        one th_step_program_run(n = 20): 16 B read + 32 B written per particle and call
  fused sorted (flow_only) the fused call on a context with the sort key set (Particles.step_view_size) and `bucket` at its
               default: the call keeps the slots tile-sorted where the auto policy sorts, as th_step_n does - same bits
  single       the same call with the option `fuse` off: 20 launches of the same kernel, 32 B per particle-step
  state_prog   20 x th_program_run of the program's state-program form: what there was before step programs
  builtin      th_step_n(20) of the built-in integrator with the noise off (the flow-only program's arithmetic, the library's
               own fused launch, tile-sorted slots where its policy sorts)
  memcpy_d2d   hipMemcpyAsync, device to device, of one 256 MiB buffer: 1.5 x this is 16 B in + 32 B out per particle
Each figure is the GPU time per call between two events on the context's stream (th_timer_start / th_timer_stop around --reps
calls, after --warmup calls); the arms alternate for --rounds rounds and the median round is reported, with the spread.  The
programs' registers / scratch / code size (th_program_query) go out with the figures.


The packed arm (--packed): the same two programs, 20 steps a call, on a packed ring (TH_STATE_F16, 8 B per particle) at every
--sizes entry the card's free memory allows (4096 and 16384: config 5's 268 M particles).  Arms per size and program:
  fused        one th_step_program_run(n = 20) with `fuse` on: where the library has th_step_packed_kernel, one launch in place
               on the packed texels - 8 B read + 16 B written per particle; before it, the staged path below
  single       the same call with `fuse` off: per step unpack into f32 staging, the f32 kernel, pack - 80 B per particle-step
  copy24       hipMemcpyAsync, device to device, of 12 B per particle: 24 B per particle through HBM, the fused call's traffic
With --against LIB the whole measurement runs in child processes, one library each (TH_LIB), alternating LIB - the parent
commit's build - and this tree's for --runs runs each in ONE session, and the fused arms are compared across the builds.  Each
child also reports the device memory the process took (torch.cuda.mem_get_info before the contexts and after the calls; the ring
is filled through th_state_device_ptr, so no staging exists but what the calls allocate) and the wall time of
StepProgram.from_source for both programs.

Usage: python tools/step_program_bench.py [--size 4096] [--steps 20] [--reps 5] [--warmup 2] [--rounds 5] [--out FILE]
       python tools/step_program_bench.py --packed [--sizes 4096 16384] [--against LIB] [--runs 2] [--steps 20] ... [--out FILE]
       (--out appends the measurement to FILE, behind whatever it holds)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_DRIFT = """__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self;
    p.x = p.x + p.z * s.dt;
    p.y = p.y + p.w * s.dt;
    return p;
}
"""
STATE_DRIFT = """struct Drift { float dt; };
__device__ float4 th_main(const th_pass &p)
{
    const Drift &u = th_uniforms<Drift>(p);
    float4 s = p.self;
    s.x = s.x + s.z * u.dt;
    s.y = s.y + s.w * u.dt;
    return s;
}
"""
# the flow-only integrator (tendrils_amd/csrc/th_logic.hpp: logic_texel_ref without its noise and target terms); %(...)s: the
# entry point, the pass type and where time / dt come from
FLOW_ONLY = """struct Logic {
    float viewSize[2];
    float time, dt, speedLimit, damping, forceWeight, flowWeight, noiseWeight, flowDecay, noiseSpeed, noiseScale, target;
    float varyForce, varyFlow, varyNoise, varyNoiseScale, varyNoiseSpeed, varyTarget;
};
__device__ float vary(float base, float offset, float variance) { return base + (offset * variance * base); }
__device__ float4 %(entry)s(const %(pass)s &p)
{
    const Logic &u = th_uniforms<Logic>(p);
    const float4 st = p.self;
    if (!(st.x != -1000000.0f || st.y != -1000000.0f)) return st;
    const float fcx = (float)p.x + 0.5f, fcy = (float)p.y + 0.5f;
    const float i = (fcx + (fcy * p.dataRes.x)) / (p.dataRes.x * p.dataRes.y);
    const float sx = st.x * u.viewSize[0], sy = st.y * u.viewSize[1];
    const float4 ft = th_flow(p, 0.0f + (1.0f * (sx + 1.0f)) / 2.0f, 0.0f + (1.0f * (sy + 1.0f)) / 2.0f);
    const float k = fmaxf(0.0f, 1.0f - ((%(clock)s.time - ft.z) * u.flowDecay));
    const float ffx = (0.0f + ft.x * k * 1.0f) / 1.0f, ffy = (0.0f + ft.y * k * 1.0f) / 1.0f;
    const float force = vary(u.forceWeight, i, u.varyForce), flow = vary(u.flowWeight, i, u.varyFlow);
    float vx = (st.z * u.damping * %(clock)s.dt) + (force * (ffx * %(clock)s.dt * flow));
    float vy = (st.w * u.damping * %(clock)s.dt) + (force * (ffy * %(clock)s.dt * flow));
    const float speed = sqrtf(vx * vx + vy * vy);
    const float r = fminf(speed, u.speedLimit) / speed;
    vx *= r; vy *= r;
    return make_float4(st.x + vx, st.y + vy, vx, vy);
}
"""
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


class DriftU(C.Structure):
    _fields_ = [("dt", C.c_float)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--flow", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--packed", action="store_true", help="the packed-ring arm")
    ap.add_argument("--sizes", type=int, nargs="+", default=(4096, 16384))
    ap.add_argument("--against", default=None, help="the parent commit's libtendrils_hip.so: alternate it with this tree's")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.packed:
        return packed_compare(args) if args.against and not args.child else packed_arm(args)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("step_program_bench: no GPU - nothing is measured without one")
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import LOGIC, Particles, Program, StepProgram, run_pass
    from tendrils_amd.tendrils import defaults

    n, steps = args.size, args.steps
    fw, fh = args.flow
    time0, dt = 1000.0, 1000.0 / 60.0
    uniforms = {k: v for k, v in defaults()["state"].items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
    uniforms.update(noiseWeight=0, viewSize=(1.0, fh / fw), time=time0, dt=dt)
    rng = np.random.default_rng(5)
    flow = np.zeros((fh, fw, 4), np.float32)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (fh, fw, 2))
    flow[..., 2] = time0 - 10.0
    flow[..., 3] = 1.0

    programs = dict(
        drift=(StepProgram.from_source(STEP_DRIFT, name="drift"), Program.from_source(STATE_DRIFT, DriftU, name="state_drift")),
        flow_only=(StepProgram.from_source(FLOW_ONLY % dict(entry="th_step_main", **{"pass": "th_step_pass"}, clock="p"), _capi.LogicUniforms, name="flow_only"),
                   Program.from_source(FLOW_ONLY % dict(entry="th_main", **{"pass": "th_pass"}, clock="u"), _capi.LogicUniforms, name="state_flow_only")),
    )

    def context(fuse=None):
        p = Particles(None, dict(shape=[n, n]))
        p.setup(2)
        if fuse is not None:
            p.option("fuse", fuse)
        ball = _capi.SpawnBallUniforms(radius=0.8, speed=0.004)
        for k in (0, 1):
            call("th_spawn_ball", p._ctx, C.byref(ball), k)
        call("th_flow_resize", p._ctx, fw, fh)
        call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
        return p

    fused, single, state, builtin, keyed = context(), context(fuse=0), context(), context(), context()
    keyed.step_view_size(uniforms["viewSize"])
    contexts = (fused, single, state, builtin, keyed)

    # the process's one HIP runtime (the copy _capi.load() settled on), for the copy arm
    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream, dst, src = C.c_void_p(), C.c_void_p(), C.c_void_p()
    call("th_stream", state._ctx, C.byref(stream))
    call("th_state_device_ptr", state._ctx, 0, C.byref(dst))
    call("th_state_device_ptr", state._ctx, 1, C.byref(src))
    nbytes = n * n * 16

    def step_program(p, prog):
        def run():
            p.logic = prog
            p.step_n(dict(uniforms), time0, dt, steps)
        return run

    def state_program(p, prog):
        def run():
            t = time0
            for _ in range(steps):
                t += dt
                run_pass(p, prog, dict(uniforms, time=t, dt=dt), _capi.TH_TARGET_RING)
        return run

    def builtin_steps():
        builtin.logic = Program(LOGIC)
        builtin.step_n(dict(uniforms), time0, dt, steps)

    def copy():
        e = hip.hipMemcpyAsync(dst, src, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
        if e:
            raise RuntimeError("hipMemcpyAsync: error %d" % e)

    # (bytes through HBM per call as the arm is built, context whose stream times it, the call)
    arms = {}
    for name, (step_form, state_form) in programs.items():
        arms[name + " fused"] = (nbytes * (1 + 2 * ((steps + 31) // 32)), fused, step_program(fused, step_form))
        if name == "flow_only":         # (+ 4 B of perm per slot and launch; the periodic re-sort's move is inside the figure)
            arms[name + " fused sorted"] = ((3 * nbytes + nbytes // 4) * ((steps + 31) // 32), keyed, step_program(keyed, step_form))
        arms[name + " single"] = (2 * nbytes * steps, single, step_program(single, step_form))
        arms[name + " state_prog"] = (2 * nbytes * steps, state, state_program(state, state_form))
    arms["builtin th_step_n"] = (3 * nbytes, builtin, builtin_steps)
    arms["memcpy_d2d"] = (2 * nbytes, state, copy)

    def timed(p, fn, reps):
        ms = C.c_float(0)
        call("th_timer_start", p._ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", p._ctx, C.byref(ms))
        return ms.value / reps

    for _, p, fn in arms.values():
        timed(p, fn, args.warmup)
    rounds = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (_, p, fn) in arms.items():
            rounds[name].append(timed(p, fn, args.reps))

    lines = ["step programs, %d x %d particles, flow %d x %d, %d steps per call, %d rounds of %d calls, arms alternating; GPU ms per call (events on the context's stream)"
             % (n, n, fw, fh, steps, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "%-24s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    result = dict(size=n, flow=[fw, fh], steps=steps, reps=args.reps, rounds=args.rounds, arms={}, query={})
    for name, (moved, _, _) in arms.items():
        ms = rounds[name]
        med = statistics.median(ms)
        result["arms"][name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), bytes=moved, gbps=moved / med / 1e6)
        lines.append("%-24s %10.4f %10.4f %10.4f %14.1f" % (name, med, min(ms), max(ms), moved / med / 1e6))
    med = {k: v["median_ms"] for k, v in result["arms"].items()}
    for name in programs:
        a, b, c = (result["arms"]["%s %s" % (name, arm)] for arm in ("fused", "single", "state_prog"))
        lines.append("%s: fused / state_prog = %.3f (rounds apart: fused max %.4f < state_prog min %.4f: %s); fused / (1.5 x memcpy_d2d) = %.3f; "
                     "single / state_prog = %.3f (single median %.4f against state_prog max %.4f)"
                     % (name, a["median_ms"] / c["median_ms"], a["max_ms"], c["min_ms"], a["max_ms"] < c["min_ms"],
                        a["median_ms"] / (1.5 * med["memcpy_d2d"]), b["median_ms"] / c["median_ms"], b["median_ms"], c["max_ms"]))
    lines.append("flow_only fused / builtin th_step_n = %.3f" % (med["flow_only fused"] / med["builtin th_step_n"]))
    a, b = result["arms"]["flow_only fused sorted"], result["arms"]["flow_only fused"]
    info = _capi.SlotOrderInfo()
    call("th_slot_order", keyed._ctx, C.byref(info))
    lines.append("flow_only fused sorted / builtin th_step_n = %.3f; fused sorted / fused = %.3f (rounds apart: sorted max %.4f < texel-order min %.4f: %s); "
                 "the keyed context: %d sorted buffers, %d sorts"
                 % (a["median_ms"] / med["builtin th_step_n"], a["median_ms"] / b["median_ms"], a["max_ms"], b["min_ms"], a["max_ms"] < b["min_ms"],
                    info.sorted_buffers, info.sorts))
    for name, (step_form, state_form) in programs.items():
        result["query"][name] = dict(step=step_form.query(fused), state=state_form.query(state))
        lines.append("th_program_query(%s): th_step_kernel %s; th_program_kernel %s"
                     % (name, json.dumps(result["query"][name]["step"]), json.dumps(result["query"][name]["state"])))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    for p in contexts:
        p.dispose()
    for pair in programs.values():
        for prog in pair:
            prog.dispose()


class _Raw:
    """device memory as torch takes it (torch.as_tensor): n int16 values at ptr"""
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<i2", data=(ptr, False), version=2)


def packed_arm(args):
    """the packed arm on the library this process loads (TH_LIB, else this tree's): prints the lines, then one JSON line"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("step_program_bench: no GPU - nothing is measured without one")
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import Particles, StepProgram
    from tendrils_amd.tendrils import defaults

    steps = args.steps
    fw, fh = args.flow
    time0, dt = 1000.0, 1000.0 / 60.0
    uniforms = {k: v for k, v in defaults()["state"].items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
    uniforms.update(noiseWeight=0, viewSize=(1.0, fh / fw), time=time0, dt=dt)
    rng = np.random.default_rng(5)
    flow = np.zeros((fh, fw, 4), np.float32)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (fh, fw, 2))
    flow[..., 2] = time0 - 10.0
    flow[..., 3] = 1.0

    sources = dict(drift=(STEP_DRIFT, None),
                   flow_only=(FLOW_ONLY % dict(entry="th_step_main", **{"pass": "th_step_pass"}, clock="p"), _capi.LogicUniforms))
    programs, compile_s = {}, {}
    for name, (source, block) in sources.items():
        t0 = time.perf_counter()
        programs[name] = StepProgram.from_source(source, block, name=name) if block else StepProgram.from_source(source, name=name)
        compile_s[name] = time.perf_counter() - t0

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    lib = os.path.realpath(_capi.load()._name)
    if lib.startswith(os.path.realpath(ROOT) + os.sep):
        lib = os.path.relpath(lib, os.path.realpath(ROOT))
    result = dict(lib=lib, steps=steps, reps=args.reps, rounds=args.rounds, compile_s=compile_s, sizes={})
    lines = ["step programs on a packed ring (TH_STATE_F16), flow %d x %d, %d steps per call, %d rounds of %d calls, arms alternating; GPU ms per call"
             % (fw, fh, steps, args.rounds, args.reps),
             "library: %s   device: %s" % (result["lib"], torch.cuda.get_device_name(0)),
             "StepProgram.from_source wall time: " + ", ".join("%s %.3f s" % kv for kv in compile_s.items())]
    torch.cuda.init()
    for n in args.sizes:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        # two contexts (ring + spare, targets, flow: 8 B x 3 + 16 B per particle each), the staged path's two f32 staging
        # buffers (32 B per particle, on whichever contexts take it), the copy's 24 B per particle
        need = n * n * (2 * 40 + 2 * 32 + 24)
        if need > free0:
            lines.append("%d x %d: skipped - %.1f GB free, about %.1f GB needed" % (n, n, free0 / 1e9, need / 1e9))
            continue

        def context(fuse=None):
            p = Particles(None, dict(shape=[n, n], stateFormat=_capi.TH_STATE_F16))
            p.setup(2)
            if fuse is not None:
                p.option("fuse", fuse)
            # the packed texels themselves, written in place: positions in [-0.8, 0.8), velocities in +-0.004
            g = torch.Generator(device="cuda").manual_seed(7)
            for k in (0, 1):
                d = C.c_void_p()
                call("th_state_device_ptr", p._ctx, k, C.byref(d))
                texels = torch.as_tensor(_Raw(d.value, n * n * 4), device="cuda").view(n * n, 4)
                chunk = 1 << 24
                for at in range(0, n * n, chunk):
                    m = min(chunk, n * n - at)
                    texels[at:at + m, :2] = torch.randint(-13107, 13107, (m, 2), dtype=torch.int16, device="cuda", generator=g)
                    vel = (torch.rand((m, 2), device="cuda", generator=g) * 0.008 - 0.004).to(torch.float16)
                    texels[at:at + m, 2:] = vel.view(torch.int16)
                call("th_state_device_ptr", p._ctx, k, C.byref(d))      # (written through the address: handed out again)
            torch.cuda.synchronize()
            call("th_flow_resize", p._ctx, fw, fh)
            call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
            return p

        fused, single = context(), context(fuse=0)

        def step_program(p, prog):
            def run():
                p.logic = prog
                p.step_n(dict(uniforms), time0, dt, steps)
            return run

        def timed(p, fn, reps):
            ms = C.c_float(0)
            call("th_timer_start", p._ctx)
            for _ in range(reps):
                fn()
            call("th_timer_stop", p._ctx, C.byref(ms))
            return ms.value / reps

        arms = {}
        for name, prog in programs.items():
            arms[name + " fused"] = (fused, step_program(fused, prog))
            arms[name + " single"] = (single, step_program(single, prog))
        for p, fn in arms.values():
            timed(p, fn, args.warmup)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                             # (the fill's temporaries)
        took = free0 - torch.cuda.mem_get_info()[0]          # both contexts and whatever their calls allocated
        # launches per call, by the library's own count
        count = {}
        for name, (p, fn) in arms.items():
            ms, k = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing", p._ctx, 1)
            fn()
            call("th_kernel_timing_read", p._ctx, C.byref(ms), C.byref(k))
            call("th_kernel_timing", p._ctx, 0)
            count[name] = k.value
        stream = C.c_void_p()
        call("th_stream", fused._ctx, C.byref(stream))
        src, dst = (torch.empty(n * n * 12, dtype=torch.uint8, device="cuda") for _ in range(2))
        src.zero_(), dst.zero_()
        torch.cuda.synchronize()

        def copy():
            e = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n * n * 12, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
            if e:
                raise RuntimeError("hipMemcpyAsync: error %d" % e)
        arms["copy24"] = (fused, copy)
        timed(fused, copy, args.warmup)
        rounds = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, (p, fn) in arms.items():
                rounds[name].append(timed(p, fn, args.reps))
        out = dict(took_bytes=took, launches=count, arms={})
        lines.append("%d x %d particles: the process took %.3f GB of device memory for two contexts and their calls" % (n, n, took / 1e9))
        lines.append("%-24s %10s %10s %10s %10s" % ("arm", "median ms", "min ms", "max ms", "launches"))
        for name, ms in rounds.items():
            out["arms"][name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
            lines.append("%-24s %10.4f %10.4f %10.4f %10s" % (name, statistics.median(ms), min(ms), max(ms), count.get(name, "")))
        for name in programs:
            a, b, c = out["arms"][name + " fused"], out["arms"][name + " single"], out["arms"]["copy24"]
            lines.append("%s: fused / single = %.3f (rounds apart: fused max %.4f < single min %.4f: %s); fused / copy24 = %.3f"
                         % (name, a["median_ms"] / b["median_ms"], a["max_ms"], b["min_ms"], a["max_ms"] < b["min_ms"], a["median_ms"] / c["median_ms"]))
        result["sizes"][str(n)] = out
        del src, dst
        fused.dispose(), single.dispose()
        torch.cuda.empty_cache()
    result["query"] = {}
    probe = Particles(None, dict(shape=[64, 64], stateFormat=_capi.TH_STATE_F16))
    probe.setup(2)
    for name, prog in programs.items():
        result["query"][name] = prog.query(probe)
        lines.append("th_program_query(%s): th_step_kernel %s" % (name, json.dumps(result["query"][name])))
    probe.dispose()
    for prog in programs.values():
        prog.dispose()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out and not args.child:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    return result


def packed_compare(args):
    """the packed arm in child processes, the parent commit's library and this tree's alternating in one session"""
    here = os.path.join(ROOT, "tendrils_amd", "lib", "libtendrils_hip.so")
    builds = (("parent", os.path.abspath(args.against)), ("this", here))
    cmd = [sys.executable, os.path.abspath(__file__), "--packed", "--child", "--steps", str(args.steps), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--flow", *map(str, args.flow), "--sizes", *map(str, args.sizes)]
    text, results = [], {name: [] for name, _ in builds}
    for run in range(args.runs):
        for name, lib in builds:
            print("run %d, %s build (%s) ..." % (run + 1, name, lib), flush=True)
            r = subprocess.run(cmd, env=dict(os.environ, TH_LIB=lib), capture_output=True, text=True, cwd=ROOT, timeout=args.child_timeout)
            if r.returncode:
                sys.exit("step_program_bench: the %s build's run failed (exit %d), nothing more is started\n%s\n%s"
                         % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
            body = r.stdout.strip().splitlines()
            results[name].append(json.loads(body[-1]))
            text += ["--- %s build, run %d" % (name, run + 1)] + body[:-1]
    text.append("--- the fused call across the builds (median ms of each run; min - max over all rounds)")
    for n in map(str, args.sizes):
        if not all(n in r["sizes"] for rs in results.values() for r in rs):
            continue
        for arm in ("drift fused", "flow_only fused"):
            row = {}
            for name, rs in results.items():
                a = [r["sizes"][n]["arms"][arm] for r in rs]
                row[name] = ([x["median_ms"] for x in a], min(x["min_ms"] for x in a), max(x["max_ms"] for x in a))
            (pm, plo, phi), (tm, tlo, thi) = row["parent"], row["this"]
            text.append("%s^2 %-16s parent %s (%.4f - %.4f)   this %s (%.4f - %.4f)   parent / this = %.2f   rounds apart (this max < parent min): %s"
                        % (n, arm, " / ".join("%.4f" % v for v in pm), plo, phi, " / ".join("%.4f" % v for v in tm), tlo, thi,
                           statistics.median(pm) / statistics.median(tm), thi < plo))
        for name, rs in results.items():
            text.append("%s^2 device memory taken, %s build: %s GB" % (n, name, " / ".join("%.3f" % (r["sizes"][n]["took_bytes"] / 1e9) for r in rs)))
    for name, rs in results.items():
        text.append("StepProgram.from_source(flow_only), %s build: %s s" % (name, " / ".join("%.3f" % r["compile_s"]["flow_only"] for r in rs)))
    text = "\n".join(text)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
