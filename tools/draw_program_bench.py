"""GPU time of a draw() pass whose vertex stage is a caller's draw program (tendrils_amd/csrc/th_drawprog.hip,
th_draw_prelude.inc) against the library's own stage on the same pipeline, on one MI355X.

Arms, all in this process, on one context in the stream-ordered pipeline with reuse off (every pass counts, scans, emits, sorts
and blends for itself - what a program pass always does); 4096^2 particles a texel or two long on a 1920 x 1080 target:
  flow_builtin    th_flow_deposit: the library's flow stage inside the rasterising kernels
  flow_program    th_draw_program_run(TH_PASS_FLOW) with that stage written out as a program (tests/test_draw_program_build.py:
                  FLOW): the vertex kernel into the vertex buffer, then the same pipeline reading it
  view_builtin    th_view_draw (beside the four arms the comparison is made of: what flow_builtin is to flow_program)
  view_program    th_draw_program_run(TH_PASS_VIEW) with the view stage written out (tests/test_gpu_draw_program.py: VIEW)
  vertex_kernel   the vertex kernel of flow_program / view_program alone (th_kernel_timing: events around that launch), against
  d2d_copy        a device-to-device copy that moves the bytes the kernel must move - 32 B read + 64 B written a particle
Each pass figure is the GPU time per call between two events on the context's stream (th_timer_start / th_timer_stop around
--reps calls, after --warmup calls); the arms alternate for --rounds rounds and the median round is reported with the spread.
The programs' registers / scratch / code size (th_program_query) go out with the figures.

Usage: python tools/draw_program_bench.py [--root 4096] [--width 1920] [--height 1080] [--reps 10] [--warmup 2] [--rounds 5] [--out profiles/draw_program.txt]

--bins: program passes through the binned pipeline (th_bins.hip: the PROGRAM instantiations; th_draw_vertex_slots_kernel) against
the stream-ordered one, and - with --parent-lib, a libtendrils_hip.so built from the parent commit - against that build.  One fresh
process per library and round (TH_LIB chooses the library), the libraries alternating; the median round is reported with the spread.
Every process measures, on one context (4096^2 particles, the C3 state of benchlib, 1920 x 1080):
  (a) pass_*     a flow / a view program pass with the policy forced to stream / bins, ring in texel order, reuse off
  (b) loop_*     the frame loop tick(); step(); draw() over the shapes whose step runs over sorted slots - GPU ms per frame, step
                 and draw apart - with both stages as programs under `auto` and under `bins`, and the library's own stages beside
                 them (th_draw: both passes in one rasterisation; and th_flow_deposit + th_view_draw: two, as a program frame has)
                 --frames frames per arm, one arm after the other at the same frames of the wake in every process
  (c) vertex_*   the vertex kernel alone (th_kernel_timing) over sorted slots and in texel order, and the unpermute of one state
                 buffer (ensure_identity: what a stream-ordered program pass costs a sorted ring, twice)
Usage: python tools/draw_program_bench.py --bins [--parent-lib PATH] [--rounds 5] [--frames 20] [--out profiles/...]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the restated stages are the tests' (one copy)


def bins_child(args):
    """one process, one library (TH_LIB): a JSON line of GPU ms per arm"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("draw_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import DrawProgram
    from tendrils_amd.tendrils import View
    from test_draw_program_build import FLOW
    from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms

    n, w, h = args.root, args.width, args.height
    workload.N = n
    flow, view = DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"), DrawProgram.from_source(VIEW, ViewUniforms, "view_stage")
    t = ta.Tendrils(View(w, h))
    t.resize()
    t.setup(n)
    p, ctx = t.particles, t.particles._ctx
    p.upload_texels(workload.synth_state(0))
    t.timer.time = 1000.0
    t.line_widths()
    out, ms = {}, C.c_float(0)
    info, order = _capi.DrawInfo(), _capi.SlotOrderInfo()

    def timed(fn, reps=1):
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        return ms.value / reps

    def kernel_timed(fn, reps):
        """(GPU ms per call, mean ms of the vertex kernel alone)"""
        mean, launches = C.c_float(0), C.c_int32(0)
        call("th_kernel_timing", ctx, 1)
        per_call = timed(fn, reps)
        call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
        call("th_kernel_timing", ctx, 0)
        assert launches.value == reps, (launches.value, reps)
        return per_call, mean.value

    def uniforms():
        return dict(t.state, time=float(t.timer.time), viewSize=t.viewSize, sinTerm=t.render_uniforms().sinTerm)

    # (b) the frame loops.  One arm after the other, the library's own stages first: a stream-ordered pass holds the ring in texel
    # order for rebucket_steps (256) frames afterwards, so an arm that takes that path comes after the arms that must not inherit
    # it.  Every library runs the arms at the same frames of the same wake; the rounds alternate the libraries.
    def both_passes():
        t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"])
        u, count = t.render_uniforms(), C.c_uint64(0)
        call("th_view_draw", ctx, C.byref(u), C.byref(count))

    def loop(name, policy, fs, rs, draw=None):
        q = dict(step=[], draw=[], sorted=[], pipeline=[])
        p.draw_pipeline(policy)
        t.flowShader, t.renderShader = fs, rs
        for k in range(3 + args.frames):              # (three frames for the pipeline to settle after the arm before)
            t.timer.tick()
            t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
            step = timed(t.step)
            ms_draw = timed(draw or t.draw)
            if k >= 3:
                call("th_draw_query", ctx, C.byref(info))
                call("th_slot_order", ctx, C.byref(order))
                q["step"].append(step); q["draw"].append(ms_draw)
                q["sorted"].append(order.sorted_buffers); q["pipeline"].append(info.pipeline)
        out[name + "_step"], out[name + "_draw"] = float(np.mean(q["step"])), float(np.mean(q["draw"]))
        out[name] = out[name + "_step"] + out[name + "_draw"]
        out["sorted_" + name] = float(np.mean(q["sorted"]))
        out["pipeline_" + name] = float(np.mean(q["pipeline"]))

    t.renderView = True
    loop("loop_builtin_th_draw", "auto", None, None)
    loop("loop_builtin_two_passes", "auto", None, None, both_passes)
    loop("loop_programs_bins", "bins", flow, view)

    # (c) the vertex kernel over sorted slots; the unpermute it spares
    p.draw_pipeline("bins")
    t.flowShader = t.renderShader = None
    t.timer.tick(); t.step(); t.draw()
    call("th_slot_order", ctx, C.byref(order))
    out["sorted_before_vertex_slots"] = order.sorted_buffers
    for name, prog, which in (("flow", flow, _capi.TH_PASS_FLOW), ("view", view, _capi.TH_PASS_VIEW)):
        run = lambda: t._draw_program(prog, which, uniforms())
        timed(run, args.warmup)
        _, out["vertex_slots_%s" % name] = kernel_timed(run, args.reps)
    call("th_slot_order", ctx, C.byref(order))
    out["sorted_after_vertex_slots"] = order.sorted_buffers
    unpermute, ptr = [], C.c_void_p()
    for _ in range(args.reps):
        t.timer.tick(); t.step(); t.draw()
        call("th_slot_order", ctx, C.byref(order))
        if order.sorted_buffers:
            unpermute.append(timed(lambda: call("th_state_device_ptr", ctx, 0, C.byref(ptr))) / order.sorted_buffers)
    out["unpermute_one_buffer"] = float(np.mean(unpermute)) if unpermute else None
    loop("loop_programs_auto", "auto", flow, view)
    t.flowShader = t.renderShader = None

    # (a) single passes, ring in texel order (one tick + step first: the C3 state a step apart, as the loop draws it)
    p.option("bucket", 0)
    t.timer.tick()
    t.step()
    p.option("draw_reuse", 0)
    for policy in ("stream", "bins"):
        p.draw_pipeline(policy)
        for name, prog, which in (("flow", flow, _capi.TH_PASS_FLOW), ("view", view, _capi.TH_PASS_VIEW)):
            run = lambda: t._draw_program(prog, which, uniforms())
            timed(run, args.warmup)
            out["pass_%s_%s" % (name, policy)], kernel = kernel_timed(run, args.reps)
            call("th_draw_query", ctx, C.byref(info))
            out["pipeline_pass_%s_%s" % (name, policy)] = info.pipeline
            if policy == "stream":
                out["vertex_texels_%s" % name] = kernel

    out["query"] = dict(flow=flow.query(p), view=view.query(p))
    out["device"] = torch.cuda.get_device_name(0)
    print("BINS_CHILD " + json.dumps(out))
    t.dispose()
    flow.dispose(), view.dispose()


def bins_main(args):
    """the driver: no GPU in this process; one child per library and round"""
    import subprocess
    libs = [("this", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    rounds = {name: [] for name, _ in libs}
    for r in range(args.rounds):
        for name, lib in (libs if r % 2 == 0 else libs[::-1]):
            env = dict(os.environ)
            if lib:
                env["TH_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--bins-child"] + [a for a in sys.argv[1:] if a != "--bins"]
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("BINS_CHILD ")]
            if done.returncode != 0 or not line:          # (a child that failed: nothing more is started on the GPU)
                sys.exit("draw_program_bench: the %s child of round %d failed (%d)\n%s\n%s" % (name, r, done.returncode, done.stdout[-2000:], done.stderr[-4000:]))
            rounds[name].append(json.loads(line[0][len("BINS_CHILD "):]))
            print("round %d %s: %s" % (r, name, line[0][len("BINS_CHILD "):]), flush=True)
    lines = ["draw programs through the bins: %d^2 particles into %d x %d; %d rounds (one process per library and round, alternating), GPU ms (events on the context's stream)"
             % (args.root, args.width, args.height, args.rounds),
             "device: %s" % rounds["this"][0]["device"],
             "loops: %d frames per arm after 3, one arm after the other; passes and kernels: %d calls after %d" % (args.frames, args.reps, args.warmup),
             "%-34s %-7s %10s %10s %10s" % ("figure", "library", "median", "min", "max")]
    keys = [k for k in rounds["this"][0] if k not in ("query", "device")]
    for k in keys:
        for name, _ in libs:
            v = [q[k] for q in rounds[name] if q.get(k) is not None]
            if v:
                lines.append("%-34s %-7s %10.4f %10.4f %10.4f" % (k, name, statistics.median(v), min(v), max(v)))
    lines.append("th_program_query: %s" % json.dumps(rounds["this"][0]["query"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bins", action="store_true")
    ap.add_argument("--bins-child", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.bins_child:
        return bins_child(args)
    if args.bins:
        return bins_main(args)

    import torch
    if not torch.cuda.is_available():
        sys.exit("draw_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import DrawProgram
    from tendrils_amd.sharding import device_view
    from tendrils_amd.tendrils import View
    from test_draw_program_build import FLOW
    from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms

    n, w, h = args.root, args.width, args.height
    programs = dict(flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"), view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"))
    t = ta.Tendrils(View(w, h))
    t.resize()
    t.setup(n)
    t.state["speedAlpha"] = 0.5
    p = t.particles
    ctx = p._ctx
    p.draw_pipeline("stream")
    p.option("draw_reuse", 0)
    # particles all over the view, each a texel or two from where it was a step ago
    gen = torch.Generator(device="cuda").manual_seed(4096)
    prev = torch.empty((n * n, 4), dtype=torch.float32, device="cuda")
    prev[:, 0] = torch.rand(n * n, generator=gen, device="cuda") * 2 - 1
    prev[:, 1] = (torch.rand(n * n, generator=gen, device="cuda") * 2 - 1) * (h / w)
    prev[:, 2:] = (torch.rand((n * n, 2), generator=gen, device="cuda") * 2 - 1) * 0.01
    cur = prev.clone()
    cur[:, :2] += (torch.rand((n * n, 2), generator=gen, device="cuda") * 2 - 1) * 0.0015
    for index, state in ((0, cur), (1, prev)):
        ptr = C.c_void_p()
        call("th_state_device_ptr", ctx, index, C.byref(ptr))
        call("th_sync", ctx)
        device_view(ptr.value, (n * n, 4), "<f4").copy_(state)
    torch.cuda.synchronize()
    del cur, prev
    t.timer.time = 1000.0
    t.line_widths()

    uniforms = dict(t.state, time=float(t.timer.time), viewSize=t.viewSize, sinTerm=t.render_uniforms().sinTerm)
    blocks = {name: prog.pack(uniforms) for name, prog in programs.items()}
    d = _capi.DepositUniforms(time=float(t.timer.time), speedLimit=float(t.state["speedLimit"]))
    d.viewSize[0], d.viewSize[1] = float(t.viewSize[0]), float(t.viewSize[1])
    r = t.render_uniforms()
    frags = {}

    def program_pass(name, which):
        def run():
            count = C.c_uint64(0)
            call("th_draw_program_run", ctx, programs[name].handle, C.byref(blocks[name]), C.sizeof(blocks[name]), which, C.byref(count))
            frags[name + "_program"] = count.value
        return run

    def builtin_pass(entry, u, name):
        def run():
            count = C.c_uint64(0)
            call(entry, ctx, C.byref(u), C.byref(count))
            frags[name] = count.value
        return run

    arms = {
        "flow_builtin": builtin_pass("th_flow_deposit", d, "flow_builtin"),
        "flow_program": program_pass("flow", _capi.TH_PASS_FLOW),
        "view_builtin": builtin_pass("th_view_draw", r, "view_builtin"),
        "view_program": program_pass("view", _capi.TH_PASS_VIEW),
    }
    kernel_of = {"flow_program": "vertex_kernel(flow)", "view_program": "vertex_kernel(view)"}

    def timed(name, fn, reps):
        """(GPU ms per call, mean ms of the vertex kernel alone or None)"""
        ms, kernel = C.c_float(0), None
        if name in kernel_of:
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if name in kernel_of:
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)
            kernel = mean.value
        return ms.value / reps, kernel

    # the copy: 48 B a particle read and written = the 96 B a particle the vertex kernel moves (torch's stream, its own events)
    src = torch.empty(n * n * 48, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy_ms(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for name, fn in arms.items():
        timed(name, fn, args.warmup)
    copy_ms(args.warmup)
    rounds = {name: [] for name in list(arms) + list(kernel_of.values()) + ["d2d_copy"]}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ms, kernel = timed(name, fn, args.reps)
            rounds[name].append(ms)
            if kernel is not None:
                rounds[kernel_of[name]].append(kernel)
        rounds["d2d_copy"].append(copy_ms(args.reps))

    queries = {name: prog.query(p) for name, prog in programs.items()}
    moved = 96 * n * n
    lines = ["draw program passes, %d^2 particles into %d x %d, stream-ordered pipeline, reuse off; %d rounds of %d calls, arms alternating; GPU ms per call (events on the stream)"
             % (n, w, h, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "fragments per pass: %s" % json.dumps(frags, sort_keys=True),
             "%-20s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    result = dict(root=n, width=w, height=h, reps=args.reps, rounds=args.rounds, query=queries, fragments=frags, arms={})
    for name, ms in rounds.items():
        med = statistics.median(ms)
        bandwidth = moved / med / 1e6 if name.startswith("vertex_kernel") or name == "d2d_copy" else None
        result["arms"][name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), gbps=bandwidth)
        lines.append("%-20s %10.4f %10.4f %10.4f %14s" % (name, med, min(ms), max(ms), "-" if bandwidth is None else "%.1f" % bandwidth))
    med = {name: v["median_ms"] for name, v in result["arms"].items()}
    lines.append("flow_program / flow_builtin = %.3f;  view_program / flow_builtin = %.3f;  view_program / view_builtin = %.3f  (time ratios)"
                 % (med["flow_program"] / med["flow_builtin"], med["view_program"] / med["flow_builtin"], med["view_program"] / med["view_builtin"]))
    lines.append("vertex_kernel(flow) / d2d_copy = %.3f;  vertex_kernel(view) / d2d_copy = %.3f  (time ratios; %d B a particle either way)"
                 % (med["vertex_kernel(flow)"] / med["d2d_copy"], med["vertex_kernel(view)"] / med["d2d_copy"], 96))
    lines.append("vertex buffer: %.0f MiB (64 B a particle)" % (64 * n * n / 2 ** 20))
    for name, info in queries.items():
        lines.append("th_program_query(%s): %s" % (name, json.dumps(info)))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    t.dispose()
    for prog in programs.values():
        prog.dispose()


if __name__ == "__main__":
    main()
