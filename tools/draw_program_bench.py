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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
