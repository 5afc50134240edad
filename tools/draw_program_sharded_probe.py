"""Draw programs on a row band at world size 1 (all a 1-GPU box allows) against the local program pass, on one MI355X: what
th_draw_program_sharded - the library's own exchange over its RCCL communicator, with nobody to exchange with - costs beside
th_draw_program_run under TH_DRAW_STREAM, and th_draw_vertex_band_kernel beside th_draw_vertex_kernel at the same shape.

Two contexts in this process hold the same state (4096^2 particles of benchlib's C3 state, two steps on; 1920 x 1080; ring in
texel order, reuse off), the library's two stages written out as programs (tests: FLOW, VIEW):
  run_flow, run_view   th_draw_program_run(TH_PASS_FLOW / TH_PASS_VIEW), policy `stream`, on the local context
  sharded_both         th_draw_program_sharded with both programs on the context that joined a communicator of one rank: both
                       passes, each emit -> counts -> (nothing to send) -> merge -> all-gather of the one owner's range
  emit_flow, emit_view th_draw_program_emit alone on that context (the whole texture is the band of all rows): no merge
  vertex(*), band(*)   the vertex kernel alone (th_kernel_timing: events around that launch) inside run_* / emit_*
Each figure is GPU ms per call between two events on the context's stream (th_timer_start / th_timer_stop around --reps calls,
after --warmup calls); the arms alternate for --rounds rounds; median, min and max of the rounds are written.  Nothing is gated.

Usage: python tools/draw_program_sharded_probe.py [--root 4096] [--width 1920] [--height 1080] [--reps 10] [--warmup 2] [--rounds 5] [--out FILE]
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
        sys.exit("draw_program_sharded_probe: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi, sharding
    from tendrils_amd._capi import call
    from tendrils_amd.particles import DrawProgram
    from tendrils_amd.tendrils import View
    from test_draw_program_build import FLOW
    from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms

    n, w, h = args.root, args.width, args.height
    workload.N = n
    programs = dict(flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"), view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"))

    def context(joined):
        t = ta.Tendrils(View(w, h))
        t.resize()
        t.setup(n)
        p = t.particles
        p.option("bucket", 0)                              # the ring stays in texel order
        p.option("draw_reuse", 0)
        p.draw_pipeline("stream")
        p.upload_texels(workload.synth_state(0))
        t.timer.time = 1000.0
        for _ in range(2):                                 # buffers[0] and [1] a step apart, as a frame loop draws them
            t.timer.tick()
            t.step()
        t.line_widths()
        t._bind_view(None)
        if joined:
            ident = (C.c_ubyte * _capi.COMM_ID_BYTES).from_buffer_copy(sharding.comm_id())
            call("th_comm_init", p._ctx, ident, 0, 1)
        return t

    local, band = context(False), context(True)
    uniforms = dict(local.draw_program_uniforms(), sinTerm=local.render_uniforms().sinTerm)
    blocks = {name: prog.pack(uniforms) for name, prog in programs.items()}
    d = _capi.DepositUniforms(time=float(local.timer.time), speedLimit=float(local.state["speedLimit"]))
    d.viewSize[0], d.viewSize[1] = float(local.viewSize[0]), float(local.viewSize[1])
    frags = {}

    def block(name):
        return programs[name].handle, C.byref(blocks[name]), C.sizeof(blocks[name])

    def run(name, which):
        def go():
            count = C.c_uint64(0)
            call("th_draw_program_run", local.particles._ctx, *block(name), which, C.byref(count))
            frags["run_" + name] = count.value
        return go

    def emit(name, which):
        def go():
            count, kp, cp = C.c_uint64(0), C.c_void_p(), C.c_void_p()
            call("th_draw_program_emit", band.particles._ctx, *block(name), which, C.byref(count), C.byref(kp), C.byref(cp))
            frags["emit_" + name] = count.value
        return go

    def sharded_both():
        a, b = C.c_uint64(0), C.c_uint64(0)
        call("th_draw_program_sharded", band.particles._ctx, *block("flow"), None, *block("view"), None, C.byref(a), C.byref(b))
        frags["sharded_flow"], frags["sharded_view"] = a.value, b.value

    arms = {"run_flow": (local, run("flow", _capi.TH_PASS_FLOW), "vertex(flow)"), "run_view": (local, run("view", _capi.TH_PASS_VIEW), "vertex(view)"),
            "sharded_both": (band, sharded_both, None),
            "emit_flow": (band, emit("flow", _capi.TH_PASS_FLOW), "band(flow)"), "emit_view": (band, emit("view", _capi.TH_PASS_VIEW), "band(view)")}

    def timed(t, fn, reps, kernel):
        """(GPU ms per call, mean ms of the vertex kernel alone or None)"""
        ctx, ms, alone = t.particles._ctx, C.c_float(0), None
        if kernel:
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if kernel:
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)
            alone = mean.value
        return ms.value / reps, alone

    # the same passes leave the same targets: one flow and one view pass each way from the same start, compared on the bits
    run("flow", _capi.TH_PASS_FLOW)()
    run("view", _capi.TH_PASS_VIEW)()
    sharded_both()
    same = bool((sharding.flow_view(local).view(torch.int32) == sharding.flow_view(band).view(torch.int32)).all()) and \
        bool((sharding.view_view(local) == sharding.view_view(band)).all())
    if not same or frags["run_flow"] != frags["sharded_flow"] or frags["run_view"] != frags["sharded_view"]:
        sys.exit("draw_program_sharded_probe: the sharded call and the local passes disagree (%s): nothing is timed" % json.dumps(frags))

    for name, (t, fn, kernel) in arms.items():
        timed(t, fn, args.warmup, kernel)
    rounds = {name: [] for name in list(arms) + [k for _, _, k in arms.values() if k]}
    for _ in range(args.rounds):
        for name, (t, fn, kernel) in arms.items():
            ms, alone = timed(t, fn, args.reps, kernel)
            rounds[name].append(ms)
            if kernel:
                rounds[kernel].append(alone)

    moved = 96 * n * n                                     # 32 B of state read + 64 B of records written a particle, either kernel
    lines = ["draw programs on a row band, world of one: %d^2 particles into %d x %d, stream-ordered, reuse off; %d rounds of %d calls, arms alternating; GPU ms per call (events on the stream)"
             % (n, w, h, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "targets after one flow and one view pass each way: equal on the bits; fragments per pass: %s" % json.dumps(frags, sort_keys=True),
             "%-16s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    med = {}
    for name, ms in rounds.items():
        med[name] = statistics.median(ms)
        alone = name.startswith(("vertex(", "band("))
        lines.append("%-16s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), "%.1f" % (moved / med[name] / 1e6) if alone else "-"))
    lines.append("sharded_both / (run_flow + run_view) = %.3f;  band(flow) / vertex(flow) = %.3f;  band(view) / vertex(view) = %.3f  (time ratios of the medians)"
                 % (med["sharded_both"] / (med["run_flow"] + med["run_view"]), med["band(flow)"] / med["vertex(flow)"], med["band(view)"] / med["vertex(view)"]))
    for name, prog in programs.items():
        lines.append("th_program_query(%s) - of th_draw_vertex_kernel: %s" % (name, json.dumps(prog.query(local.particles))))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in (local, band):
        t.dispose()
    for prog in programs.values():
        prog.dispose()


if __name__ == "__main__":
    main()
