"""GPU time of a draw() pass with a caller's fragment stage (tendrils_amd/csrc/th_fragprog.hip, th_fragment_prelude.inc) against
the same pass without it, and of the fragment kernel alone against a copy of the bytes it moves, on one MI355X.

One process, one context: 4096^2 particles in the C3 state of benchlib after a few steps (every line a texel or two long) on a
1920 x 1080 target, the stream-ordered pipeline with reuse off on every arm (a pass with a fragment stage never reuses).  Arms,
all the flow pass with the library's vertex stage:
  plain       th_flow_deposit
  identity    th_draw_stages_run with `return f.color` - the compiler proves the store writes what the load read and drops both:
              the kernel of this program is empty, and the arm shows what the stage costs a pass beside its kernel (the launch)
  gain        ... with `color * uniform`: the 16-byte load and the 16-byte store, no use of x, y - the key load is dropped
  stripe      ... with `color * ((x + 3 y) & 1 ? uniform : 1)`: the key load and the split into x, y beside them, no tap - what the
              split costs shows against gain and against the copy of its 36 bytes
  vignette    ... with the program of the tests (tests/test_fragment_program_build.py: VIGNETTE): key, x and y, a colour-map tap
The kernel alone is th_kernel_timing's event pair around its launch; copy(N) is a device-to-device copy that reads and writes N
bytes a fragment in all (32: what gain's kernel moves; 36: vignette's, beside its taps of a map that stays in cache).
Each pass figure is GPU ms per call between two events on the context's stream around --reps calls, after --warmup calls; the arms
alternate for --rounds rounds and the median round is reported with the spread.  th_program_query's registers / scratch / code
size go out with the figures.

--bins: the stage through the binned pipeline (TH_OPT_STAGE_BINS, th_fragment_bins_kernel) instead.  Five contexts in the same
state run the frame loop - tick(); step(); draw() - side by side, policy auto:
  loop(off)      flowShader = renderShader = (None, vignette), option off: both passes stream-ordered, the ring in texel order
  loop(on)       the same shaders, option on: both passes through the bins, the ring in its tile-sorted slots
  loop(identity, off) / loop(identity, on)  the same pair with `return f.color` in both passes: the stage changes nothing, so these
                 loops draw what loop(builtin) draws, frame for frame (a vignette in the flow pass changes the field the particles
                 follow: those loops go their own way, and within a few dozen frames nearly all their fragments lie in crowded bins)
  loop(builtin)  no shaders: the library's own binned frame loop (one rasterisation for both passes), beside both
Each figure is wall ms per frame around --reps frames that end in a synchronise, after --warmup-frames frames; the arms alternate
for --rounds rounds (every context has then run the same number of frames) and the median round is reported.  Then, on the
loop(on) context, the flow pass alone: th_draw_stages_run with `gain` and with the vignette through the bins - the pass between
two events, and th_kernel_timing's pair around th_fragment_bins_kernel - against copy(40): a device-to-device copy that moves
40 bytes a fragment in all, what the kernel moves (an 8-byte key and 16 bytes read, 16 bytes written).

--line: a stage that reads the fragment's line (th_line(f); th_fragline.hip, th_fragment_line_kernel).  One context in the state of
the figures without --bins, the flow pass stream-ordered, reuse off; --line-width W draws it W texels wide (a GL that honours
gl.lineWidth; 1: the reference's captured GL).  Arms:
  plain       th_flow_deposit
  vignette    th_draw_stages_run with the tests' VIGNETTE: it does not name th_line and launches what it always did
  falloff     ... with alpha scaled by fmaxf(1 - fabsf(th_line(f).across) / half_width, 0) (the reference's @todo in src/flow/index.frag;
              tests/test_fragment_program_line_build.py: FALLOFF): the line kernel behind the scatter, then th_fragment_line_kernel
kernel(...) is th_kernel_timing's pair around the stage's kernel alone - the line kernel is not inside it.  copy(36) moves what the
vignette kernel moves, copy(48) what th_fragment_line_kernel moves (a 16-byte record and the varying read, the varying written), and
copy(lines) what the line kernel moves: 16 bytes written and one key read a fragment, two state texels, `count` and `offset` a line.
The line kernel's own time is a kernel trace's to give (fragment_lines_kernel, fragment_lines_long_kernel beside deposit_emit_kernel):
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fragment_program_bench.py --line --rounds 1 --reps 5
pass(falloff) - pass(vignette) - (kernel(falloff) - kernel(vignette)) is the same figure from the events, and is printed.

--line --bins: such a stage through the binned pipeline (TH_OPT_LINE_BINS beside TH_OPT_STAGE_BINS; th_fragline.hip:
fragment_line_ends_kernel, fragment_lines_bins_kernel; th_fragment_line_bins_kernel).  Four contexts in the same state run the frame
loop side by side, stage_bins = 1 in all of them, policy auto (--line-width above 2: policy bins - the auto policy leaves wide lines
to the stream-ordered pipeline):
  loop(falloff, off)  flowShader = (None, falloff), line_bins off: the flow pass stream-ordered, the ring pulled to texel order
  loop(falloff, on)   the same shader, line_bins on: the flow pass through the bins, the ring in its tile-sorted slots
  loop(identity)      flowShader = (None, `return f.color`): a stage that does not read the line, through the bins
  loop(builtin)       no shaders
(the falloff changes the field the particles follow: its two loops draw the same frames as each other, not as the other two.)
Then, on a context three steps in with policy bins, the flow pass alone: th_flow_deposit, th_draw_stages_run with `gain` (the bins
kernel, no line) and with the falloff (the two line kernels, then th_fragment_line_bins_kernel) - the pass between two events and
th_kernel_timing's pair around the stage's kernel.  The two line kernels together, from the events:
pass(falloff) - pass(gain) - (kernel(falloff) - kernel(gain)); each alone is a kernel trace's to give, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fragment_program_bench.py --line --bins --rounds 1 --reps 5 --warmup-frames 2
copy(ends) moves what fragment_line_ends_kernel moves (two 16-byte state texels read and 16 bytes written a line), copy(records)
what fragment_lines_bins_kernel moves (an 8-byte key and 16 bytes of endpoints read, 16 bytes written a fragment), copy(56) what
th_fragment_line_bins_kernel moves (key, record and varying read, the varying written).

--pair [--bins]: both passes' stages over ONE rasterisation (th_draw_stages_pair, Tendrils.pairedStages; th_fragment_pair_kernel /
th_fragment_pair_bins_kernel).  Seven contexts in the same state run the frame loop side by side, policy auto, stage_bins off
(--bins: on) in all of them:
  loop(identity, off) / loop(identity, on)   flowShader = renderShader = (None, `return f.color`), pairedStages off / on
  loop(vignette, off) / loop(vignette, on)   ... the tests' VIGNETTE in both passes
  loop(vignette, flow alone, off) / (.., on) flowShader = (None, vignette) and no renderShader
  loop(builtin)                              no shaders: th_draw's one rasterisation
An off arm issues the calls draw() has always issued - two stage passes, two rasterisations - through code this call does not touch:
it is what the parent commit runs (--arms off,builtin runs on a commit without the call).  After the last frame the flow field and
the view of every on / off pair are compared bit for bit.  Then, on a context three steps in, each pair kernel alone -
th_kernel_timing's pair around the one launch of a th_draw_stages_pair with the program in the view slot - against copy(36) (--bins:
copy(40)): a device-to-device copy of the bytes the kernel moves a fragment - the key (4 bytes; 8 in the page store), 16 bytes read,
16 written.

Usage: python tools/fragment_program_bench.py [--bins | --line [--bins] [--line-width 1] | --pair [--bins] [--arms off,on,builtin]] [--root 4096] [--width 1920] [--height 1080] [--reps 10] [--warmup 2] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the test programs are the tests' (one copy)

GAIN = """struct GainUniforms { float gain; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const float g = th_uniforms<GainUniforms>(f).gain;
    return make_float4(f.color.x * g, f.color.y * g, f.color.z, f.color.w * g);
}
"""

STRIPE = """struct GainUniforms { float gain; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const float g = ((f.x + 3u * f.y) & 1u) ? th_uniforms<GainUniforms>(f).gain : 1.0f;
    return make_float4(f.color.x * g, f.color.y * g, f.color.z, f.color.w * g);
}
"""


class GainUniforms(C.Structure):
    _fields_ = [("gain", C.c_float)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bins", action="store_true", help="the stage through the binned pipeline: frame loops with the option off / on, the bins kernel alone")
    ap.add_argument("--warmup-frames", type=int, default=12, help="--bins: frames every loop runs before anything is timed")
    ap.add_argument("--line", action="store_true", help="a stage that reads the fragment's line: the pass, the stage's kernel, the copies of what it and the line kernel move")
    ap.add_argument("--line-width", type=float, default=1.0, help="--line: the width the flow pass is drawn with")
    ap.add_argument("--pair", action="store_true", help="both passes' stages over one rasterisation: frame loops with Tendrils.pairedStages off / on, each pair kernel alone (--bins: stage_bins on)")
    ap.add_argument("--arms", default="off,on,builtin", help="--pair: the loops to run (off,builtin: what a commit without the call can run)")
    args = ap.parse_args()
    if args.pair:
        return pair_main(args)
    if args.bins and args.line:
        return line_bins_main(args)
    if args.bins:
        return bins_main(args)
    if args.line:
        return line_main(args)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fragment_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd._capi import call
    from tendrils_amd.particles import FragmentProgram, draw_stages
    from tendrils_amd.tendrils import View
    from test_fragment_program_build import IDENTITY, VIGNETTE, FragUniforms

    n, w, h = args.root, args.width, args.height
    workload.N = n
    programs = dict(identity=FragmentProgram.from_source(IDENTITY, name="identity"),
                    gain=FragmentProgram.from_source(GAIN, GainUniforms, "gain"),
                    stripe=FragmentProgram.from_source(STRIPE, GainUniforms, "stripe"),
                    vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"))
    t = ta.Tendrils(View(w, h))
    t.resize()
    t.setup(n)
    p, ctx = t.particles, t.particles._ctx
    p.upload_texels(workload.synth_state(0))
    t.colorMap.set_pixels(np.random.default_rng(7).uniform(0, 1, (64, 64, 4)).astype(np.float32))
    t.timer.time = 1000.0
    for _ in range(3):                               # the C3 state a few frames in: buffers[1] -> buffers[0] are the lines
        t.timer.tick()
        t.step()
    p.draw_pipeline("stream")
    p.option("draw_reuse", 0)
    t.line_widths()
    uniforms = dict(t.state, gain=0.5, tint=[0.5, 0.25, 0.75, 0.875], invRes=[1.0 / w, 1.0 / h], edge=3.5 / (w * w + h * h))
    d = t.deposit_uniforms()
    held = {name: draw_stages(None, prog, uniforms, d) for name, prog in programs.items()}
    frags = {}

    def plain():
        count = C.c_uint64(0)
        call("th_flow_deposit", ctx, C.byref(d), C.byref(count))
        frags["plain"] = count.value

    def staged(name):
        def run():
            count = C.c_uint64(0)
            call("th_draw_stages_run", ctx, C.byref(held[name][0]), 0, C.byref(count))
            frags[name] = count.value
        return run

    arms = dict(plain=plain, identity=staged("identity"), gain=staged("gain"), stripe=staged("stripe"), vignette=staged("vignette"))

    def timed(name, fn, reps):
        """(GPU ms per call, mean ms of the fragment kernel alone or None)"""
        ms, kernel = C.c_float(0), None
        if name != "plain":
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if name != "plain":
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)
            kernel = mean.value
        return ms.value / reps, kernel

    for name, fn in arms.items():
        timed(name, fn, args.warmup)
    total = frags["plain"]
    assert all(v == total for v in frags.values()), frags
    copies = {}
    for moved in (32, 36):                           # half read, half written (torch's stream, its own events)
        src = torch.empty(total * moved // 2, dtype=torch.uint8, device="cuda")
        copies[moved] = (src, torch.empty_like(src))

    def copy_ms(moved, reps):
        src, dst = copies[moved]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for moved in copies:
        copy_ms(moved, args.warmup)
    rounds = {}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ms, kernel = timed(name, fn, args.reps)
            rounds.setdefault("pass(%s)" % name, []).append(ms)
            if kernel is not None:
                rounds.setdefault("kernel(%s)" % name, []).append(kernel)
        for moved in copies:
            rounds.setdefault("copy(%d)" % moved, []).append(copy_ms(moved, args.reps))

    queries = {name: prog.query(p) for name, prog in programs.items()}
    bytes_of = {"kernel(gain)": 32, "kernel(stripe)": 36, "kernel(vignette)": 36, "copy(32)": 32, "copy(36)": 36}
    lines = ["fragment stage in the flow pass, %d^2 particles (C3 state, 3 steps in) into %d x %d, stream-ordered pipeline, reuse off; "
             "%d rounds of %d calls, arms alternating; GPU ms per call (events on the stream)" % (n, w, h, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "fragments per pass: %d" % total,
             "%-20s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    med = {}
    for name, ms in rounds.items():
        med[name] = statistics.median(ms)
        gbps = "%.1f" % (bytes_of[name] * total / med[name] / 1e6) if name in bytes_of else "-"
        lines.append("%-20s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), gbps))
    lines.append("pass(identity) / pass(plain) = %.3f;  pass(gain) / pass(plain) = %.3f;  pass(stripe) / pass(plain) = %.3f;  pass(vignette) / pass(plain) = %.3f  (time ratios)"
                 % tuple(med["pass(%s)" % k] / med["pass(plain)"] for k in ("identity", "gain", "stripe", "vignette")))
    lines.append("kernel(gain) / copy(32) = %.3f;  kernel(stripe) / copy(36) = %.3f;  kernel(vignette) / copy(36) = %.3f  (time ratios, the same bytes a fragment)"
                 % (med["kernel(gain)"] / med["copy(32)"], med["kernel(stripe)"] / med["copy(36)"], med["kernel(vignette)"] / med["copy(36)"]))
    for name, info in queries.items():
        lines.append("th_program_query(%s): %s" % (name, json.dumps(info)))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(root=n, width=w, height=h, reps=args.reps, rounds=args.rounds, fragments=total, query=queries, median_ms=med)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    t.dispose()
    for prog in programs.values():
        prog.dispose()


def line_main(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fragment_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd._capi import call
    from tendrils_amd.particles import FragmentProgram, draw_stages
    from tendrils_amd.tendrils import View
    from test_fragment_program_build import VIGNETTE, FragUniforms
    from test_fragment_program_line_build import FALLOFF

    class Falloff(C.Structure):
        _fields_ = [("halfWidth", C.c_float)]

    n, w, h = args.root, args.width, args.height
    workload.N = n
    programs = dict(vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"),
                    falloff=FragmentProgram.from_source(FALLOFF, Falloff, "falloff"))
    opts = ta.defaults()
    opts["lineWidthRange"] = (1, max(1.0, args.line_width))
    opts["state"]["flowWidth"] = args.line_width
    t = ta.Tendrils(View(w, h), opts)
    t.resize()
    t.setup(n)
    p, ctx = t.particles, t.particles._ctx
    p.upload_texels(workload.synth_state(0))
    t.colorMap.set_pixels(np.random.default_rng(7).uniform(0, 1, (64, 64, 4)).astype(np.float32))
    t.timer.time = 1000.0
    for _ in range(3):
        t.timer.tick()
        t.step()
    p.draw_pipeline("stream")
    p.option("draw_reuse", 0)
    t.line_widths()
    uniforms = dict(t.state, halfWidth=0.5 * args.line_width + 0.5, tint=[0.5, 0.25, 0.75, 0.875], invRes=[1.0 / w, 1.0 / h], edge=3.5 / (w * w + h * h), gain=0.625)
    d = t.deposit_uniforms()
    held = {name: draw_stages(None, prog, uniforms, d) for name, prog in programs.items()}
    frags = {}

    def plain():
        count = C.c_uint64(0)
        call("th_flow_deposit", ctx, C.byref(d), C.byref(count))
        frags["plain"] = count.value

    def staged(name):
        def run():
            count = C.c_uint64(0)
            call("th_draw_stages_run", ctx, C.byref(held[name][0]), 0, C.byref(count))
            frags[name] = count.value
        return run

    arms = dict(plain=plain, vignette=staged("vignette"), falloff=staged("falloff"))

    def timed(name, fn, reps):
        ms, kernel = C.c_float(0), None
        if name != "plain":
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if name != "plain":
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)
            kernel = mean.value
        return ms.value / reps, kernel

    for name, fn in arms.items():
        timed(name, fn, args.warmup)
    total = frags["plain"]
    assert all(v == total for v in frags.values()), frags
    moved = {"copy(36)": 36 * total, "copy(48)": 48 * total, "copy(lines)": 20 * total + 40 * n * n}
    copies = {}
    for name, size in moved.items():                 # half read, half written
        src = torch.empty(size // 2, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))

    def copy_ms(name, reps):
        src, dst = copies[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for name in copies:
        copy_ms(name, args.warmup)
    rounds = {}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ms, kernel = timed(name, fn, args.reps)
            rounds.setdefault("pass(%s)" % name, []).append(ms)
            if kernel is not None:
                rounds.setdefault("kernel(%s)" % name, []).append(kernel)
        for name in copies:
            rounds.setdefault(name, []).append(copy_ms(name, args.reps))
    queries = {name: prog.query(p) for name, prog in programs.items()}
    moved.update({"kernel(vignette)": 36 * total, "kernel(falloff)": 48 * total})
    lines = ["a stage that reads the fragment's line, the flow pass at width %g, %d^2 particles (C3 state, 3 steps in) into %d x %d, stream-ordered pipeline, reuse off; "
             "%d rounds of %d calls, arms alternating; GPU ms per call (events on the stream)" % (args.line_width, n, w, h, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "fragments per pass: %d; lines: %d" % (total, n * n),
             "%-20s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    med = {}
    for name, ms in rounds.items():
        med[name] = statistics.median(ms)
        gbps = "%.1f" % (moved[name] / med[name] / 1e6) if name in moved else "-"
        lines.append("%-20s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), gbps))
    line_kernels = med["pass(falloff)"] - med["pass(vignette)"] - (med["kernel(falloff)"] - med["kernel(vignette)"])
    lines.append("pass(vignette) / pass(plain) = %.3f;  pass(falloff) / pass(plain) = %.3f;  pass(falloff) / pass(vignette) = %.3f  (time ratios)"
                 % (med["pass(vignette)"] / med["pass(plain)"], med["pass(falloff)"] / med["pass(plain)"], med["pass(falloff)"] / med["pass(vignette)"]))
    lines.append("the line kernels, from the events: pass(falloff) - pass(vignette) - (kernel(falloff) - kernel(vignette)) = %.4f ms;  / copy(lines) = %.3f;  kernel(falloff) / copy(48) = %.3f"
                 % (line_kernels, line_kernels / med["copy(lines)"], med["kernel(falloff)"] / med["copy(48)"]))
    for name, info in queries.items():
        lines.append("th_program_query(%s): %s" % (name, json.dumps(info)))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(root=n, width=w, height=h, line_width=args.line_width, reps=args.reps, rounds=args.rounds, fragments=total, query=queries, median_ms=med)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    t.dispose()
    for prog in programs.values():
        prog.dispose()


def bins_main(args):
    import time

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fragment_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import FragmentProgram
    from tendrils_amd.tendrils import View
    from test_fragment_program_build import IDENTITY, VIGNETTE, FragUniforms

    n, w, h = args.root, args.width, args.height
    workload.N = n
    identity = FragmentProgram.from_source(IDENTITY, name="identity")
    vignette = FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette")
    gain = FragmentProgram.from_source(GAIN, GainUniforms, "gain")
    block = dict(gain=0.5, tint=[0.5, 0.25, 0.75, 0.875], invRes=[1.0 / w, 1.0 / h], edge=3.5 / (w * w + h * h))
    state0 = workload.synth_state(0)
    cmap = np.random.default_rng(7).uniform(0, 1, (64, 64, 4)).astype(np.float32)

    def loop(stage, stage_bins):
        opts = ta.defaults()
        if stage is not None:
            opts.update(flowShader=(None, stage), renderShader=(None, stage))
        t = ta.Tendrils(View(w, h), opts)
        t.resize()
        t.setup(n)
        t.particles.upload_texels(state0)
        t.colorMap.set_pixels(cmap)
        t.uniforms["render"].update(block)
        t.particles.option("stage_bins", stage_bins)
        t.timer.time = 1000.0
        return t

    loops = {"off": loop(vignette, 0), "on": loop(vignette, 1), "identity, off": loop(identity, 0), "identity, on": loop(identity, 1), "builtin": loop(None, 0)}

    def frames(t, count):
        """wall ms per frame"""
        t.particles.sync()
        t0 = time.perf_counter()
        for _ in range(count):
            t.timer.tick()
            t.step()
            t.draw()
        t.particles.sync()
        return (time.perf_counter() - t0) * 1e3 / count

    def held(t):
        info, order = _capi.DrawInfo(), _capi.SlotOrderInfo()
        call("th_draw_query", t.particles._ctx, C.byref(info))
        call("th_slot_order", t.particles._ctx, C.byref(order))
        return dict(pipeline="bins" if info.pipeline == 1 else "stream", fragments=int(info.fragments), crowded_fragments=int(info.crowded_fragments),
                    sorted_buffers=int(order.sorted_buffers))

    for t in loops.values():
        frames(t, args.warmup_frames)
    rounds = {}
    for _ in range(args.rounds):
        for name, t in loops.items():
            rounds.setdefault("loop(%s)" % name, []).append(frames(t, args.reps))
    state = {name: held(t) for name, t in loops.items()}
    assert state["on"]["fragments"] == state["off"]["fragments"], state      # (the same frames: the same lines)
    assert state["identity, on"]["fragments"] == state["identity, off"]["fragments"] == state["builtin"]["fragments"], state

    # the flow pass alone (no step in between: every call draws the same lines), on two states: a context three steps in - every
    # line a texel or two long, no crowded bin: the state of the stream-ordered figures (without --bins) - and the loop(on)
    # context as its frames left it
    fresh = loop(None, 1)
    for _ in range(3):
        fresh.timer.tick()
        fresh.step()
    fresh.line_widths()
    totals = {}
    for label, t in (("3 steps in", fresh), ("after the loop", loops["on"])):
        totals[label] = passes(args, t, label, dict(gain=gain, vignette=vignette), block, rounds)
        assert held(t)["pipeline"] == "bins", held(t)
        state[label] = held(t)

    lines = ["fragment stage through the bins (TH_OPT_STAGE_BINS), %d^2 particles (C3 state) into %d x %d, policy auto; %d frames of warm-up a loop, then "
             "%d rounds of %d frames / calls, arms alternating; loop: wall ms per frame (synchronised); pass, kernel, copy: GPU ms per call (events)"
             % (n, w, h, args.warmup_frames, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0)]
    for name in state:
        lines.append("%s: %s" % ("loop(%s) after its last frame" % name if name in loops else "the flow pass " + name, json.dumps(state[name])))
    lines.append("%-36s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)"))
    med = {}
    for name, ms in rounds.items():
        med[name] = statistics.median(ms)
        label = name.split(" @ ")[-1]
        gbps = "%.1f" % (40 * totals[label] / med[name] / 1e6) if name.startswith(("kernel(", "copy(")) else "-"
        lines.append("%-36s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), gbps))
    lines.append("loop(on) / loop(off) = %.3f;  loop(identity, on) / loop(identity, off) = %.3f;  loop(identity, on) / loop(builtin) = %.3f;  loop(identity, off) / loop(builtin) = %.3f  (time ratios)"
                 % (med["loop(on)"] / med["loop(off)"], med["loop(identity, on)"] / med["loop(identity, off)"], med["loop(identity, on)"] / med["loop(builtin)"],
                    med["loop(identity, off)"] / med["loop(builtin)"]))
    for label in totals:
        m = lambda arm: med["%s @ %s" % (arm, label)]      # noqa: E731
        lines.append("%s: pass(gain) / pass(plain) = %.3f;  pass(vignette) / pass(plain) = %.3f;  kernel(gain) / copy(40) = %.3f;  kernel(vignette) / copy(40) = %.3f  (time ratios)"
                     % (label, m("pass(gain)") / m("pass(plain)"), m("pass(vignette)") / m("pass(plain)"), m("kernel(gain)") / m("copy(40)"), m("kernel(vignette)") / m("copy(40)")))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(root=n, width=w, height=h, reps=args.reps, rounds=args.rounds, fragments=totals, state=state, median_ms=med)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in list(loops.values()) + [fresh]:
        t.dispose()
    for prog in (identity, vignette, gain):
        prog.dispose()


def line_bins_main(args):
    import time

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fragment_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import FragmentProgram, draw_stages
    from tendrils_amd.tendrils import View
    from test_fragment_program_build import IDENTITY
    from test_fragment_program_line_build import FALLOFF

    class Falloff(C.Structure):
        _fields_ = [("halfWidth", C.c_float)]

    n, w, h = args.root, args.width, args.height
    workload.N = n
    identity = FragmentProgram.from_source(IDENTITY, name="identity")
    falloff = FragmentProgram.from_source(FALLOFF, Falloff, "falloff")
    gain = FragmentProgram.from_source(GAIN, GainUniforms, "gain")
    block = dict(gain=0.5, halfWidth=0.5 * args.line_width + 0.5)
    state0 = workload.synth_state(0)
    cmap = np.random.default_rng(7).uniform(0, 1, (64, 64, 4)).astype(np.float32)
    policy = "bins" if args.line_width > 2.0 else "auto"

    def loop(stage, line_bins, pipeline=policy):
        opts = ta.defaults()
        opts["lineWidthRange"] = (1, max(1.0, args.line_width))
        opts["state"]["flowWidth"] = args.line_width
        if stage is not None:
            opts.update(flowShader=(None, stage))
        t = ta.Tendrils(View(w, h), opts)
        t.resize()
        t.setup(n)
        t.particles.upload_texels(state0)
        t.colorMap.set_pixels(cmap)
        t.uniforms["render"].update(block)
        t.particles.draw_pipeline(pipeline)
        t.particles.option("stage_bins", 1)
        t.particles.option("line_bins", line_bins)
        t.timer.time = 1000.0
        return t

    loops = {"falloff, off": loop(falloff, 0), "falloff, on": loop(falloff, 1), "identity": loop(identity, 0), "builtin": loop(None, 0)}

    def frames(t, count):
        """wall ms per frame"""
        t.particles.sync()
        t0 = time.perf_counter()
        for _ in range(count):
            t.timer.tick()
            t.step()
            t.draw()
        t.particles.sync()
        return (time.perf_counter() - t0) * 1e3 / count

    def held(t):
        info, order = _capi.DrawInfo(), _capi.SlotOrderInfo()
        call("th_draw_query", t.particles._ctx, C.byref(info))
        call("th_slot_order", t.particles._ctx, C.byref(order))
        return dict(pipeline="bins" if info.pipeline == 1 else "stream", fragments=int(info.fragments), crowded_fragments=int(info.crowded_fragments),
                    sorted_buffers=int(order.sorted_buffers), flow_fragments=int(getattr(t, "fragments", 0)))

    for t in loops.values():
        frames(t, args.warmup_frames)
    rounds = {}
    for _ in range(args.rounds):
        for name, t in loops.items():
            rounds.setdefault("loop(%s)" % name, []).append(frames(t, args.reps))
    state = {name: held(t) for name, t in loops.items()}
    assert state["falloff, on"]["flow_fragments"] == state["falloff, off"]["flow_fragments"], state      # (the same frames: the same lines)
    assert state["identity"]["flow_fragments"] == state["builtin"]["flow_fragments"], state

    # the flow pass alone, three steps in (every call draws the same lines), policy bins
    fresh = loop(None, 1, "bins")
    for _ in range(3):
        fresh.timer.tick()
        fresh.step()
    fresh.line_widths()
    ctx, d = fresh.particles._ctx, fresh.deposit_uniforms()
    uniforms = dict(fresh.state, **block)
    stages = {name: draw_stages(None, prog, uniforms, d) for name, prog in (("gain", gain), ("falloff", falloff))}
    frags = {}

    def plain():
        count = C.c_uint64(0)
        call("th_flow_deposit", ctx, C.byref(d), C.byref(count))
        frags["plain"] = count.value

    def staged(name):
        def run():
            count = C.c_uint64(0)
            call("th_draw_stages_run", ctx, C.byref(stages[name][0]), 0, C.byref(count))
            frags[name] = count.value
        return run

    arms = dict(plain=plain, gain=staged("gain"), falloff=staged("falloff"))

    def timed(name, fn, reps):
        ms, kernel = C.c_float(0), None
        if name != "plain":
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if name != "plain":
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)          # (one attempt a pass: nothing was repeated)
            kernel = mean.value
        return ms.value / reps, kernel

    for name, fn in arms.items():
        timed(name, fn, args.warmup)
        assert held(fresh)["pipeline"] == "bins", (name, held(fresh))
    total = frags["plain"]
    assert all(v == total for v in frags.values()), frags
    moved = {"copy(ends)": 48 * n * n, "copy(records)": 40 * total, "copy(56)": 56 * total}
    copies = {}
    for name, size in moved.items():                 # half read, half written
        src = torch.empty(size // 2, dtype=torch.uint8, device="cuda")
        copies[name] = (src, torch.empty_like(src))

    def copy_ms(name, reps):
        src, dst = copies[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for name in copies:
        copy_ms(name, args.warmup)
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ms, kernel = timed(name, fn, args.reps)
            rounds.setdefault("pass(%s)" % name, []).append(ms)
            if kernel is not None:
                rounds.setdefault("kernel(%s)" % name, []).append(kernel)
        for name in copies:
            rounds.setdefault(name, []).append(copy_ms(name, args.reps))
    state["the flow pass, 3 steps in"] = held(fresh)
    moved.update({"kernel(gain)": 40 * total, "kernel(falloff)": 56 * total})

    lines = ["a stage that reads the fragment's line through the bins (TH_OPT_LINE_BINS), flow lines at width %g, %d^2 particles (C3 state) into %d x %d, "
             "stage_bins = 1, policy %s; %d frames of warm-up a loop, then %d rounds of %d frames / calls, arms alternating; loop: wall ms per frame "
             "(synchronised); pass, kernel, copy: GPU ms per call (events)" % (args.line_width, n, w, h, policy, args.warmup_frames, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "fragments of the flow pass, 3 steps in: %d; lines: %d" % (total, n * n)]
    for name in state:
        lines.append("%s: %s" % ("loop(%s) after its last frame" % name if name in loops else name, json.dumps(state[name])))
    lines.append("%-28s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)"))
    med = {}
    for name, ms in rounds.items():
        med[name] = statistics.median(ms)
        gbps = "%.1f" % (moved[name] / med[name] / 1e6) if name in moved else "-"
        lines.append("%-28s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), gbps))
    both = med["pass(falloff)"] - med["pass(gain)"] - (med["kernel(falloff)"] - med["kernel(gain)"])
    lines.append("loop(falloff, on) / loop(falloff, off) = %.3f;  loop(falloff, on) / loop(identity) = %.3f;  loop(identity) / loop(builtin) = %.3f  (time ratios)"
                 % (med["loop(falloff, on)"] / med["loop(falloff, off)"], med["loop(falloff, on)"] / med["loop(identity)"], med["loop(identity)"] / med["loop(builtin)"]))
    lines.append("pass(gain) / pass(plain) = %.3f;  pass(falloff) / pass(plain) = %.3f;  pass(falloff) / pass(gain) = %.3f;  kernel(falloff) / copy(56) = %.3f  (time ratios)"
                 % (med["pass(gain)"] / med["pass(plain)"], med["pass(falloff)"] / med["pass(plain)"], med["pass(falloff)"] / med["pass(gain)"], med["kernel(falloff)"] / med["copy(56)"]))
    lines.append("the two line kernels, from the events: pass(falloff) - pass(gain) - (kernel(falloff) - kernel(gain)) = %.4f ms;  / (copy(ends) + copy(records)) = %.3f"
                 % (both, both / (med["copy(ends)"] + med["copy(records)"])))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(root=n, width=w, height=h, line_width=args.line_width, reps=args.reps, rounds=args.rounds, fragments=total, state=state, median_ms=med)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in list(loops.values()) + [fresh]:
        t.dispose()
    for prog in (identity, falloff, gain):
        prog.dispose()


def passes(args, t, label, programs, block, rounds):
    """the flow pass of `t` without a stage and with each of `programs`, the bins kernel alone, the copy of its bytes: into
    `rounds` under "<arm> @ <label>"; returns the pass's fragments"""
    import torch
    from tendrils_amd._capi import call
    from tendrils_amd.particles import draw_stages
    ctx, d = t.particles._ctx, t.deposit_uniforms()
    uniforms = dict(t.state, **block)
    stages = {name: draw_stages(None, prog, uniforms, d) for name, prog in programs.items()}
    frags = {}

    def plain():
        count = C.c_uint64(0)
        call("th_flow_deposit", ctx, C.byref(d), C.byref(count))
        frags["plain"] = count.value

    def staged(name):
        def run():
            count = C.c_uint64(0)
            call("th_draw_stages_run", ctx, C.byref(stages[name][0]), 0, C.byref(count))
            frags[name] = count.value
        return run

    arms = dict(plain=plain, **{name: staged(name) for name in programs})

    def timed(name, fn, reps):
        ms, kernel = C.c_float(0), None
        if name != "plain":
            call("th_kernel_timing", ctx, 1)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        if name != "plain":
            mean, launches = C.c_float(0), C.c_int32(0)
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert launches.value == reps, (launches.value, reps)          # (one attempt a pass: nothing was repeated)
            kernel = mean.value
        return ms.value / reps, kernel

    for name, fn in arms.items():
        timed(name, fn, args.warmup)
    total = frags["plain"]
    assert all(v == total for v in frags.values()), frags
    src = torch.empty(total * 20, dtype=torch.uint8, device="cuda")          # (40 bytes a fragment in all: half read, half written)
    dst = torch.empty_like(src)

    def copy_ms(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    copy_ms(args.warmup)
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ms, kernel = timed(name, fn, args.reps)
            rounds.setdefault("pass(%s) @ %s" % (name, label), []).append(ms)
            if kernel is not None:
                rounds.setdefault("kernel(%s) @ %s" % (name, label), []).append(kernel)
        rounds.setdefault("copy(40) @ %s" % label, []).append(copy_ms(args.reps))
    return total


def pair_main(args):
    import time

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fragment_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import FragmentProgram, draw_stages
    from tendrils_amd.tendrils import View
    from test_fragment_program_build import IDENTITY, VIGNETTE, FragUniforms

    n, w, h = args.root, args.width, args.height
    workload.N = n
    identity = FragmentProgram.from_source(IDENTITY, name="identity")
    vignette = FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette")
    gain = FragmentProgram.from_source(GAIN, GainUniforms, "gain")
    block = dict(gain=0.5, tint=[0.5, 0.25, 0.75, 0.875], invRes=[1.0 / w, 1.0 / h], edge=3.5 / (w * w + h * h))
    state0 = workload.synth_state(0)
    cmap = np.random.default_rng(7).uniform(0, 1, (64, 64, 4)).astype(np.float32)
    stage_bins = 1 if args.bins else 0
    wanted = set(args.arms.split(","))

    def loop(flow_stage, view_stage, paired):
        opts = ta.defaults()
        if flow_stage is not None:
            opts.update(flowShader=(None, flow_stage))
        if view_stage is not None:
            opts.update(renderShader=(None, view_stage))
        if paired:
            opts.update(pairedStages=True)
        t = ta.Tendrils(View(w, h), opts)
        t.resize()
        t.setup(n)
        t.particles.upload_texels(state0)
        t.colorMap.set_pixels(cmap)
        t.uniforms["render"].update(block)
        t.particles.option("stage_bins", stage_bins)
        t.timer.time = 1000.0
        return t

    shaders = {"identity": (identity, identity), "vignette": (vignette, vignette), "vignette, flow alone": (vignette, None)}
    loops = {}
    for name, (flow_stage, view_stage) in shaders.items():
        for arm in ("off", "on"):
            if arm in wanted:
                loops["%s, %s" % (name, arm)] = loop(flow_stage, view_stage, arm == "on")
    if "builtin" in wanted:
        loops["builtin"] = loop(None, None, False)

    def frames(t, count):
        """wall ms per frame"""
        t.particles.sync()
        t0 = time.perf_counter()
        for _ in range(count):
            t.timer.tick()
            t.step()
            t.draw()
        t.particles.sync()
        return (time.perf_counter() - t0) * 1e3 / count

    def held(t):
        info, order = _capi.DrawInfo(), _capi.SlotOrderInfo()
        call("th_draw_query", t.particles._ctx, C.byref(info))
        call("th_slot_order", t.particles._ctx, C.byref(order))
        return dict(pipeline="bins" if info.pipeline == 1 else "stream", fragments=int(info.fragments), crowded_fragments=int(info.crowded_fragments),
                    sorted_buffers=int(order.sorted_buffers), rasterisations=getattr(t, "rasterisations", None))

    for t in loops.values():
        frames(t, args.warmup_frames)
    rounds = {}
    for _ in range(args.rounds):
        for name, t in loops.items():
            rounds.setdefault("loop(%s)" % name, []).append(frames(t, args.reps))
    state = {name: held(t) for name, t in loops.items()}
    same = {}
    if "on" in wanted and "off" in wanted:
        # the same frames, the same bits: the flow field and the view of each on / off pair after the last frame
        for name in shaders:
            on, off = loops[name + ", on"], loops[name + ", off"]
            assert state[name + ", on"]["fragments"] == state[name + ", off"]["fragments"] and on.rasterisations == 1, (name, state)
            same[name] = bool((on.flow.read().view(np.uint32) == off.flow.read().view(np.uint32)).all() and (on.read_view() == off.read_view()).all())
            assert same[name], "loop(%s): the paired frames are not the unpaired frames" % name

    # each pair kernel alone, on a context three steps in (every line a texel or two long, no crowded bin): one th_draw_stages_pair
    # with the program in the VIEW slot - one launch, th_kernel_timing's pair around it - against a device-to-device copy of the
    # bytes the kernel moves a fragment: the key (4 bytes stream-ordered, 8 in the page store), 16 bytes read, 16 written
    kernels, total = {}, 0
    if "on" in wanted:
        fresh = loop(None, None, False)
        if args.bins:
            fresh.particles.draw_pipeline("bins")
        for _ in range(3):
            fresh.timer.tick()
            fresh.step()
        fresh.line_widths()
        ctx = fresh.particles._ctx
        uniforms = dict(fresh.state, **block)
        d, r = fresh.deposit_uniforms(), fresh.render_uniforms()
        flow_slot = draw_stages(None, None, uniforms, d)

        def kernel_ms(prog, reps):
            view_slot = draw_stages(None, prog, uniforms, r)
            count, ran, mean, launches = C.c_uint64(0), C.c_int32(0), C.c_float(0), C.c_int32(0)
            call("th_kernel_timing", ctx, 1)
            for _ in range(reps):
                call("th_draw_stages_pair", ctx, C.byref(flow_slot[0]), C.byref(view_slot[0]), C.byref(count), C.byref(ran))
            call("th_kernel_timing_read", ctx, C.byref(mean), C.byref(launches))
            call("th_kernel_timing", ctx, 0)
            assert ran.value == 1 and launches.value == reps, (ran.value, launches.value, reps)
            return mean.value, int(count.value)

        per_fragment = 40 if args.bins else 36
        for name, prog in (("gain", gain), ("vignette", vignette)):
            _, total = kernel_ms(prog, args.warmup)
        src = torch.empty(total * (per_fragment // 2), dtype=torch.uint8, device="cuda")          # (half read, half written)
        dst = torch.empty_like(src)

        def copy_ms(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        copy_ms(args.warmup)
        for _ in range(args.rounds):
            for name, prog in (("gain", gain), ("vignette", vignette)):
                kernels.setdefault("kernel(%s)" % name, []).append(kernel_ms(prog, args.reps)[0])
            kernels.setdefault("copy(%d)" % per_fragment, []).append(copy_ms(args.reps))
        state["the pair call, 3 steps in"] = held(fresh)
        assert state["the pair call, 3 steps in"]["pipeline"] == ("bins" if args.bins else "stream"), state
        fresh.dispose()

    kernel_name = "th_fragment_pair_bins_kernel" if args.bins else "th_fragment_pair_kernel"
    lines = ["both passes' fragment stages over one rasterisation (th_draw_stages_pair; Tendrils.pairedStages), stage_bins %d: %d^2 particles (C3 state) "
             "into %d x %d, policy auto; %d frames of warm-up a loop, then %d rounds of %d frames / calls, arms alternating; loop: wall ms per "
             "frame of step(); draw() (synchronised); kernel (%s alone, th_kernel_timing), copy: GPU ms per call (events)"
             % (stage_bins, n, w, h, args.warmup_frames, args.rounds, args.reps, kernel_name),
             "device: %s" % torch.cuda.get_device_name(0), "arms: %s" % args.arms,
             "on / off pairs after their last frame, flow field and view bit for bit: %s" % json.dumps(same)]
    for name in state:
        lines.append("%s: %s" % ("loop(%s) after its last frame" % name if name in loops else name, json.dumps(state[name])))
    lines.append("%-36s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)"))
    med = {}
    for name, ms in list(rounds.items()) + list(kernels.items()):
        med[name] = statistics.median(ms)
        gbps = "%.1f" % ((40 if args.bins else 36) * total / med[name] / 1e6) if name in kernels else "-"
        lines.append("%-36s %10.4f %10.4f %10.4f %14s" % (name, med[name], min(ms), max(ms), gbps))
    if "on" in wanted and "off" in wanted:
        for name in shaders:
            on, off = rounds["loop(%s, on)" % name], rounds["loop(%s, off)" % name]
            lines.append("loop(%s): on / off = %.3f (time ratio of the medians); on %.4f .. %.4f, off %.4f .. %.4f: the on arm's range %s below the off arm's"
                         % (name, med["loop(%s, on)" % name] / med["loop(%s, off)" % name], min(on), max(on), min(off), max(off),
                            "lies" if max(on) < min(off) else "does NOT lie"))
        if "builtin" in wanted:
            lines.append("loop(identity, on) / loop(builtin) = %.3f;  loop(identity, off) / loop(builtin) = %.3f  (time ratios)"
                         % (med["loop(identity, on)"] / med["loop(builtin)"], med["loop(identity, off)"] / med["loop(builtin)"]))
    if kernels:
        copy = "copy(%d)" % (40 if args.bins else 36)
        lines.append("kernel(gain) / %s = %.3f;  kernel(vignette) / %s = %.3f  (time ratios; %d fragments)"
                     % (copy, med["kernel(gain)"] / med[copy], copy, med["kernel(vignette)"] / med[copy], total))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(root=n, width=w, height=h, reps=args.reps, rounds=args.rounds, stage_bins=stage_bins, fragments=total, state=state, median_ms=med)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in loops.values():
        t.dispose()
    for prog in (identity, vignette, gain):
        prog.dispose()


if __name__ == "__main__":
    main()
