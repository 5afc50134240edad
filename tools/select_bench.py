"""GPU time of select (tendrils_amd/csrc/th_select.hip) against what bounds it and against the route it replaces, on one MI355X:
4096 x 4096 particles under a 1920 x 1080 flow, after 20 steps of the reference's default uniforms from a uniform seeded state.

Rings, one context each:
  texel    f32 ring, TH_OPT "bucket" 0: the slots in texel order - a wave's ballot is the mask word
  sorted   f32 ring, "bucket" 1: tile-sorted slots as the fused launch of th_step_n(20) leaves them - the perm table, the cleared
           mask and an integer atomic OR per match
  packed   TH_STATE_F16 ring (8 B a particle), "bucket" 0
Selections:
  nothing     an empty box (x0 == x1)
  stride64    index % 64 == 0 of the live particles
  quarter     the box of the view's upper right quarter
  everything  no clause: every live particle
Arms, all in this process, alternating, GPU ms per call between two events on the context's stream (th_timer_start / _stop):
  <selection>        th_select_async with capacity = matched: mark (+ clear and count over sorted slots), scan, total, gather
  <selection> count  th_select_async with capacity 0: no gather pass
  measure_1          th_measure_async of tools/measure_program_bench.py's one-channel program: the floor of reading the ring once
  memcpy_d2d         hipMemcpyAsync, device to device, of one ring buffer (texel and packed rings)
... and against the WALL clock, on the texel ring (a download would move the sorted ring to texel order), --wall-reps calls each:
  select <selection> wall   Particles.select(capacity=matched): the synchronous call, the records in host memory
  download + flatnonzero    th_download_state of the buffer and numpy's evaluation of the quarter box: the route select replaces
Each figure is ms per call over --reps calls after --warmup calls; the arms alternate for --rounds rounds, the median round is
reported with the range.

Usage: python tools/select_bench.py [--size 4096] [--grid 1920 1080] [--steps 20] [--reps 10] [--warmup 2] [--rounds 5] [--wall-reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.measure_program_bench import ONE      # noqa: E402

HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("select_bench: no GPU - nothing is measured without one")
    import numpy as np
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import MeasureProgram
    from tendrils_amd.tendrils import View

    n, (gw, gh) = args.size, args.grid
    one = MeasureProgram.from_source(ONE, channels=1, name="one")
    state = workload.synth_rows(n, n, 12345)
    flow = np.zeros((gh, gw, 4), np.float32)
    rng = np.random.default_rng(4242)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (gh, gw, 2))
    flow[..., 2], flow[..., 3] = 2990.0, 1.0
    rings = {}
    for name, fmt, bucket in (("texel", _capi.TH_STATE_F32, 0), ("sorted", _capi.TH_STATE_F32, 1), ("packed", _capi.TH_STATE_F16, 0)):
        opts = ta.defaults()
        opts.update(rows=n, globalHeight=n, stateFormat=fmt)
        t = ta.Tendrils(View(gw, gh), opts)
        t.resize()
        t.setup(n)
        t.particles.option("bucket", bucket)
        t.particles.upload_texels(state)
        t.flow.set_pixels(flow)
        t.timer.time = 3000.0
        t.step_n(args.steps)
        is_sorted = C.c_int32(0)
        call("th_slot_order_read", t.particles._ctx, 0, None, None, 0, None, None, C.byref(is_sorted))
        assert bool(is_sorted.value) == (name == "sorted"), (name, is_sorted.value)
        rings[name] = t
    del state

    view = rings["texel"].viewSize
    quarter = (0.0, 0.0, 1.0 / view[0], 1.0 / view[1])
    selections = dict(nothing=dict(box=(0.25, -2.0, 0.25, 2.0)), stride64=dict(stride=64, phase=0), quarter=dict(box=quarter), everything=dict())
    facts = {}
    for ring, t in rings.items():
        facts[ring] = {}
        for sel, kw in selections.items():
            s = t.particles.select(capacity=0, **kw)
            facts[ring][sel] = dict(particles=s.particles, live=s.live, matched=s.matched)

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def select_arm(t, kw, capacity):
        u, index = t.particles._select_args(kw.get("box"), kw.get("speed"), kw.get("stride", 1), kw.get("phase", 0), False, 0)
        return lambda: call("th_select_async", t.particles._ctx, C.byref(u), index, capacity, None, None)

    def measure_arm(t):
        out = C.c_void_p()
        return lambda: call("th_measure_async", t.particles._ctx, one.handle, None, 0, 0, C.byref(out))

    def copy_arm(t, texel_bytes):
        # (the copy overwrites ring buffer 1 of a context the other arms share: they all read buffer 0 only)
        ctx = t.particles._ctx
        stream, dst, src = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call("th_stream", ctx, C.byref(stream))
        call("th_state_device_ptr", ctx, 1, C.byref(dst))
        call("th_state_device_ptr", ctx, 0, C.byref(src))

        def copy():
            e = hip.hipMemcpyAsync(dst, src, n * n * texel_bytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
            if e:
                raise RuntimeError("hipMemcpyAsync: error %d" % e)
        return copy

    arms = {}                                     # name -> (bytes of the ring buffer, Tendrils, the call)
    for ring, texel_bytes in (("texel", 16), ("sorted", 16), ("packed", 8)):
        t = rings[ring]
        for sel, kw in selections.items():
            arms["%s %s" % (ring, sel)] = (n * n * texel_bytes, t, select_arm(t, kw, facts[ring][sel]["matched"]))
            arms["%s %s count" % (ring, sel)] = (n * n * texel_bytes, t, select_arm(t, kw, 0))
        arms[ring + " measure_1"] = (n * n * texel_bytes, t, measure_arm(t))
    for ring, texel_bytes in (("texel", 16), ("packed", 8)):      # (th_state_device_ptr would move the sorted ring to texel order)
        arms[ring + " memcpy_d2d"] = (n * n * texel_bytes, rings[ring], copy_arm(rings[ring], texel_bytes))

    def timed(t, fn, reps):
        ms = C.c_float(0)
        call("th_timer_start", t.particles._ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", t.particles._ctx, C.byref(ms))
        return ms.value / reps

    # the wall-clock arms, on the texel ring
    p = rings["texel"].particles
    wall = {}
    for sel in ("stride64", "quarter"):
        kw, capacity = selections[sel], facts["texel"][sel]["matched"]
        wall["select %s wall" % sel] = (lambda kw=kw, capacity=capacity: p.select(capacity=capacity, **kw))

    def download_route():
        st = p.read(0).reshape(-1, 4)
        x, y = st[:, 0], st[:, 1]
        live = ~((x == np.float32(-1e6)) & (y == np.float32(-1e6)))
        at = np.flatnonzero(live & (x >= np.float32(quarter[0])) & (x < np.float32(quarter[2])) & (y >= np.float32(quarter[1])) & (y < np.float32(quarter[3])))
        return st[at], at
    wall["download + flatnonzero"] = download_route
    assert len(download_route()[1]) == facts["texel"]["quarter"]["matched"]      # (the two routes agree on who is inside)

    def timed_wall(fn, reps):
        p.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1000.0 / reps

    for _, t, fn in arms.values():
        timed(t, fn, args.warmup)
    for fn in wall.values():
        timed_wall(fn, 1)
    rounds = {name: [] for name in list(arms) + list(wall)}
    for _ in range(args.rounds):
        for name, (_, t, fn) in arms.items():
            rounds[name].append(timed(t, fn, args.reps))
        for name, fn in wall.items():
            rounds[name].append(timed_wall(fn, args.wall_reps))

    lines = ["select, %d x %d particles under a %d x %d flow, after %d steps, %d rounds of %d calls (wall-clock arms: %d), arms alternating; ms per call"
             % (n, n, gw, gh, args.steps, args.rounds, args.reps, args.wall_reps),
             "device: %s" % torch.cuda.get_device_name(0)]
    for ring, f in facts.items():
        lines.append("%-7s %s" % (ring, json.dumps(f)))
    lines.append("%-28s %10s %10s %10s %18s" % ("arm (GPU ms)", "median ms", "min ms", "max ms", "ring GB/s (median)"))
    result = dict(size=n, grid=[gw, gh], steps=args.steps, reps=args.reps, rounds=args.rounds, wall_reps=args.wall_reps, facts=facts, arms={}, wall={})
    for name, (size, _, _) in arms.items():
        med, lo, hi = statistics.median(rounds[name]), min(rounds[name]), max(rounds[name])
        result["arms"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi, ring_bytes=size)
        lines.append("%-28s %10.4f %10.4f %10.4f %18.1f" % (name, med, lo, hi, size / med / 1e6))
    lines.append("%-28s %10s %10s %10s" % ("arm (wall-clock ms, texel)", "median ms", "min ms", "max ms"))
    for name in wall:
        med, lo, hi = statistics.median(rounds[name]), min(rounds[name]), max(rounds[name])
        result["wall"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi)
        lines.append("%-28s %10.3f %10.3f %10.3f" % (name, med, lo, hi))
    route = result["wall"]["download + flatnonzero"]["median_ms"]
    for sel in ("stride64", "quarter"):
        mine = result["wall"]["select %s wall" % sel]["median_ms"]
        lines.append("select %s / download route = %.4f (wall-clock medians): select is %s"
                     % (sel, mine / route, "FASTER" if mine < route else "NOT faster"))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in rings.values():
        t.dispose()
    one.dispose()


if __name__ == "__main__":
    main()
