"""GPU time of the histogram (tendrils_amd/csrc/th_histogram.hip) against what bounds it and against the route it replaces, on one
MI355X: 4096 x 4096 particles under a 1920 x 1080 flow, after 20 steps of the reference's default uniforms from a uniform seeded
state - the skew this workload really has (profiles/histogram.txt: the largest of 1024 speed bins holds under 1 % of the
particles) - and on a ring made for the worst case.

Rings, one context each:
  texel    f32 ring, TH_OPT "bucket" 0: the slots in texel order
  sorted   f32 ring, "bucket" 1: tile-sorted slots as the fused launch of th_step_n(20) leaves them (no clause reads the perm table)
  packed   TH_STATE_F16 ring (8 B a particle), "bucket" 0
  onebin   f32 ring in texel order, NOT stepped, every velocity (0.003, 0.004): every live particle in ONE bin of the speed's
           histogram - the worst case of the LDS atomics, all 64 lanes of every wave on one address
Histograms:
  x          TH_HIST_X, 1024 bins over (-1, 1): the spread case
  speed      TH_HIST_SPEED, 1024 bins over (0, speedLimit] (hi = the float above speedLimit: the cap has the last bin)
  key        one TH_HIST_KEY pass of TH_HIST_SPEED: 2048 bins, shift 21
  quantile   a whole Particles.quantiles("speed", 0.5): three key passes, each synchronised and read back - GPU ms over the three
Arms, all in this process, alternating, GPU ms per call between two events on the context's stream (th_timer_start / _stop):
  <histogram>   th_histogram_async (quantile: the synchronous passes)
  measure_1     th_measure_async of tools/measure_program_bench.py's one-channel program: the floor of reading the ring once
  memcpy_d2d    hipMemcpyAsync, device to device, of one ring buffer (texel and packed rings)
... and against the WALL clock, --wall-reps calls each:
  histogram speed wall / quantile wall   Particles.histogram / .quantiles: the synchronous calls, the result in host memory (every ring)
  download + np.histogram / np.partition th_download_state of the buffer and numpy's histogram of the speeds / their median: the
                                         route the calls replace (on the texel ring: a download would move the sorted ring to texel order)
Each figure is ms per call over --reps calls after --warmup calls; the arms alternate for --rounds rounds, the median round is
reported with the range.

Usage: python tools/histogram_bench.py [--size 4096] [--grid 1920 1080] [--steps 20] [--reps 10] [--warmup 2] [--rounds 5] [--wall-reps 3] [--out FILE]
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
RINGS = (("texel", "f32", 0, 16), ("sorted", "f32", 1, 16), ("packed", "f16", 0, 8), ("onebin", "f32", 0, 16))      # name, format, bucket, bytes a texel


def make_rings(n, grid, steps):
    """the four contexts, stepped (but "onebin"): {name: Tendrils}"""
    import numpy as np
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.tendrils import View

    gw, gh = grid
    state = workload.synth_rows(n, n, 12345)
    flow = np.zeros((gh, gw, 4), np.float32)
    rng = np.random.default_rng(4242)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (gh, gw, 2))
    flow[..., 2], flow[..., 3] = 2990.0, 1.0
    rings = {}
    for name, fmt, bucket, _ in RINGS:
        opts = ta.defaults()
        opts.update(rows=n, globalHeight=n, stateFormat=_capi.TH_STATE_F16 if fmt == "f16" else _capi.TH_STATE_F32)
        t = ta.Tendrils(View(gw, gh), opts)
        t.resize()
        t.setup(n)
        t.particles.option("bucket", bucket)
        if name == "onebin":
            state[..., 2], state[..., 3] = np.float32(0.003), np.float32(0.004)
        t.particles.upload_texels(state)
        t.flow.set_pixels(flow)
        t.timer.time = 3000.0
        if name != "onebin":
            t.step_n(steps)
        is_sorted = C.c_int32(0)
        call("th_slot_order_read", t.particles._ctx, 0, None, None, 0, None, None, C.byref(is_sorted))
        assert bool(is_sorted.value) == (name == "sorted"), (name, is_sorted.value)
        rings[name] = t
    return rings


def histograms(speed_limit):
    """{name: (channel, mode, bins, lo, hi, key_shift)}"""
    import numpy as np
    from tendrils_amd import _capi
    cap = float(np.nextafter(np.float32(speed_limit), np.float32(np.inf)))
    return dict(x=(_capi.HIST_X, _capi.HIST_LINEAR, 1024, -1.0, 1.0, 0), speed=(_capi.HIST_SPEED, _capi.HIST_LINEAR, 1024, 0.0, cap, 0),
                key=(_capi.HIST_SPEED, _capi.HIST_KEY, 2048, 0.0, 0.0, 21))


def histogram_arm(t, spec):
    """the enqueue-only call of one histogram over buffer 0 of `t`"""
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    channel, mode, bins, lo, hi, shift = spec
    u, index = t.particles._histogram_args(channel, mode, bins, {})
    u.lo, u.hi, u.key_shift = lo, hi, shift
    return lambda: call("th_histogram_async", t.particles._ctx, C.byref(u), index, None, None)


def timed(t, fn, reps):
    from tendrils_amd._capi import call
    ms = C.c_float(0)
    call("th_timer_start", t.particles._ctx)
    for _ in range(reps):
        fn()
    call("th_timer_stop", t.particles._ctx, C.byref(ms))
    return ms.value / reps


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
        sys.exit("histogram_bench: no GPU - nothing is measured without one")
    import numpy as np
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import MeasureProgram

    n, (gw, gh) = args.size, args.grid
    one = MeasureProgram.from_source(ONE, channels=1, name="one")
    rings = make_rings(n, (gw, gh), args.steps)
    limit = float(rings["texel"].state["speedLimit"])
    specs = histograms(limit)
    facts = {}
    for ring, t in rings.items():
        h = t.particles.histogram("speed", 1024, (specs["speed"][3], specs["speed"][4]))
        facts[ring] = dict(particles=h.particles, live=h.live, matched=h.matched, above=h.above, nan=h.nan, last_bin=int(h.counts[-1]),
                           largest_bin_share=float(h.counts.max()) / max(h.matched, 1), median_speed=float(t.particles.quantiles("speed", 0.5)))

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

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
    for ring, _fmt, _bucket, texel_bytes in RINGS:
        t = rings[ring]
        for name, spec in specs.items():
            arms["%s %s" % (ring, name)] = (n * n * texel_bytes, t, histogram_arm(t, spec))
        arms[ring + " quantile"] = (n * n * texel_bytes, t, (lambda t=t: t.particles.quantiles("speed", 0.5)))
        arms[ring + " measure_1"] = (n * n * texel_bytes, t, measure_arm(t))
    for ring, texel_bytes in (("texel", 16), ("packed", 8)):      # (th_state_device_ptr would move the sorted ring to texel order)
        arms[ring + " memcpy_d2d"] = (n * n * texel_bytes, rings[ring], copy_arm(rings[ring], texel_bytes))

    # the wall-clock arms
    wall = {}
    for ring, t in rings.items():
        wall["%s histogram speed wall" % ring] = (lambda t=t: t.particles.histogram("speed", 1024, (specs["speed"][3], specs["speed"][4])))
        wall["%s quantile wall" % ring] = (lambda t=t: t.particles.quantiles("speed", 0.5))
    p = rings["texel"].particles
    lo32, hi32 = np.float32(specs["speed"][3]), np.float32(specs["speed"][4])

    def speeds():
        st = p.read(0).reshape(-1, 4)
        live = ~((st[:, 0] == np.float32(-1e6)) & (st[:, 1] == np.float32(-1e6)))
        v = st[live, 2:]
        return np.sqrt((v[:, 0] * v[:, 0]) + (v[:, 1] * v[:, 1]))

    def download_histogram():
        return np.histogram(speeds(), 1024, (lo32, hi32))[0]

    def download_median():
        s = speeds()
        return np.partition(s, len(s) // 2)[len(s) // 2]
    wall["download + np.histogram"] = download_histogram
    wall["download + np.partition"] = download_median
    assert float(download_median()) == facts["texel"]["median_speed"]              # (the two routes agree on the median)

    def timed_wall(fn, reps):
        for t in rings.values():
            t.particles.sync()
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

    lines = ["histogram, %d x %d particles under a %d x %d flow, after %d steps (speedLimit %g), %d rounds of %d calls (wall-clock arms: %d), arms alternating; ms per call"
             % (n, n, gw, gh, args.steps, limit, args.rounds, args.reps, args.wall_reps),
             "device: %s" % torch.cuda.get_device_name(0)]
    for ring, f in facts.items():
        lines.append("%-7s %s" % (ring, json.dumps(f)))
    lines.append("%-28s %10s %10s %10s %18s %12s" % ("arm (GPU ms)", "median ms", "min ms", "max ms", "ring GB/s (median)", "x measure_1"))
    result = dict(size=n, grid=[gw, gh], steps=args.steps, reps=args.reps, rounds=args.rounds, wall_reps=args.wall_reps, facts=facts, arms={}, wall={})
    for name, (size, _, _) in arms.items():
        med, lo, hi = statistics.median(rounds[name]), min(rounds[name]), max(rounds[name])
        floor = statistics.median(rounds[name.split()[0] + " measure_1"])
        result["arms"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi, ring_bytes=size, measures=med / floor)
        lines.append("%-28s %10.4f %10.4f %10.4f %18.1f %12.2f" % (name, med, lo, hi, size / med / 1e6, med / floor))
    lines.append("%-34s %10s %10s %10s" % ("arm (wall-clock ms)", "median ms", "min ms", "max ms"))
    for name in wall:
        med, lo, hi = statistics.median(rounds[name]), min(rounds[name]), max(rounds[name])
        result["wall"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi)
        lines.append("%-34s %10.3f %10.3f %10.3f" % (name, med, lo, hi))
    for mine, route in (("histogram speed wall", "download + np.histogram"), ("quantile wall", "download + np.partition")):
        theirs = result["wall"][route]["median_ms"]
        for ring in rings:
            ours = result["wall"]["%s %s" % (ring, mine)]["median_ms"]
            lines.append("%s %s / %s = %.5f (wall-clock medians): the call is %s" % (ring, mine, route, ours / theirs, "FASTER" if ours < theirs else "NOT faster"))
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
