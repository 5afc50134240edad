"""GPU time of a follow sample (tendrils_amd/csrc/th_follow.hip) against the route it replaces and against what bounds it, on one
MI355X: 4096 x 4096 particles under a 1920 x 1080 flow, after 20 steps of the reference's default uniforms from a uniform seeded
state.

Rings, one context each:
  texel    f32 ring, TH_OPT "bucket" 0: the slots in texel order - the slot of a followed texel is the texel, no table
  sorted   f32 ring, "bucket" 1: tile-sorted slots as the fused launch of th_step_n(20) leaves them - the slot table
  packed   TH_STATE_F16 ring (8 B a particle), "bucket" 0
Sets, each ring's own:
  stride64    select(stride=64).index: 1 : 64 of the live particles (262 144 when all are live)
  quarter4k   the box of the view's upper right quarter, thinned by a stride to about 4 096
Arms, all in this process, alternating, GPU ms per call between two events on the context's stream (th_timer_start / _stop):
  sample            th_follow_sample of buffer 0 with a valid slot table: one gather of n texels
  sample + locate   (sorted ring) the same call behind a step() that has re-sorted the slots ("resort_steps" 1: every single
                    step lays out a new order), the step outside the events: fill, the walk over perm, the gather.  The bench
                    asserts that `locates` grew by one per call.
  select            th_select_async of the SAME set where a predicate still describes it - stride 64, capacity = matched: the
                    route a sample replaces (two walks over the ring); the quarter4k set has its own predicate (box + stride)
  memcpy_d2d        hipMemcpyAsync, device to device, of n x 16 bytes (one row of the history into the next)
Each figure is ms per call over --reps calls after --warmup calls; the arms alternate for --rounds rounds, the median round is
reported with the range.

THE RULE, written before the run: on every ring a cached sample of the stride64 set is faster than the select of that set by
more than the rounds' ranges - max(sample rounds) < min(select rounds); and on the sorted ring a sample with a locate amortised
over the re-sort period of 64 single steps - (63 x sample + (sample + locate)) / 64, medians - stays below select's median too.

Usage: python tools/follow_bench.py [--size 4096] [--grid 1920 1080] [--steps 20] [--reps 10] [--warmup 2] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIP_MEMCPY_DEVICE_TO_DEVICE = 3
RESORT_PERIOD = 64                            # th_options::resort_steps: single steps between two re-sorts
RULE = ("rule (written before the run): on every ring max(sample stride64 rounds) < min(select stride64 rounds); on the sorted ring "
        "(63 x sample + (sample + locate)) / 64 < select, medians")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("follow_bench: no GPU - nothing is measured without one")
    import numpy as np
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.tendrils import View

    n, (gw, gh) = args.size, args.grid
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
    rings["sorted"].particles.option("resort_steps", 1)      # (the sample + locate arm: every single step re-sorts)

    view = rings["texel"].viewSize
    quarter = (0.0, 0.0, 1.0 / view[0], 1.0 / view[1])
    predicates, facts = {}, {}
    for ring, t in rings.items():
        inside = t.particles.select(capacity=0, box=quarter).matched
        predicates[ring] = dict(stride64=dict(stride=64, phase=0), quarter4k=dict(box=quarter, stride=max(1, inside // 4096), phase=0))
        facts[ring] = {}

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def timed(t, fn, reps, before=None):
        """ms per call of fn between two events on the context's stream; `before` runs in front of every call, outside them"""
        ctx, total, ms = t.particles._ctx, 0.0, C.c_float(0)
        if before is None:
            call("th_timer_start", ctx)
            for _ in range(reps):
                fn()
            call("th_timer_stop", ctx, C.byref(ms))
            return ms.value / reps
        for _ in range(reps):
            before()
            call("th_timer_start", ctx)
            fn()
            call("th_timer_stop", ctx, C.byref(ms))
            total += ms.value
        return total / reps

    def select_arm(t, kw, capacity):
        u, index = t.particles._select_args(kw.get("box"), None, kw.get("stride", 1), kw.get("phase", 0), False, 0)
        return lambda: call("th_select_async", t.particles._ctx, C.byref(u), index, capacity, None, None)

    def copy_arm(t, members):
        ctx = t.particles._ctx
        stream, history = C.c_void_p(), C.c_void_p()
        call("th_stream", ctx, C.byref(stream))
        call("th_follow_query", ctx, None, C.byref(history), None)
        src, dst = history.value, history.value + members * 16      # (rows 0 and 1 of a history of depth 4)

        def copy():
            e = hip.hipMemcpyAsync(dst, src, members * 16, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
            if e:
                raise RuntimeError("hipMemcpyAsync: error %d" % e)
        return copy

    def stepped(t):
        def step():
            t.timer.tick()
            t.step()
        return step

    lines = ["follow, %d x %d particles under a %d x %d flow, after %d steps, %d rounds of %d calls, arms alternating; GPU ms per call"
             % (n, n, gw, gh, args.steps, args.rounds, args.reps), "device: %s" % torch.cuda.get_device_name(0), RULE]
    print("\n".join(lines), flush=True)
    result = dict(size=n, grid=[gw, gh], steps=args.steps, reps=args.reps, rounds=args.rounds, facts=facts, arms={})
    rounds = {}
    for which in ("stride64", "quarter4k"):
        arms = {}                                 # name -> (Tendrils, the call, what runs in front of every call or None)
        for ring, t in rings.items():
            kw = predicates[ring][which]
            chosen = t.particles.select(**kw)
            follow = t.follow(chosen.index, depth=4)
            facts[ring][which] = dict(particles=chosen.particles, live=chosen.live, followed=len(follow), predicate={k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()})
            sample = (lambda follow=follow: follow.sample(time=0.0))
            sample()                              # (the slot table of the sorted ring is there before anything is timed)
            arms["%s %s sample" % (ring, which)] = (t, sample, None)
            if ring == "sorted":
                arms["%s %s sample + locate" % (ring, which)] = (t, sample, stepped(t))
            arms["%s %s select" % (ring, which)] = (t, select_arm(t, kw, chosen.matched), None)
            arms["%s %s memcpy_d2d" % (ring, which)] = (t, copy_arm(t, len(follow)), None)
            facts[ring][which]["follow"] = follow
        for name, (t, fn, before) in arms.items():
            timed(t, fn, args.warmup, before)
            if before is None and name.endswith(" sample"):
                fn()                              # (behind another arm's steps: the table is the current order's again)
        for _ in range(args.rounds):
            for name, (t, fn, before) in arms.items():
                follow = facts[name.split()[0]][which]["follow"]
                if before is None and name.endswith(" sample"):
                    fn()                          # (cached: the sorted ring's order may have changed under the locate arm)
                locates = follow.info.locates
                rounds.setdefault(name, []).append(timed(t, fn, args.reps, before))
                grown = follow.info.locates - locates
                if name.endswith(" sample + locate"):
                    assert grown == args.reps, (name, grown)       # every call behind a step walked perm
                elif name.endswith(" sample"):
                    assert grown == 0, (name, grown)               # ... and no cached one did
        for ring in rings:
            facts[ring][which]["locates"] = facts[ring][which].pop("follow").info.locates

    for ring, f in facts.items():
        lines.append("%-7s %s" % (ring, json.dumps(f)))
    lines.append("%-36s %10s %10s %10s" % ("arm (GPU ms)", "median ms", "min ms", "max ms"))
    for name, values in rounds.items():
        med, lo, hi = statistics.median(values), min(values), max(values)
        result["arms"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi)
        lines.append("%-36s %10.4f %10.4f %10.4f" % (name, med, lo, hi))
    for ring in rings:
        mine, route = rounds["%s stride64 sample" % ring], rounds["%s stride64 select" % ring]
        ok = max(mine) < min(route)
        lines.append("%s: sample stride64 / select stride64 = %.4f (medians), max sample %.4f vs min select %.4f: the rule %s"
                     % (ring, statistics.median(mine) / statistics.median(route), max(mine), min(route), "HOLDS" if ok else "FAILS"))
    cached, located = statistics.median(rounds["sorted stride64 sample"]), statistics.median(rounds["sorted stride64 sample + locate"])
    route = statistics.median(rounds["sorted stride64 select"])
    amortised = ((RESORT_PERIOD - 1) * cached + located) / RESORT_PERIOD
    lines.append("sorted: a sample with a locate every %d steps = %.4f ms amortised vs select %.4f ms: the rule %s"
                 % (RESORT_PERIOD, amortised, route, "HOLDS" if amortised < route else "FAILS"))
    result["amortised_ms"] = amortised
    text = "\n".join(lines)
    print("\n".join(lines[3:]))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in rings.values():
        t.dispose()


if __name__ == "__main__":
    main()
