"""GPU time of the density map (tendrils_amd/csrc/th_density.hip) against what bounds it, on one MI355X: 4096 x 4096 particles
onto a 1920 x 1080 grid (the flow's shape, the view size step() hands the integrator), after 20 steps of the reference's default
uniforms from a uniform seeded state.

Rings, one context each:
  texel    f32 ring, TH_OPT "bucket" 0: the slots in texel order - neighbouring slots anywhere in the view
  sorted   f32 ring, "bucket" 1: tile-sorted slots as the fused launch of th_step_n(20) leaves them - sorted in front of the
           launch, so 20 steps old: a particle has drifted up to 0.01 of the view (10 cells) a step since
  fresh    the same, re-sorted in front of the last TWO steps ("rebucket_steps" 1 for a launch of two: the shortest fused
           launch): a block of slots is one neighbourhood of the view
  packed   TH_STATE_F16 ring (8 B a particle), "bucket" 0
Arms, all in this process, alternating:
  density         th_density_async: clear + tally + convert, between two events on the context's stream (th_timer_start / _stop)
  plain_atomics   the comparison arm the product does not carry: one global integer atomic per word per particle and nothing
                  summed on chip - as a measure program whose sample function adds the particle's count and its two velocity
                  quanta to accumulators of the tool's own (the same cell and quantum arithmetic, the same three atomics; no
                  clear and no convert pass, and over sorted slots a perm load the density does not need)
  measure_1       th_measure_async of tools/measure_program_bench.py's one-channel program: a pass over the same ring that adds
                  nothing to memory
  memcpy_d2d      hipMemcpyAsync, device to device, of one ring buffer (texel and packed rings)
Each figure is GPU ms per call over --reps calls after --warmup calls; the arms alternate for --rounds rounds, the median round
is reported with the range.

Usage: python tools/density_bench.py [--size 4096] [--grid 1920 1080] [--steps 20] [--reps 10] [--warmup 2] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.measure_program_bench import ONE      # noqa: E402

PLAIN = """struct Plain { unsigned long long *sum; unsigned *cnt; float vx, vy; int w, h; };
__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    const Plain &u = th_uniforms<Plain>(m);
    const float4 s = m.self;
    if (s.x == -1000000.0f && s.y == -1000000.0f) return th_no_sample();
    const float fx = floorf((((s.x * u.vx) + 1.0f) * 0.5f) * (float)u.w);
    const float fy = floorf((((s.y * u.vy) + 1.0f) * 0.5f) * (float)u.h);
    if (!(fx >= 0.0f && fx <= (float)(u.w - 1) && fy >= 0.0f && fy <= (float)(u.h - 1))) return th_no_sample();
    const unsigned cell = (unsigned)(int)fy * (unsigned)u.w + (unsigned)(int)fx;
    atomicAdd(&u.cnt[cell], 1u);
    if (fabsf(s.z) < __builtin_huge_valf())
        atomicAdd(&u.sum[2 * (size_t)cell], (unsigned long long)__float2ll_rn(fminf(fmaxf(s.z, -4.0f), 4.0f) * 4294967296.0f));
    if (fabsf(s.w) < __builtin_huge_valf())
        atomicAdd(&u.sum[2 * (size_t)cell + 1], (unsigned long long)__float2ll_rn(fminf(fmaxf(s.w, -4.0f), 4.0f) * 4294967296.0f));
    return th_no_sample();
}
"""
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


class Plain(C.Structure):
    _fields_ = [("sum", C.c_void_p), ("cnt", C.c_void_p), ("vx", C.c_float), ("vy", C.c_float), ("w", C.c_int32), ("h", C.c_int32)]


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
        sys.exit("density_bench: no GPU - nothing is measured without one")
    import numpy as np
    import tendrils_amd as ta
    from benchlib import workload
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import MeasureProgram
    from tendrils_amd.tendrils import View

    n, (gw, gh) = args.size, args.grid
    progs = dict(one=MeasureProgram.from_source(ONE, channels=1, name="one"),
                 plain=MeasureProgram.from_source(PLAIN, Plain, channels=1, name="plain_atomics"))
    state = workload.synth_rows(n, n, 12345)
    flow = np.zeros((gh, gw, 4), np.float32)
    rng = np.random.default_rng(4242)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (gh, gw, 2))
    flow[..., 2], flow[..., 3] = 2990.0, 1.0
    rings, facts = {}, {}
    for name, fmt, bucket in (("texel", _capi.TH_STATE_F32, 0), ("sorted", _capi.TH_STATE_F32, 1), ("fresh", _capi.TH_STATE_F32, 1),
                              ("packed", _capi.TH_STATE_F16, 0)):
        opts = ta.defaults()
        opts.update(rows=n, globalHeight=n, stateFormat=fmt)
        t = ta.Tendrils(View(gw, gh), opts)
        t.resize()
        t.setup(n)
        t.particles.option("bucket", bucket)
        t.particles.upload_texels(state)
        t.flow.set_pixels(flow)
        t.timer.time = 3000.0
        if name == "fresh":
            t.step_n(args.steps - 2)
            t.particles.option("rebucket_steps", 1)
            t.step_n(2)
        else:
            t.step_n(args.steps)
        is_sorted = C.c_int32(0)
        call("th_slot_order_read", t.particles._ctx, 0, None, None, 0, None, None, C.byref(is_sorted))
        assert bool(is_sorted.value) == (name in ("sorted", "fresh")), (name, is_sorted.value)
        d = t.density()
        facts[name] = {k: getattr(d, k) for k, _ in _capi.DensityInfo._fields_}
        rings[name] = t
    del state

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    acc_sum = torch.zeros(2 * gw * gh, dtype=torch.int64, device="cuda")
    acc_cnt = torch.zeros(gw * gh, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def density_arm(t):
        u, out = _capi.DensityUniforms(), C.c_void_p()
        u.viewSize[0], u.viewSize[1], u.w, u.h, u.dest, u.slot = t.viewSize[0], t.viewSize[1], gw, gh, _capi.VIEW_TEXTURE, 0
        return lambda: call("th_density_async", t.particles._ctx, C.byref(u), 0, C.byref(out))

    def plain_arm(t):
        u, out = Plain(acc_sum.data_ptr(), acc_cnt.data_ptr(), t.viewSize[0], t.viewSize[1], gw, gh), C.c_void_p()
        return lambda: call("th_measure_async", t.particles._ctx, progs["plain"].handle, C.byref(u), C.sizeof(u), 0, C.byref(out))

    def measure_arm(t):
        out = C.c_void_p()
        return lambda: call("th_measure_async", t.particles._ctx, progs["one"].handle, None, 0, 0, C.byref(out))

    def copy_arm(t, texel_bytes):
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

    arms = {}                                     # name -> (bytes of the ring read per call, Tendrils, the call)
    for ring, texel_bytes in (("texel", 16), ("sorted", 16), ("fresh", 16), ("packed", 8)):
        t = rings[ring]
        arms[ring + " density"] = (n * n * texel_bytes, t, density_arm(t))
        arms[ring + " plain_atomics"] = (n * n * texel_bytes, t, plain_arm(t))
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

    for _, t, fn in arms.values():
        timed(t, fn, args.warmup)
    rounds = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (_, t, fn) in arms.items():
            rounds[name].append(timed(t, fn, args.reps))

    lines = ["density map, %d x %d particles onto %d x %d, after %d steps, %d rounds of %d calls, arms alternating; GPU ms per call"
             % (n, n, gw, gh, args.steps, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0)]
    for ring, f in facts.items():
        lines.append("%-7s %s" % (ring, json.dumps(f)))
    lines.append("%-22s %10s %10s %10s %18s" % ("arm", "median ms", "min ms", "max ms", "ring GB/s (median)"))
    result = dict(size=n, grid=[gw, gh], steps=args.steps, reps=args.reps, rounds=args.rounds, facts=facts, arms={})
    for name, (size, _, _) in arms.items():
        med, lo, hi = statistics.median(rounds[name]), min(rounds[name]), max(rounds[name])
        result["arms"][name] = dict(median_ms=med, min_ms=lo, max_ms=hi, ring_bytes=size)
        lines.append("%-22s %10.4f %10.4f %10.4f %18.1f" % (name, med, lo, hi, size / med / 1e6))
    for ring in ("texel", "sorted", "fresh", "packed"):
        a, b = result["arms"][ring + " density"], result["arms"][ring + " plain_atomics"]
        lines.append("%s: density / plain_atomics = %.3f (medians; rounds' range of density %.4f ms, of plain_atomics %.4f ms)"
                     % (ring, a["median_ms"] / b["median_ms"], a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"]))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for t in rings.values():
        t.dispose()
    for prog in progs.values():
        prog.dispose()


if __name__ == "__main__":
    main()
