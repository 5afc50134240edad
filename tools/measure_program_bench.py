"""GPU time of a measure program (tendrils_amd/csrc/th_measure.hip, th_measure_prelude.inc) against what bounds it, on one
MI355X: 4096 x 4096 particles, a 1920 x 1080 flow field, an f32 ring (16 B a particle) and a TH_STATE_F16 ring (8 B).

Arms, all in this process, per ring:
  measure_1 / measure_8   th_measure_async of a 1-channel / an 8-channel program that reads every component of `self`:
                          "kernel" is the caller's kernel alone, on its own event pair (th_kernel_timing); "call" the kernel and
                          the library's fold, between two events on the context's stream (th_timer_start / _stop)
  stats                   th_stats_async of the same buffer (stats_kernel + stats_fold_kernel; a packed ring: through its f32
                          view, an unpack pass first), between two events on the stream - the fixed-function reduction
  memcpy_d2d              hipMemcpyAsync, device to device, of one ring buffer (as tools/program_bench.py does it)
Each figure is GPU ms per call over --reps calls after --warmup calls; the arms alternate for --rounds rounds, the median round
is reported with the range.  Registers, LDS and scratch of the programs' kernels (th_program_query) go out with the figures.

Usage: python tools/measure_program_bench.py [--size 4096] [--reps 20] [--warmup 3] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = (m.self.x + m.self.y) + (m.self.z * m.self.z + m.self.w * m.self.w);
    return s;
}
"""
EIGHT = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = m.self.x; s.v[1] = m.self.y; s.v[2] = m.self.z; s.v[3] = m.self.w;
    s.v[4] = m.self.z * m.self.z + m.self.w * m.self.w;
    s.v[5] = (float)(m.index & 1023u); s.v[6] = m.uv.x; s.v[7] = m.uv.y;
    return s;
}
"""
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("measure_program_bench: no GPU - nothing is measured without one")
    import numpy as np
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import MeasureProgram, Particles

    n = args.size
    progs = {1: MeasureProgram.from_source(ONE, channels=1, name="one"), 8: MeasureProgram.from_source(EIGHT, channels=8, name="eight")}
    rng = np.random.default_rng(1)
    band = np.empty((256, n, 4), np.float32)              # the same 256 rows all the way down: content is irrelevant to the time
    band[..., :2] = rng.uniform(-1, 1, (256, n, 2))
    band[..., 2:] = rng.uniform(-0.01, 0.01, (256, n, 2))
    rings = {}
    for name, fmt in (("f32", _capi.TH_STATE_F32), ("packed", _capi.TH_STATE_F16)):
        p = Particles(None, dict(shape=[n, n], stateFormat=fmt))
        p.setup(2)
        call("th_flow_resize", p._ctx, 1920, 1080)
        for y0 in range(0, n, 256):
            rows = min(256, n - y0)
            call("th_upload_state", p._ctx, 0, band.ctypes.data_as(_capi._fp), 0, y0, n, rows)
        rings[name] = p

    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def copy_arm(p, texel_bytes):
        stream, dst, src = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call("th_stream", p._ctx, C.byref(stream))
        call("th_state_device_ptr", p._ctx, 1, C.byref(dst))
        call("th_state_device_ptr", p._ctx, 0, C.byref(src))

        def copy():
            e = hip.hipMemcpyAsync(dst, src, n * n * texel_bytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
            if e:
                raise RuntimeError("hipMemcpyAsync: error %d" % e)
        return copy

    def measure_arm(p, prog):
        out = C.c_void_p()
        return lambda: call("th_measure_async", p._ctx, prog.handle, None, 0, 0, C.byref(out))

    def stats_arm(p):
        out = C.c_void_p()
        return lambda: call("th_stats_async", p._ctx, C.c_float(0.01), C.byref(out))

    # name -> (bytes read per call, bytes moved per call, context, the call, has a kernel of its own to time)
    arms = {}
    for ring, texel_bytes in (("f32", 16), ("packed", 8)):
        p = rings[ring]
        size = n * n * texel_bytes
        arms[ring + " measure_1"] = (size, p, measure_arm(p, progs[1]), True)
        arms[ring + " measure_8"] = (size, p, measure_arm(p, progs[8]), True)
        arms[ring + " stats"] = (size, p, stats_arm(p), False)
        arms[ring + " memcpy_d2d"] = (2 * size, p, copy_arm(p, texel_bytes), False)

    def timed(p, fn, reps, kernel):
        ms, kms, k = C.c_float(0), C.c_float(0), C.c_int32(0)
        if kernel:
            call("th_kernel_timing", p._ctx, 1)
        call("th_timer_start", p._ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", p._ctx, C.byref(ms))
        if kernel:
            call("th_kernel_timing_read", p._ctx, C.byref(kms), C.byref(k))
            call("th_kernel_timing", p._ctx, 0)
            assert k.value == reps, (k.value, reps)
        return ms.value / reps, kms.value

    for _, p, fn, kernel in arms.values():
        timed(p, fn, args.warmup, kernel)
    rounds = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (_, p, fn, kernel) in arms.items():
            rounds[name].append(timed(p, fn, args.reps, kernel))

    def row(values):
        return statistics.median(values), min(values), max(values)

    lines = ["measure programs, %d x %d particles, flow 1920 x 1080, %d rounds of %d calls, arms alternating; GPU ms per call"
             % (n, n, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "%-20s %-7s %10s %10s %10s %14s" % ("arm", "events", "median ms", "min ms", "max ms", "GB/s (median)")]
    result = dict(size=n, reps=args.reps, rounds=args.rounds, arms={}, query={})
    for name, (moved, _, _, kernel) in arms.items():
        med, lo, hi = row([r[0] for r in rounds[name]])
        result["arms"][name] = dict(call=dict(median_ms=med, min_ms=lo, max_ms=hi), bytes=moved)
        lines.append("%-20s %-7s %10.4f %10.4f %10.4f %14.1f" % (name, "call", med, lo, hi, moved / med / 1e6))
        if kernel:
            med, lo, hi = row([r[1] for r in rounds[name]])
            result["arms"][name]["kernel"] = dict(median_ms=med, min_ms=lo, max_ms=hi)
            lines.append("%-20s %-7s %10.4f %10.4f %10.4f %14.1f" % (name, "kernel", med, lo, hi, moved / med / 1e6))
    for ring in ("f32", "packed"):
        a, s = result["arms"][ring + " measure_1"]["call"], result["arms"][ring + " stats"]["call"]
        lines.append("%s: measure_1 / stats = %.3f (calls, median; rounds' range of measure_1 %.4f ms, of stats %.4f ms)"
                     % (ring, a["median_ms"] / s["median_ms"], a["max_ms"] - a["min_ms"], s["max_ms"] - s["min_ms"]))
    for ring, p in rings.items():
        for channels, prog in progs.items():
            info = prog.query(p)
            result["query"]["%s measure_%d" % (ring, channels)] = info
            lines.append("th_program_query(%d channel%s): %s   (th_measure_kernel; the packed ring runs th_measure_packed_kernel of the same module)"
                         % (channels, "" if channels == 1 else "s", json.dumps(info)))
        break
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for p in rings.values():
        p.dispose()
    for prog in progs.values():
        prog.dispose()


if __name__ == "__main__":
    main()
