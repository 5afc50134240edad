"""GPU time of a user program's pass (tendrils_amd/csrc/th_program.hip) against what bounds it, on one MI355X.

Arms, all in this process, at 4096 x 4096 texels (a 256 MiB RGBA32F ring buffer):
  identity         th_program_run of `return p.self;` from buffers[1] into buffers[0] (256 MiB read + 256 MiB written)
  identity_packed  the same program on a TH_STATE_F16 ring (128 MiB buffers: unpack to f32 staging, the pass, pack again)
  memcpy_d2d       hipMemcpyAsync, device to device, buffers[1] -> buffers[0] of the f32 ring on the context's stream
  spawn_init       th_spawn_init's fill of buffers[0] (256 MiB written, nothing read)
Each figure is the GPU time per call between two events on the context's stream (th_timer_start / th_timer_stop around
--reps calls, after --warmup calls); the arms alternate for --rounds rounds and the median round is reported, with the
spread.  The program's registers / scratch / code size (th_program_query) go out with the figures.

Usage: python tools/program_bench.py [--size 4096] [--reps 20] [--warmup 3] [--rounds 5] [--out profiles/user_program.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IDENTITY = """__device__ float4 th_main(const th_pass &p)
{
    return p.self;
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
        sys.exit("program_bench: no GPU - nothing is measured without one")
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import Particles, Program

    n = args.size
    prog = Program.from_source(IDENTITY, name="identity")
    f32 = Particles(None, dict(shape=[n, n]))
    f32.setup(2)
    packed = Particles(None, dict(shape=[n, n], stateFormat=_capi.TH_STATE_F16))
    packed.setup(2)
    for p in (f32, packed):
        call("th_spawn_init", p._ctx, 1)

    # the process's one HIP runtime (the copy _capi.load() settled on), for the copy arm
    runtime, = _capi._mapped("libamdhip64")
    hip = C.CDLL(runtime)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream, dst, src = C.c_void_p(), C.c_void_p(), C.c_void_p()
    call("th_stream", f32._ctx, C.byref(stream))
    call("th_state_device_ptr", f32._ctx, 0, C.byref(dst))
    call("th_state_device_ptr", f32._ctx, 1, C.byref(src))
    nbytes = n * n * 16

    def run_program(p):
        return lambda: call("th_program_run", p._ctx, prog.handle, None, 0, _capi.TH_SOURCE_NONE, 0)

    def copy():
        e = hip.hipMemcpyAsync(dst, src, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
        if e:
            raise RuntimeError("hipMemcpyAsync: error %d" % e)

    # (bytes moved per call, context whose stream times it, the call)
    arms = {
        "identity": (2 * nbytes, f32, run_program(f32)),
        "identity_packed": (2 * nbytes // 2, packed, run_program(packed)),
        "memcpy_d2d": (2 * nbytes, f32, copy),
        "spawn_init": (nbytes, f32, lambda: call("th_spawn_init", f32._ctx, 0)),
    }

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

    info = prog.query(f32)
    lines = ["user program pass, %d x %d texels, %d rounds of %d calls, arms alternating; GPU ms per call (events on the context's stream)"
             % (n, n, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "%-16s %10s %10s %10s %12s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    result = dict(size=n, reps=args.reps, rounds=args.rounds, query=info, arms={})
    for name, (moved, _, _) in arms.items():
        ms = rounds[name]
        med = statistics.median(ms)
        result["arms"][name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), bytes=moved, gbps=moved / med / 1e6)
        lines.append("%-16s %10.4f %10.4f %10.4f %12.1f" % (name, med, min(ms), max(ms), moved / med / 1e6))
    lines.append("identity / memcpy_d2d = %.3f (time ratio; bytes are the same)"
                 % (result["arms"]["identity"]["median_ms"] / result["arms"]["memcpy_d2d"]["median_ms"]))
    lines.append("th_program_query(identity): " + json.dumps(info))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for p in (f32, packed):
        p.dispose()
    prog.dispose()


if __name__ == "__main__":
    main()
