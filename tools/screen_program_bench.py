"""GPU time of a screen program's pass (tendrils_amd/csrc/th_screen.hip, th_screen_prelude.inc) against the library's own kernel
for the same job, on one MI355X.

Arms, all in this process, on one context with a 1920 x 1080 view (RGBA8 images of 7.9 MiB) and one view buffer; the screen
is bound and every pass reads buffers[0]:
  view_copy      th_view_copy(0): the library's copy kernel (source read, destination read, destination written: 12 B a texel)
  copy_blend     a copy program (th_tex at uv), gl_blend = 1 (the same 12 B a texel)
  copy_store     the same program, gl_blend = 0 (source read, destination written: 8 B a texel)
  box9           a 3 x 3 box through th_texel, gl_blend = 0 (8 B a texel must move; the other eight taps are neighbours' texels)
  gather20       20 taps at fixed pseudo-random offsets within 9 texels, gl_blend = 0 (8 B a texel must move) - the access
                 pattern of a scattered blur
Each figure is the GPU time per call between two events on the context's stream (th_timer_start / th_timer_stop around
--reps calls, after --warmup calls); the arms alternate for --rounds rounds and the median round is reported, with the
spread, and as the bandwidth the bytes a pass MUST move would need.  Every program's registers / scratch / code size
(th_program_query) go out with the figures.

Usage: python tools/screen_program_bench.py [--width 1920] [--height 1080] [--reps 50] [--warmup 5] [--rounds 5] [--out profiles/screen_program.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY = """__device__ float4 th_screen(const th_screen_pass &s)
{
    return th_tex(s, 0, s.uv.x, s.uv.y);
}
"""

BOX9 = """__device__ float4 th_screen(const th_screen_pass &s)
{
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const float4 t = th_texel(s, 0, s.x + dx, s.y + dy);
            a = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
        }
    const float k = 1.0f / 9.0f;
    return make_float4(a.x * k, a.y * k, a.z * k, a.w * k);
}
"""


def gather_source(taps=20, radius=9, seed=20):
    """`taps` offsets inside a disc of `radius` texels, drawn once from a seeded generator and written into the source"""
    import random
    rng = random.Random(seed)
    offsets = []
    while len(offsets) < taps:
        dx, dy = rng.randint(-radius, radius), rng.randint(-radius, radius)
        if dx * dx + dy * dy <= radius * radius and (dx, dy) not in offsets:
            offsets.append((dx, dy))
    table = ", ".join("{%d, %d}" % o for o in offsets)
    return """__device__ float4 th_screen(const th_screen_pass &s)
{
    const int taps[%d][2] = {%s};
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < %d; ++k) {
        const float4 t = th_texel(s, 0, s.x + taps[k][0], s.y + taps[k][1]);
        a = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
    }
    const float w = 1.0f / %d.0f;
    return make_float4(a.x * w, a.y * w, a.z * w, a.w * w);
}
""" % (taps, table, taps, taps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("screen_program_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import ScreenProgram
    from tendrils_amd.sharding import device_view
    from tendrils_amd.tendrils import View

    w, h = args.width, args.height
    programs = dict(copy=ScreenProgram.from_source(COPY, name="copy"), box9=ScreenProgram.from_source(BOX9, name="box9"),
                    gather20=ScreenProgram.from_source(gather_source(), name="gather20"))
    t = ta.Tendrils(View(w, h), dict(numBuffers=1))
    t.resize()
    t.setup(8)
    ctx = t.particles._ctx
    # a picture with every alpha in it: the blend's arithmetic runs on what a frame would hold
    for image in (t.buffers[0], None):
        t._bind_view(image)
        ptr = C.c_void_p()
        call("th_view_device_ptr", ctx, C.byref(ptr))
        call("th_sync", ctx)
        device_view(ptr.value, (w * h, 4), "|u1").copy_(torch.randint(0, 256, (w * h, 4), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
    t._bind_view(None)
    unit = (_capi.ScreenUnit * 1)()
    unit[0].source, unit[0].index = _capi.VIEW_BUFFER, 0

    def run(name, gl_blend):
        return lambda: call("th_screen_run", ctx, programs[name].handle, None, 0, unit, 1, _capi.SCREEN_TARGET_VIEW, 0, gl_blend)

    texels = w * h
    # (bytes a call must move, the call)
    arms = {
        "view_copy": (12 * texels, lambda: call("th_view_copy", ctx, 0)),
        "copy_blend": (12 * texels, run("copy", 1)),
        "copy_store": (8 * texels, run("copy", 0)),
        "box9": (8 * texels, run("box9", 0)),
        "gather20": (8 * texels, run("gather20", 0)),
    }

    def timed(fn, reps):
        ms = C.c_float(0)
        call("th_timer_start", ctx)
        for _ in range(reps):
            fn()
        call("th_timer_stop", ctx, C.byref(ms))
        return ms.value / reps

    for _, fn in arms.values():
        timed(fn, args.warmup)
    rounds = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (_, fn) in arms.items():
            rounds[name].append(timed(fn, args.reps))

    queries = {name: p.query(t.particles) for name, p in programs.items()}
    lines = ["screen program pass into the screen from buffers[0], %d x %d texels (RGBA8), %d rounds of %d calls, arms alternating; GPU ms per call (events on the context's stream)"
             % (w, h, args.rounds, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "%-12s %10s %10s %10s %14s" % ("arm", "median ms", "min ms", "max ms", "GB/s (median)")]
    result = dict(width=w, height=h, reps=args.reps, rounds=args.rounds, query=queries, arms={})
    for name, (moved, _) in arms.items():
        ms = rounds[name]
        med = statistics.median(ms)
        result["arms"][name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), bytes=moved, gbps=moved / med / 1e6)
        lines.append("%-12s %10.4f %10.4f %10.4f %14.1f" % (name, med, min(ms), max(ms), moved / med / 1e6))
    lines.append("copy_blend / view_copy = %.3f (time ratio; bytes are the same)"
                 % (result["arms"]["copy_blend"]["median_ms"] / result["arms"]["view_copy"]["median_ms"]))
    for name, info in queries.items():
        lines.append("th_program_query(%s): %s" % (name, json.dumps(info)))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    t.dispose()
    for p in programs.values():
        p.dispose()


if __name__ == "__main__":
    main()
