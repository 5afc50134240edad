"""GPU time of th_flow_lines on a 1920 x 1080 flow (tendrils_amd/csrc/th_flowline.hip).

Two sizes: the demo's (4 strokes x 12 points) and a stress size (256 strokes x 64 points, ~32 k triangles), pointer-like
speeds.  For each: triangles, covered fragments (the numpy restatement's count on the demo size; the HIP path's own
output otherwise: texels whose value changed), flow bytes touched (32 B per covered texel: one read, one write) and the
GPU time per call (th_timer_start / th_timer_stop on the context's stream, median of --reps calls after --warmup).  The
comparison arm (--naive) runs the same calls with TH_FLOWLINE_NAIVE=1 (every texel walks every triangle, as the
GeometrySpawner's fill) in a child process, on the demo size and on a smaller stress case.

Usage: python tools/flow_line_bench.py [--reps 50] [--warmup 5] [--naive] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def strokes(seed, nlines, npts, step=0.03):
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(nlines):
        p = [rng.uniform(-0.8, 0.8, 2)]
        ang = rng.uniform(0, 2 * np.pi)
        for _ in range(npts - 1):
            ang += rng.uniform(-0.3, 0.3)
            p.append(p[-1] + step * rng.uniform(0.5, 1.5) * np.array([np.cos(ang), np.sin(ang)]))
        t = 5000.0 + 16.7 * np.arange(npts)
        lines.append((np.array(p, np.float32), t, False))
    return lines


def run(size, lines, reps, warmup):
    import tendrils_amd as ta
    from tendrils_amd import _capi, flow_line as FL
    from tendrils_amd.tendrils import View
    w, h = 1920, 1080
    t = ta.Tendrils(View(w, h))
    t.resize()
    t.setup(16)
    t.flow.shape = [w, h]
    base = np.zeros((h, w, 4), np.float32)
    t.flow.set_pixels(base)
    u = FL.defaults()
    u["viewSize"] = [h / w, 1.0]
    ctx = t.particles._ctx
    FL.draw_lines(ctx, u, lines)
    once = t.flow.read()
    covered = int((once != 0).any(-1).sum())
    # the call alone: arguments packed once (what FL.draw_lines packs per call)
    pts = np.ascontiguousarray(np.concatenate([p for p, _, _ in lines]), np.float32)
    tms = np.ascontiguousarray(np.concatenate([t for _, t, _ in lines]), np.float64)
    offs = np.ascontiguousarray(np.cumsum([0] + [len(t) for _, t, _ in lines]), np.int32)
    closed = np.zeros(len(lines), np.int32)
    ip = C.POINTER(C.c_int32)
    args = (ctx, C.byref(FL.uniforms_struct(u)), pts.ctypes.data_as(_capi._fp), tms.ctypes.data_as(C.POINTER(C.c_double)),
            offs.ctypes.data_as(ip), closed.ctypes.data_as(ip), len(lines))
    times = []
    for k in range(warmup + reps):
        _capi.call("th_timer_start", ctx)
        _capi.call("th_flow_lines", *args)
        ms = C.c_float(0)
        _capi.call("th_timer_stop", ctx, C.byref(ms))
        if k >= warmup:
            times.append(ms.value)
    t.dispose()
    tri = sum(2 * len(p) - 2 for p, _, _ in lines)
    return {"size": size, "strokes": len(lines), "points": int(sum(len(p) for p, _, _ in lines)), "triangles": tri,
            "covered_texels": covered, "flow_bytes_touched": 32 * covered,
            "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)),
            "naive": os.environ.get("TH_FLOWLINE_NAIVE") == "1"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--naive", action="store_true", help="also run the per-texel comparison arm (child process)")
    ap.add_argument("--arm", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    cases = {"demo": (1, 4, 12), "stress": (2, 256, 64), "stress_small": (3, 32, 64)}
    names = a.arm.split(",") if a.arm else ["demo", "stress"]
    out = []
    for name in names:
        seed, n, m = cases[name]
        r = run(name, strokes(seed, n, m), a.reps, a.warmup)
        print(json.dumps(r))
        out.append(r)
    if a.naive and not a.arm:
        env = dict(os.environ, TH_FLOWLINE_NAIVE="1")
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", "demo,stress_small", "--reps", str(max(3, a.reps // 10)),
                              "--warmup", "1"], env=env, capture_output=True, text=True, timeout=1200)
        sys.stdout.write(res.stdout)
        if res.returncode != 0:
            sys.stderr.write(res.stderr)
            return res.returncode
        out += [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
        binned_small = run("stress_small", strokes(3, 32, 64), a.reps, a.warmup)
        print(json.dumps(binned_small))
        out.append(binned_small)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
