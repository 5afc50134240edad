"""Capture the reference's own flow lines (FlowLine / FlowLines of its compiled demo bundle) into tests/golden/flowline_*.npz.

Runs only where the reference checkout and kaleido (headless Chromium + SwiftShader, WebGL 1 with float render targets)
are present.  The reference's bundle is read at run time, joined with tools/capture_flow_lines.js in a temporary
directory and never written into this repository.  Every case drives FlowLines.get(id, {closed}) / FlowLine.add(), then
for each line of `active` in its own order: the uniforms, update(), draw() into an RGBA32F framebuffer of the flow's
shape with SRC_ALPHA / ONE_MINUS_SRC_ALPHA blending (as Tendrils.step() leaves it).

Each fixture holds (meta JSON under "uniforms", as tests/helpers.py:load reads it):
  points [P,2] f32, times [P] f64, offsets [L+1] i32, closed [L] i32   the lines in creation order (ids in meta)
  flow0 [H,W,4] f32 (only when the initial field is not zero)
  a_<name>, a_offsets                                                   the attribute arrays after update(), draw order
  idx [K] i32, val [K,4] f32                                            covered texels and the flow there after draw()
Coverage is the union of the texels draw() changed over the given field and over a constant field of 7s.

Usage: python tools/capture_flow_lines.py [--out tests/golden] [--check]   (--check: compare with the committed files)
"""
import argparse
import base64
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

REF = os.environ.get("TENDRILS_REFERENCE", "/root/reference")      # the reference checkout (as oracle/ref_runner.py)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ATTRS = ("position", "normal", "miter", "previous", "time", "dt")
ASIZE = {"position": 2, "normal": 2, "miter": 1, "previous": 2, "time": 1, "dt": 1}
DEFAULT_UNIFORMS = {"speed": 3.0, "rad": 0.1, "crestShape": 0.6, "speedLimit": 0.01, "viewSize": [1.0, 1.0]}


def _b64(a, dtype):
    return base64.b64encode(np.ascontiguousarray(a, dtype=dtype).tobytes()).decode()


def _f32(s):
    return np.frombuffer(base64.b64decode(s), dtype=np.float32).copy()


class Runner:
    """The demo bundle with its bootstrap handing out the module loader (the same one-token change of the webpack
    prologue the fixture generator under oracle/ makes), followed by the capture harness."""

    def __init__(self):
        from kaleido.scopes.plotly import PlotlyScope
        self._tmp = tempfile.mkdtemp(prefix="tendrils_flowline_")
        with open(os.path.join(REF, "docs/js/demo.js")) as f:
            text = f.read()
        boot = 't.p="",t(0)}(['
        assert text.find(boot) == 405
        text = text.replace(boot, 't.p="",t}([', 1)
        with open(os.path.join(HERE, "capture_flow_lines.js")) as f:
            harness = f.read()
        stub = os.path.join(self._tmp, "stub.js")
        with open(stub, "w") as f:
            f.write(text + "\n" + harness)
        self._scope = PlotlyScope(plotlyjs="file://" + stub)

    def run(self, job):
        raw = self._scope.transform({"data": [], "layout": {"job": job}}, format="svg")
        res = json.loads(raw.decode())
        if "error" in res:
            raise RuntimeError("capture harness: %s\n%s" % (res["error"], res.get("stack")))
        if res.get("err"):
            raise RuntimeError("GL error %s" % res["err"])
        return res


# ---- the cases ---------------------------------------------------------------------------------------------------------
def stroke(rng, n, start, step, turn=0.25, t0=5000.0, dt=16.7, jitter=3.0):
    """A pointer-like stroke: n f32 points from `start`, each about `step` NDC from the last, heading wandering by up to
    `turn` rad per point; times dt ms apart with jitter."""
    pts, ang = [np.array(start, np.float64)], rng.uniform(0, 2 * np.pi)
    for _ in range(n - 1):
        ang += rng.uniform(-turn, turn)
        pts.append(pts[-1] + step * rng.uniform(0.6, 1.4) * np.array([np.cos(ang), np.sin(ang)]))
    times = t0 + np.cumsum(np.r_[0.0, dt + rng.uniform(-jitter, jitter, n - 1)])
    return np.array(pts, np.float32), times


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    a_pts, a_t = stroke(rng, 12, (-0.5, -0.2), 0.06)
    out.append(dict(name="open_160x90", shape=(160, 90), lines=[(1, False, a_pts, a_t)]))
    field = np.zeros((90, 160, 4), np.float32)
    field[..., :2] = rng.uniform(-0.01, 0.01, (90, 160, 2))
    field[..., 2] = rng.uniform(4000.0, 5000.0, (90, 160))
    field[..., 3] = rng.uniform(0.0, 1.0, (90, 160))
    out.append(dict(name="over_field_160x90", shape=(160, 90), lines=[(1, False, a_pts, a_t)], flow0=field))
    ang = np.linspace(0, 2 * np.pi, 9)[:-1]
    ring = np.stack([0.45 * np.cos(ang) + 0.1, 0.6 * np.sin(ang)], 1).astype(np.float32)
    out.append(dict(name="closed_160x90", shape=(160, 90), lines=[(2, True, ring, 6000.0 + 16.0 * np.arange(8))]))
    sharp = np.array([[-0.7, -0.5], [-0.3, -0.1], [0.1, 0.3], [-0.2, 0.32], [-0.55, 0.36], [0.4, -0.6]], np.float32)
    out.append(dict(name="sharp_turn_160x90", shape=(160, 90), lines=[(0, False, sharp, 7000.0 + 20.0 * np.arange(6))],
                    uniforms={"speedLimit": 0.02}))
    off = np.array([[-1.3, 0.2], [-0.9, 0.25], [-0.5, 0.9], [-0.2, 1.4], [0.3, 0.8], [0.8, 0.5], [1.25, -0.2],
                    [0.9, -1.3]], np.float32)
    out.append(dict(name="offscreen_160x90", shape=(160, 90), lines=[(5, False, off, 8000.0 + 17.0 * np.arange(8))],
                    uniforms={"rad": 0.15}))
    b_pts, b_t = stroke(rng, 10, (0.3, 0.4), 0.05)
    c_pts, c_t = stroke(rng, 9, (0.0, -0.1), 0.07)
    out.append(dict(name="two_lines_160x90", shape=(160, 90), lines=[(7, False, b_pts, b_t), (3, False, c_pts, c_t)]))
    d_pts, d_t = stroke(rng, 14, (-0.3, 0.3), 0.05)
    out.append(dict(name="npot_97x61", shape=(97, 61), lines=[(1, False, d_pts, d_t)],
                    uniforms={"speed": 2.0, "rad": 0.12, "crestShape": 0.3, "viewSize": [0.8, 1.0]}))
    big = []
    for i, (sx, sy) in enumerate([(-0.6, -0.4), (0.2, 0.5), (0.5, -0.5)]):
        p, t = stroke(rng, 16, (sx, sy), 0.04, t0=9000.0 + 5.0 * i)
        big.append((i + 1, False, p, t))
    out.append(dict(name="large_480x270", shape=(480, 270), lines=big, uniforms={"viewSize": [0.5625, 1.0]}))
    eq = np.array([[-0.5, 0.0], [-0.3, 0.1], [-0.3, 0.1], [0.0, 0.05], [0.2, -0.1], [0.45, -0.05]], np.float32)
    out.append(dict(name="equal_points_160x90", shape=(160, 90), lines=[(1, False, eq, 9500.0 + 16.0 * np.arange(6))]))
    return out


# ---- writing ---------------------------------------------------------------------------------------------------------
def write_npz(path, arrs):
    """np.load-compatible npz with fixed member dates, so that regenerating gives the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    data = buf.getvalue()
    with open(path, "wb") as f:
        f.write(data)
    return data


def job_of(case, flow0):
    w, h = case["shape"]
    uni = dict(DEFAULT_UNIFORMS, **case.get("uniforms", {}))
    return {"kind": "flowline", "flowW": w, "flowH": h, "flow": None if flow0 is None else _b64(flow0, np.float32),
            "uniforms": uni, "trim": case.get("trim"),
            "lines": [{"id": lid, "closed": bool(cl), "points": [[float(x), float(y)] for x, y in pts],
                       "times": [float(t) for t in ts]} for lid, cl, pts, ts in case["lines"]]}


def capture(runner, case):
    w, h = case["shape"]
    flow0 = case.get("flow0")
    base = flow0 if flow0 is not None else np.zeros((h, w, 4), np.float32)
    res = runner.run(job_of(case, flow0))
    got = _f32(res["out"]).reshape(h, w, 4)
    sevens = np.full((h, w, 4), 7.0, np.float32)
    res7 = runner.run(job_of(case, sevens))
    got7 = _f32(res7["out"]).reshape(h, w, 4)
    changed = (got.view(np.uint32) != base.view(np.uint32)).any(-1) | (got7.view(np.uint32) != sevens.view(np.uint32)).any(-1)
    idx = np.flatnonzero(changed.ravel()).astype(np.int32)
    pts = np.concatenate([l[2] for l in case["lines"]]).astype(np.float32)
    tms = np.concatenate([np.asarray(l[3], np.float64) for l in case["lines"]])
    offs = np.cumsum([0] + [len(l[2]) for l in case["lines"]]).astype(np.int32)
    arrs = {"points": pts, "times": tms, "offsets": offs, "closed": np.array([int(l[1]) for l in case["lines"]], np.int32),
            "idx": idx, "val": got.reshape(-1, 4)[idx]}
    if flow0 is not None:
        arrs["flow0"] = flow0.astype(np.float32)
    per = {k: [] for k in ATTRS}
    aoff = [0]
    for a in res["attrs"]:
        for k in ATTRS:
            per[k].append(_f32(a[k]).reshape(-1, ASIZE[k]) if ASIZE[k] > 1 else _f32(a[k]))
        aoff.append(aoff[-1] + len(per["miter"][-1]))
    for k in ATTRS:
        arrs["a_" + k] = np.concatenate(per[k]) if per[k] else np.zeros((0,) + ((ASIZE[k],) if ASIZE[k] > 1 else ()), np.float32)
    arrs["a_offsets"] = np.array(aoff, np.int32)
    meta = {"flowShape": [w, h], "uniforms": dict(DEFAULT_UNIFORMS, **case.get("uniforms", {})),
            "ids": [l[0] for l in case["lines"]], "order": res["order"], "floatBlend": res["floatBlend"],
            "samples": res["samples"]}
    arrs["uniforms"] = np.array(json.dumps(meta, sort_keys=True))
    return arrs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the files in --out")
    a = ap.parse_args(argv)
    runner = Runner()
    bad = 0
    for case in cases():
        arrs = capture(runner, case)
        path = os.path.join(a.out, "flowline_%s.npz" % case["name"])
        if a.check:
            tmp = os.path.join(runner._tmp, "check.npz")
            data = write_npz(tmp, arrs)
            same = os.path.exists(path) and open(path, "rb").read() == data
            bad += not same
            print("%-40s %s" % (os.path.basename(path), "identical" if same else "DIFFERS"))
        else:
            os.makedirs(a.out, exist_ok=True)
            data = write_npz(path, arrs)
            print("wrote %-36s %7.1f KiB  %d covered texels" % (os.path.basename(path), len(data) / 1024, len(arrs["idx"])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
