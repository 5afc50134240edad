"""Capture the reference's own colour-map blend (Blend / AudioTexture of its compiled demo bundle) into tests/golden/blend_*.npz.

Runs only where the reference checkout and kaleido (headless Chromium + SwiftShader, WebGL 1 with float render targets)
are present.  The reference's bundle is read at run time, joined with tools/capture_blend.js in a temporary directory and
never written into this repository.  Every case builds its views from the reference's own objects - AudioTexture(gl, n)
filled through waveform() / frequencies() / assign() + apply(), gl-fbo objects with and without {float: true} - and runs
Blend.draw(target, undefined, clear) into a float gl-fbo of the target's shape, with the GL state Tendrils.step() leaves
behind (BLEND, SRC_ALPHA / ONE_MINUS_SRC_ALPHA) or the context's initial one.

Each fixture holds (meta JSON under "uniforms", as tests/helpers.py:load reads it):
  tex<k>                     texture k: [n] f32 (an AudioTexture's array as the reference mapped it), [h,w,4] u8 or [h,w,4] f32
  raw<k>                     (audio textures) the analyser bytes [n] u8 - or floats, map "assign" - the reference's map was given
  views [V] i32, alphas [V] f32      the blend's views (indices of textures, a texture may be named twice) and alphas
  prefill [H,W,4] f32        (clear = false only) the target before the draw
  out [H,W,4] f32            the target after Blend.draw
  meta: target [W,H], glBlend, clear, formats / maps / shapes per texture, floatBlend

Usage: python tools/capture_blend.py [--out tests/golden] [--check]   (--check: compare with the committed files)
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


def _b64(a, dtype):
    return base64.b64encode(np.ascontiguousarray(a, dtype=dtype).tobytes()).decode()


def _f32(s):
    return np.frombuffer(base64.b64decode(s), dtype=np.float32).copy()


class Runner:
    """The demo bundle with its bootstrap handing out the module loader (the same one-token change of the webpack
    prologue the flow lines' capture makes), followed by the capture harness."""

    def __init__(self):
        from kaleido.scopes.plotly import PlotlyScope
        self._tmp = tempfile.mkdtemp(prefix="tendrils_blend_")
        with open(os.path.join(REF, "docs/js/demo.js")) as f:
            text = f.read()
        boot = 't.p="",t(0)}(['
        assert text.find(boot) == 405
        text = text.replace(boot, 't.p="",t}([', 1)
        with open(os.path.join(HERE, "capture_blend.js")) as f:
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
def audio(rng, n, how):
    """analyser bytes for an AudioTexture of n bins, to go through the reference's `how` map"""
    return dict(type="audio", n=n, map=how, data=rng.integers(0, 256, n, dtype=np.uint8))


def audio_floats(rng, n, lo, hi):
    return dict(type="audio", n=n, map="assign", data=rng.uniform(lo, hi, n).astype(np.float32))


def rgba8(rng, w, h):
    return dict(type="rgba8", w=w, h=h, data=rng.integers(0, 256, (h, w, 4), dtype=np.uint8))


def rgba32f(rng, w, h, lo=0.0, hi=1.0):
    return dict(type="rgba32f", w=w, h=h, data=rng.uniform(lo, hi, (h, w, 4)).astype(np.float32))


def cases():
    rng = np.random.default_rng(20261018)
    out = []
    mic, track, video = audio(rng, 8, "frequencies"), audio(rng, 16, "waveform"), rgba8(rng, 12, 10)
    demo = dict(textures=[mic, track, video], views=[0, 1, 2], alphas=[0.1, 0.3, 0.8], clear=True)
    out.append(dict(demo, name="demo_24x16", target=(24, 16), gl_blend=True))
    out.append(dict(demo, name="first_frame_24x16", target=(24, 16), gl_blend=False))
    image = rgba32f(rng, 5, 7)
    out.append(dict(name="unit_target_1x1", target=(1, 1), gl_blend=True, clear=True,
                    textures=[mic, image, video], views=[0, 1, 2], alphas=[0.1, 0.3, 0.8]))
    wide = rgba32f(rng, 5, 7, -0.5, 1.75)          # float texels above 1 and below 0
    frame = rgba8(rng, 40, 30)
    dot = rgba32f(rng, 1, 1)
    out.append(dict(name="npot_17x9", target=(17, 9), gl_blend=True, clear=True,
                    textures=[wide, frame, dot], views=[0, 1, 2], alphas=[1.5, 0.6, -0.25]))
    prefill = rng.uniform(-0.25, 1.25, (9, 17, 4)).astype(np.float32)
    out.append(dict(name="noclear_17x9", target=(17, 9), gl_blend=True, clear=False, prefill=prefill,
                    textures=[image, frame, track], views=[0, 1, 2], alphas=[0.4, 0.25, 0.2]))
    eight = [audio(rng, 8, "frequencies"), rgba8(rng, 7, 3), rgba32f(rng, 3, 5), audio_floats(rng, 32, -1.0, 1.0),
             rgba8(rng, 26, 22), rgba32f(rng, 13, 11)]
    out.append(dict(name="eight_views_13x11", target=(13, 11), gl_blend=True, clear=True, textures=eight,
                    views=[0, 1, 2, 3, 0, 4, 5, 3], alphas=[0.1, 0.2, 0.15, 0.05, 0.12, 0.3, 0.25, 0.08]))
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


def job_of(case):
    w, h = case["target"]
    texs = []
    for t in case["textures"]:
        if t["type"] == "audio":
            texs.append({"type": "audio", "n": t["n"], "map": t["map"],
                         "data": _b64(t["data"], np.float32 if t["map"] == "assign" else np.uint8)})
        else:
            texs.append({"type": t["type"], "w": t["w"], "h": t["h"],
                         "data": _b64(t["data"], np.uint8 if t["type"] == "rgba8" else np.float32)})
    return {"kind": "blend", "targetW": w, "targetH": h, "alphas": [float(a) for a in case["alphas"]],
            "glBlend": bool(case["gl_blend"]), "clear": bool(case["clear"]),
            "prefill": None if case.get("prefill") is None else _b64(case["prefill"], np.float32),
            "textures": texs, "views": [int(v) for v in case["views"]]}


def capture(runner, case):
    w, h = case["target"]
    res = runner.run(job_of(case))
    assert res["blendEnabled"] == bool(case["gl_blend"]) and res["resolution"] == [w, h], res
    arrs = {"out": _f32(res["out"]).reshape(h, w, 4), "views": np.array(case["views"], np.int32),
            "alphas": np.array(case["alphas"], np.float32)}
    if case.get("prefill") is not None:
        arrs["prefill"] = case["prefill"]
    for k, t in enumerate(case["textures"]):
        if t["type"] == "audio":
            arrs["raw%d" % k] = t["data"]
            arrs["tex%d" % k] = _f32(res["arrays"][k])
            assert len(arrs["tex%d" % k]) == t["n"]
        else:
            arrs["tex%d" % k] = t["data"]
    meta = {"target": [w, h], "glBlend": bool(case["gl_blend"]), "clear": bool(case["clear"]),
            "formats": [t["type"] for t in case["textures"]], "maps": [t.get("map") for t in case["textures"]],
            "shapes": res["shapes"], "floatBlend": res["floatBlend"]}
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
        path = os.path.join(a.out, "blend_%s.npz" % case["name"])
        if a.check:
            tmp = os.path.join(runner._tmp, "check.npz")
            data = write_npz(tmp, arrs)
            same = os.path.exists(path) and open(path, "rb").read() == data
            bad += not same
            print("%-40s %s" % (os.path.basename(path), "identical" if same else "DIFFERS"))
        else:
            os.makedirs(a.out, exist_ok=True)
            data = write_npz(path, arrs)
            print("wrote %-36s %7.1f KiB" % (os.path.basename(path), len(data) / 1024))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
