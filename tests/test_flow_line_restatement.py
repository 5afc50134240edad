"""The numpy restatement of flow-line drawing (tests/flowline_restatement.py) against the reference's own captures
(tests/golden/flowline_*.npz).  CPU only.

Coverage - which texels receive fragments - must match texel for texel.  Values within the deposit tolerance of
tests/test_deposit_oracle.py, except x and y: the captured rasteriser interpolates from the snapped vertices with
arithmetic of its own, and the measured maximum deviation over these captures is 4.77e-7 (y, closed_160x90; the
others stay below 1.5e-7), so xy are held to 4.8e-7 instead of 5e-8.  Measured maxima per channel: x 1.43e-7,
y 4.77e-7, z (time, ms) 6.8e-3 with times ~ 7000 (the 1e-6 bound relative to the strokes' times), alpha 1.01e-6."""
import numpy as np
import pytest

import flowline_restatement as R
from helpers import golden, load

XY_TOL = 4.8e-7


def flowline_close(got, ref, time):
    """time: the scale of the strokes' times (ms), as the deposit tolerance's `time`"""
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ok = (d[..., 0] <= XY_TOL) & (d[..., 1] <= XY_TOL) & (d[..., 2] <= 1e-6 * abs(time) + 1e-6) & (d[..., 3] <= 1e-5)
    return ok | (np.isnan(got) & np.isnan(ref)).all(-1)


def fixture_case(path):
    """(meta, initial flow, expected flow, covered mask, lines as (points, times, closed) in draw order)"""
    fx = load(path)
    m = fx["meta"]
    w, h = m["flowShape"]
    base = fx["flow0"] if "flow0" in fx else np.zeros((h, w, 4), np.float32)
    ref = base.copy().reshape(-1, 4)
    ref[fx["idx"]] = fx["val"]
    cov = np.zeros(w * h, bool)
    cov[fx["idx"]] = True
    ids = [str(i) for i in m["ids"]]
    lines = []
    for oid in m["order"]:
        i = ids.index(oid)
        a, b = fx["offsets"][i], fx["offsets"][i + 1]
        lines.append((fx["points"][a:b], fx["times"][a:b], bool(fx["closed"][i])))
    return m, base, ref.reshape(h, w, 4), cov.reshape(h, w), lines


def restated(base, lines, uniforms):
    from tendrils_amd import flow_line as FL
    got = base.copy()
    cov = np.zeros(got.shape[:2], np.int64)
    R.draw(got, [FL.attributes(*l) for l in lines], uniforms, cov)
    return got, cov


@pytest.mark.parametrize("path", golden("flowline"), ids=lambda p: p.split("/")[-1][:-4])
def test_restatement_matches_reference_capture(path):
    m, base, ref, cov_ref, lines = fixture_case(path)
    assert m["floatBlend"] and m["samples"] == 0
    got, cov = restated(base, lines, m["uniforms"])
    assert ((cov > 0) == cov_ref).all(), "coverage differs in %d texels" % ((cov > 0) != cov_ref).sum()
    ok = flowline_close(got, ref, max(np.abs(l[1]).max() for l in lines))
    assert ok.all(), "%d texels out of tolerance; max dev %s" % ((~ok).sum(), np.abs(got.astype(np.float64) - ref).reshape(-1, 4).max(0))
    untouched = ~cov_ref
    assert (got[untouched].view(np.uint32) == base[untouched].view(np.uint32)).all()
