"""Flow lines on the host side (CPU only): th_flow_line_attributes against the reference's own attribute arrays
(tests/golden/flowline_*.npz, tools/capture_flow_lines.py) bit for bit, the FlowLine / FlowLines bookkeeping of
src/flow-line/index.js and multi.js, and argument errors of the two entry points."""
import ctypes as C

import numpy as np
import pytest

from helpers import golden, load

FIXTURES = golden("flowline")


@pytest.fixture(scope="module")
def FL():
    import os
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    _capi.load()
    from tendrils_amd import flow_line
    return flow_line


def drawn_lines(fx):
    """(index in creation order, draw position) of every drawn line"""
    ids = [str(i) for i in fx["meta"]["ids"]]
    return [(ids.index(oid), k) for k, oid in enumerate(fx["meta"]["order"])]


def test_fixtures_present():
    assert len(FIXTURES) >= 9
    names = {p.split("/")[-1] for p in FIXTURES}
    for want in ("open_160x90", "over_field_160x90", "closed_160x90", "sharp_turn_160x90", "offscreen_160x90",
                 "two_lines_160x90", "npot_97x61", "large_480x270", "equal_points_160x90"):
        assert "flowline_%s.npz" % want in names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_attributes_bit_exact(FL, path):
    fx = load(path)
    for i, k in drawn_lines(fx):
        a, b = fx["offsets"][i], fx["offsets"][i + 1]
        got = FL.attributes(fx["points"][a:b], fx["times"][a:b], fx["closed"][i])
        va, vb = fx["a_offsets"][k], fx["a_offsets"][k + 1]
        for name in FL.ATTRIBUTES:
            ref = fx["a_" + name][va:vb]
            g = got[name]
            assert g.shape == ref.shape, (name, g.shape, ref.shape)
            same = (g.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(g) & np.isnan(ref))
            assert same.all(), "%s: %d of %d values differ" % (name, (~same).sum(), same.size)


def test_equal_points_give_infinite_miters(FL):
    """Two equal consecutive points: polyline-normals divides by a zero dot product (the reference's own arrays agree)"""
    pts = np.array([[0, 0], [0.5, 0], [0.5, 0], [1, 0.2]], np.float32)
    a = FL.attributes(pts, [0.0, 16.0, 32.0, 48.0])
    assert np.isinf(a["miter"]).any()
    assert np.isfinite(a["position"]).all()


def test_vertex_counts(FL):
    p = np.array([[0, 0], [0.1, 0], [0.2, 0.1]], np.float32)
    t = [1.0, 2.0, 3.0]
    assert len(FL.attributes(p, t)["miter"]) == 6
    assert len(FL.attributes(p, t, closed=True)["miter"]) == 8
    assert len(FL.attributes(p[:1], t[:1])["miter"]) == 0
    assert len(FL.attributes(p[:1], t[:1], closed=True)["miter"]) == 0
    assert len(FL.attributes(p[:0], t[:0])["miter"]) == 0


def test_closed_line_times(FL):
    """A closed line repeats its first point and time at the end; dt there is times[0] - times[-1]
    (src/flow-line/index.js:38-41, 57-72)."""
    p = np.array([[0, 0], [0.3, 0], [0.3, 0.3]], np.float32)
    t = [100.0, 116.5, 133.0]
    a = FL.attributes(p, t, closed=True)
    assert a["time"].tolist() == [100.0, 100.0, 116.5, 116.5, 133.0, 133.0, 100.0, 100.0]
    assert a["dt"].tolist() == [-33.0, -33.0, 16.5, 16.5, 16.5, 16.5, -33.0, -33.0]
    assert (a["previous"][0] == p[2]).all() and (a["previous"][-1] == p[2]).all()
    assert (a["position"][-1] == p[0]).all()
    o = FL.attributes(p, t)
    assert o["dt"].tolist() == [0.0, 0.0, 16.5, 16.5, 16.5, 16.5]
    assert (o["previous"][0] == p[0]).all()
    # miter sign: -1 on even vertices, +1 on odd
    assert (np.sign(o["miter"][0::2]) == -1).all() and (np.sign(o["miter"][1::2]) == 1).all()


def test_flowline_bookkeeping(FL):
    fl = FL.FlowLine()
    assert fl.line.uniforms == {"color": [1.0, 1.0, 1.0, 1.0], "rad": 0.1, "viewSize": [1.0, 1.0], "speed": 3.0,
                                "speedLimit": 0.01, "crestShape": 0.6}
    fl.add(10.0, [0.0, 0.0]).add(20.0, [0.1, 0.0]).add(30.0, [0.2, 0.0])
    fl.insert(25.0, [0.15, 0.05])
    fl.insert(5.0, [-0.1, 0.0])
    fl.insert(20.0, [0.11, 0.0])            # after the equal time: findIndex looks for the first later time
    assert fl.times == [5.0, 10.0, 20.0, 20.0, 25.0, 30.0]
    assert fl.line.path[3] == [0.11, 0.0]
    assert fl.findIndex(20.0) == 4 and fl.findIndex(100.0) == 6 and fl.findIndex(0.0) == 0
    assert fl.at(1) == {"time": 10.0, "point": [0.0, 0.0]}
    assert fl.at(9) == {"time": None, "point": None}
    assert fl.length == 6
    assert fl.trim(15.0, 30.0) == 4          # drops times < 30 - 15
    assert fl.times == [20.0, 20.0, 25.0, 30.0]
    assert fl.trim(0.0, 100.0) == 0 and fl.line.path == []
    assert fl.trim(0.0, 100.0) == 0
    c = FL.FlowLine({"closed": True})
    assert c.line.closed


def test_flowlines_active_order_and_trim(FL):
    lines = FL.FlowLines()
    for i, id in enumerate([7, "b", 3, "a", 10, "3"]):
        lines.get(id).add(100.0 + i, [0.0, 0.1 * i])
    assert list(lines.active) == ["3", "7", "10", "b", "a"]       # JS: integer keys ascending, then insertion order
    assert lines.get(3).times == [102.0, 105.0]                   # 3 and "3" are one key
    assert lines.get("3") is lines.active[3]
    assert lines.trim(0.0, 103.5) == 2                            # lines whose every point is older go
    assert list(lines.active) == ["3", "10"]
    assert lines.active["3"].times == [105.0]
    opts = lines.get(99, {"closed": True})
    assert opts.line.closed and list(lines.active) == ["3", "10", "99"]
    assert lines.trim(0.0, 1e9) == 0 and len(lines.active) == 0


def test_update_snapshots_what_draw_draws(FL):
    fl = FL.FlowLine()
    fl.add(0.0, [0.0, 0.0]).add(16.0, [0.1, 0.0])
    fl.update()
    fl.add(32.0, [0.2, 0.0])
    pts, times, closed = fl.line._drawn
    assert len(pts) == 2 and len(times) == 2 and not closed
    assert len(fl.line.attributes["miter"]) == 4


def test_argument_errors(FL):
    from tendrils_amd import _capi
    lib = _capi.load()
    nv = C.c_int32(-1)
    pts = np.zeros((3, 2), np.float32)
    tms = np.zeros(3, np.float64)
    fp, dp = pts.ctypes.data_as(_capi._fp), tms.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.th_flow_line_attributes(fp, dp, -1, 0, 0, C.byref(nv), None, None, None, None, None, None) == 1
    assert lib.th_flow_line_attributes(fp, dp, 3, 0, 0, None, None, None, None, None, None, None) == 1
    assert lib.th_flow_line_attributes(None, dp, 3, 0, 0, C.byref(nv), None, None, None, None, None, None) == 1
    assert lib.th_flow_line_attributes(fp, dp, 3, 0, 0, C.byref(nv), None, None, None, None, None, None) == 0 and nv.value == 6
    assert lib.th_flow_line_attributes(fp, dp, 3, 0, 5, C.byref(nv), None, None, None, None, None, None) == 1   # too small
    assert lib.th_flow_line_attributes(fp, dp, 3, 0, 6, C.byref(nv), None, None, None, None, None, None) == 1   # null arrays
    assert lib.th_flow_line_attributes(None, None, 0, 0, 0, C.byref(nv), None, None, None, None, None, None) == 0 and nv.value == 0
    u = _capi.FlowLineUniforms(3.0, 0.1, 0.6, 0.01, (C.c_float * 2)(1.0, 1.0))
    offs = np.array([0, 3], np.int32)
    cl = np.zeros(1, np.int32)
    ip = C.POINTER(C.c_int32)
    assert lib.th_flow_lines(None, C.byref(u), fp, dp, offs.ctypes.data_as(ip), cl.ctypes.data_as(ip), 1) == 1   # null context
    with pytest.raises(ValueError):
        FL.attributes(pts, tms[:2])
    with pytest.raises(RuntimeError):
        FL._bound[0] = None
        FL.FlowLine().add(0.0, [0.0, 0.0]).add(1.0, [0.1, 0.0]).update().draw()
