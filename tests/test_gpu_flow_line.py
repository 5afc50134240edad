"""Flow lines on the GPU (th_flow_lines, tendrils_amd/csrc/th_flowline.hip): the binned HIP path against the reference's
captures (tests/golden/flowline_*.npz) through the Python and the Node host, against the numpy restatement
(tests/flowline_restatement.py) on seeded cases no capture covers, and its place in the frame: batching, no-ops, the next
step reading what the lines drew, row-band shards, packed rings, the release library."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import flowline_restatement as R
from helpers import bits_equal, golden
from test_flow_line_restatement import fixture_case, flowline_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = golden("flowline")


def tendrils_with_flow(base, n=16, opts=None):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    h, w = base.shape[:2]
    t = ta.Tendrils(View(w, h), opts)
    t.resize()
    t.setup(n)
    t.flow.shape = [w, h]
    t.flow.set_pixels(base)
    return t


def uniforms_of(meta_uniforms):
    from tendrils_amd.flow_line import defaults
    u = defaults()
    u.update(meta_uniforms)
    return u


def check(got, want, cov, base, time):
    """coverage from the restatement / capture: covered texels within tolerance, the others untouched bit for bit"""
    ok = flowline_close(got, want, time)
    assert ok[cov].all(), "%d covered texels out of tolerance; max dev %s" % (
        (~ok[cov]).sum(), np.abs(got[cov].astype(np.float64) - want[cov]).max(0))
    assert bits_equal(got[~cov], base[~cov]).all(), "%d texels outside the strokes changed" % (~bits_equal(got[~cov], base[~cov])).sum()


@pytest.mark.parametrize("batched", [True, False], ids=["FlowLines.draw", "FlowLine.draw"])
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_hip_matches_reference_capture(path, batched):
    import tendrils_amd as ta
    m, base, ref, cov, lines = fixture_case(path)
    t = tendrils_with_flow(base)
    fls = ta.FlowLines()
    ids = [str(i) for i in m["ids"]]
    for oid, (pts, times, closed) in zip(m["order"], lines):
        fl = fls.get(oid, {"closed": closed})
        for p, tm in zip(pts, times):
            fl.add(float(tm), [float(p[0]), float(p[1])])
    assert list(fls.active) == m["order"] and sorted(ids) == sorted(m["order"])
    t.flow.bind()
    if batched:
        for fl in fls.active.values():
            fl.line.uniforms.update(m["uniforms"])
        fls.draw()
    else:
        for fl in fls.active.values():
            fl.line.uniforms.update(m["uniforms"])
            fl.update().draw()
    got = t.flow.read()
    t.dispose()
    check(got, ref, cov, base, max(np.abs(l[1]).max() for l in lines))


def random_case(seed, w, h, nlines, npts, step=0.05, jitter=0.0):
    """seeded strokes: pointer-like ones, long ones, tiny ones, degenerate ones (repeated points, one point), strokes
    entirely off screen, strokes along tile edges"""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(nlines):
        kind = i % 6
        n = int(rng.integers(1, npts + 1)) if kind != 1 else npts
        start = rng.uniform(-1.1, 1.1, 2)
        if kind == 4:
            start = rng.uniform(1.6, 3.0, 2) * rng.choice([-1, 1], 2)           # off screen
        ang = rng.uniform(0, 2 * np.pi)
        st = step * (0.05 if kind == 2 else 1.0)                                 # tiny triangles
        pts = [start]
        for _ in range(n - 1):
            ang += rng.uniform(-0.6, 0.6)
            pts.append(pts[-1] + st * rng.uniform(0.3, 1.5) * np.array([np.cos(ang), np.sin(ang)]))
        pts = np.array(pts, np.float32)
        if kind == 3 and n > 2:
            pts[n // 2] = pts[n // 2 - 1]                                         # equal consecutive points
        if kind == 5:                                                            # along a tile edge (x = 16 texels)
            pts[:, 0] = np.float32(2 * 16.0 / w - 1)
        times = 1000.0 + 16.7 * np.arange(n) + rng.uniform(0, 3, n)
        lines.append((pts, times, bool(rng.random() < 0.15)))
    base = np.zeros((h, w, 4), np.float32)
    base[..., :2] = rng.uniform(-0.01, 0.01, (h, w, 2))
    base[..., 2] = 900.0
    base[..., 3] = rng.uniform(0, 1, (h, w))
    return lines, base


def restate(base, lines, u):
    from tendrils_amd import flow_line as FL
    want = base.copy()
    cov = np.zeros(want.shape[:2], np.int64)
    R.draw(want, [FL.attributes(*l) for l in lines], u, cov)
    return want, cov > 0


def hip_draw(t, lines, u, calls=1):
    from tendrils_amd import flow_line as FL
    ctx = t.particles._ctx
    if calls == 1:
        FL.draw_lines(ctx, u, lines)
    else:
        for l in lines:
            FL.draw_lines(ctx, u, [l])
    return t.flow.read()


@pytest.mark.parametrize("seed,w,h,nlines,npts,u", [
    (1, 160, 90, 40, 12, {}),
    (2, 97, 61, 60, 20, {"rad": 0.2, "speedLimit": 0.005}),
    (3, 480, 270, 300, 16, {"viewSize": [0.5625, 1.0]}),
    (4, 256, 256, 8, 200, {"speed": 1.0, "crestShape": 0.9}),          # long strokes
    (5, 1920, 1080, 200, 12, {"viewSize": [0.5625, 1.0]}),
    (6, 33, 17, 50, 8, {"rad": 0.6}),                                   # wide strokes over a tiny field
])
def test_hip_matches_restatement_on_random_strokes(seed, w, h, nlines, npts, u):
    lines, base = random_case(seed, w, h, nlines, npts)
    uu = uniforms_of(u)
    want, cov = restate(base, lines, uu)
    assert cov.sum() > 0
    t = tendrils_with_flow(base)
    got = hip_draw(t, lines, uu)
    t.dispose()
    check(got, want, cov, base, 2000.0)


def test_repeated_calls_equal_one_batched_call():
    lines, base = random_case(11, 320, 180, 64, 16)
    u = uniforms_of({})
    a = tendrils_with_flow(base)
    one = hip_draw(a, lines, u, calls=1)
    a.dispose()
    b = tendrils_with_flow(base)
    many = hip_draw(b, lines, u, calls=len(lines))
    b.dispose()
    assert bits_equal(one, many).all()
    c = tendrils_with_flow(base)                   # and twice over (the scratch kept from the first call)
    hip_draw(c, lines, u)
    twice = hip_draw(c, lines, u)
    c.dispose()
    from tendrils_amd import flow_line as FL
    d = base.copy()
    R.draw(d, [FL.attributes(*l) for l in lines], u)
    R.draw(d, [FL.attributes(*l) for l in lines], u)
    assert flowline_close(twice, d, 2000.0).all()


def test_no_lines_leave_the_flow_bit_identical():
    from tendrils_amd import flow_line as FL
    lines, base = random_case(12, 96, 54, 1, 2)
    t = tendrils_with_flow(base)
    FL.draw_lines(t.particles._ctx, uniforms_of({}), [])
    FL.draw_lines(t.particles._ctx, uniforms_of({}), [(np.zeros((1, 2), np.float32), np.zeros(1), False),
                                                       (np.zeros((0, 2), np.float32), np.zeros(0), True)])
    got = t.flow.read()
    t.dispose()
    assert bits_equal(got, base).all()


def test_next_step_reads_the_lines():
    """Lines drawn between draw() and step() are what the next step() reads: the same step over the flow downloaded after
    the lines (uploaded into a second context) gives the same particles."""
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    n, view = 64, (160, 90)
    rng = np.random.default_rng(5)
    st = np.zeros((n, n, 4), np.float32)
    st[..., :2] = rng.uniform(-1, 1, (n, n, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (n, n, 2))
    lines, _ = random_case(13, view[0], view[1], 20, 12)
    outs = []
    flow_after = None
    for k in range(2):
        t = ta.Tendrils(View(*view))
        t.resize()
        t.setup(n)
        t.particles.upload_texels(st)
        t.timer.time = 1100.0
        t.timer.tick()
        t.step()
        t.draw()
        if k == 0:
            t.flow.bind()
            fls = ta.FlowLines()
            for i, (pts, times, closed) in enumerate(lines):
                fl = fls.get(i, {"closed": closed})
                for p, tm in zip(pts, times):
                    fl.add(float(tm), [float(p[0]), float(p[1])])
            fls.trim(1 / t.state["flowDecay"], t.timer.time)
            for fl in fls.active.values():
                fl.line.uniforms.update(t.state)
                fl.update().draw()
            flow_after = t.flow.read()
        else:
            before = t.flow.read()
            assert not bits_equal(before, flow_after).all()
            t.flow.set_pixels(flow_after)
        t.timer.tick()
        t.step()
        outs.append(t.particles.read(0))
        t.dispose()
    assert bits_equal(outs[0], outs[1]).all()


def test_two_rank_loopback_world_draws_the_whole_lines():
    from test_gpu_loopback import inputs, world_of
    n, view = 64, (96, 54)
    cur, prev, base = inputs(n, view, 21)
    lines, _ = random_case(14, view[0], view[1], 24, 10)
    u = uniforms_of({})
    want, cov = restate(base, lines, u)
    from tendrils_amd import flow_line as FL
    one = tendrils_with_flow(base)
    FL.draw_lines(one.particles._ctx, u, lines)
    single = one.flow.read()
    one.dispose()
    check(single, want, cov, base, 2000.0)
    shards = world_of(n, view, 2, cur, prev, base)
    for t in shards:
        FL.draw_lines(t.particles._ctx, u, lines)
    got = [t.flow.read() for t in shards]
    for t in shards:
        t.dispose()
    for g in got:
        assert bits_equal(g, single).all()


def test_wide_packed_ring_draws_lines():
    """A 16384-wide context on a packed (TH_STATE_F16) ring, one row band: flow stays RGBA32F and takes lines."""
    import tendrils_amd as ta
    lines, base = random_case(15, 480, 270, 40, 12)
    u = uniforms_of({"viewSize": [0.5625, 1.0]})
    want, cov = restate(base, lines, u)
    opts = ta.defaults()
    opts.update(row0=0, rows=8, globalHeight=16384, stateFormat=ta.TH_STATE_F16)
    t = tendrils_with_flow(base, n=16384, opts=opts)
    got = hip_draw(t, lines, u)
    t.dispose()
    check(got, want, cov, base, 2000.0)


CHILD = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tendrils_amd import _capi
lib = _capi.load()
assert os.path.realpath(lib._name) == os.path.realpath(RELEASE), lib._name
assert not hasattr(lib, "th_comm_loopback_id")
from test_gpu_flow_line import tendrils_with_flow, check
from test_flow_line_restatement import fixture_case
import tendrils_amd as ta
m, base, ref, cov, lines = fixture_case(PATH)
t = tendrils_with_flow(base)
t.flow.bind()
fls = ta.FlowLines()
for oid, (pts, times, closed) in zip(m["order"], lines):
    fl = fls.get(oid, {"closed": closed})
    for p, tm in zip(pts, times):
        fl.add(float(tm), [float(p[0]), float(p[1])])
    fl.line.uniforms.update(m["uniforms"])
fls.draw()
got = t.flow.read()
t.dispose()
check(got, ref, cov, base, max(np.abs(l[1]).max() for l in lines))
print("release ok")
'''


def test_release_library_draws_a_fixture():
    release = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
    assert os.path.exists(release), "make release first (__graft_entry__.build() does)"
    path = [p for p in FIXTURES if p.endswith("two_lines_160x90.npz")][0]
    code = "ROOT=%r\nRELEASE=%r\nPATH=%r\n" % (ROOT, release, path) + CHILD
    env = dict(os.environ, TH_LIB=release)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "release ok" in r.stdout, r.stdout + r.stderr


def test_node_host_matches_reference_captures():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "tendrils_amd", "lib", "tendrils_flow_lines.node")
    assert node, "node is required"
    assert os.path.exists(addon), "the flow-lines addon was not built"
    script = os.path.join(ROOT, "tests", "js", "flow_lines_fixture.js")
    for path in FIXTURES:
        m, base, ref, cov, lines = fixture_case(path)
        job = {"w": int(base.shape[1]), "h": int(base.shape[0]), "uniforms": m["uniforms"],
               "lines": [{"id": oid, "closed": cl, "points": pts.astype(np.float64).tolist(), "times": times.tolist()}
                         for oid, (pts, times, cl) in zip(m["order"], lines)]}
        fd, jpath = tempfile.mkstemp(suffix=".json")
        os.close(fd)
        np.save(jpath + ".npy", base)
        with open(jpath, "w") as f:
            json.dump(job, f)
        out = jpath + ".out"
        try:
            r = subprocess.run([node, script, jpath, jpath + ".npy", out], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            got = np.fromfile(out, np.float32).reshape(base.shape)
        finally:
            for p in (jpath, jpath + ".npy", out):
                if os.path.exists(p):
                    os.remove(p)
        check(got, ref, cov, base, max(np.abs(l[1]).max() for l in lines))
