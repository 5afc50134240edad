"""The windowed lattice hash of the fused integrator (th_logic.hpp "over a window", th_step.hip: hash_window).

A fused launch whose noise coordinates the host can bound hashes the lattice over periodically extended tables, indexed by
i - c with c a multiple of 289 per launch, and leaves the mod 289 of every coordinate out; lanes beyond win_bound =
min(pos_bound, N / max|noiseScale'|), N = 64 noise units, take the reference-order branch.  Whatever a launch decides, the
ring must hold the bytes of the paths that know no window: the reference-order kernel, the texel-order path and the fused
path with hash_window = 0.  The window is an exact-mode path (between win_bound and pos_bound fast mode has its own
arithmetic, which the reference-order branch does not give): in fast mode no launch takes it, and the fused path gives the
bytes of the texel-order path as before.

256^2 particles over a 96 x 54 field, step_n calls of 2, 3 and 32 steps on one context.  |pos| is log-uniform up to 0.999
win_bound with either sign; four rows lie within 0.1 % of +-win_bound, one row at |pos| = 50 (beyond win_bound, inside
pos_bound), one at 3e6 (beyond pos_bound), some texels are inert and a few NaN.  The cases put the window at the defaults, across
a multiple of 289 between two launches, at negative z, at two spreads of the noise scale, and make the host refuse it twice.
The window of every launch is recomputed here as the host computes it; what the cases cover is computed in the restatement's
fp32 arithmetic and asserted (for the f32 inputs: a packed ring clamps |pos| to 2, a tenth of win_bound)."""
import math

import numpy as np
import pytest

from helpers import bits_equal, pack_state, unpack_state

pytestmark = pytest.mark.gpu

N = 256
VIEW = (96, 54)
VIEW_SIZE = (1.0, 96.0 / 54.0)          # cover_aspect of the view
STEPS = (2, 3, 32)                      # consecutive step_n calls of one context: fused launches of 2, 3 and 32 steps
DT = 1000.0 / 60.0
WIN_N = 64.0                            # |pos * noiseScale'| <= N inside win_bound
WIN_SPAN, WIN_MAX_CELL, WIN_MIN_VIEWS = 286, 8958, 2.0
DEFAULTS = dict(noiseScale=2.125, varyNoiseScale=0.5, noiseSpeed=0.00025, varyNoiseSpeed=0.1)

CASES = {
    # B's z near 1235, iz near 1646
    "default": dict(over={}, time0=1000.0),
    # the first cell of B's z range passes 1734 = 6 * 289 between the launch of 3 steps and the launch of 32
    "edge": dict(over=dict(noiseSpeed=0.05), time0=1915.0),
    # z < 0 in both evaluations
    "negative": dict(over=dict(noiseSpeed=-0.05, varyNoiseSpeed=0.01), time0=40000.0),
    # one scale for every particle: the rows at +-win_bound reach the ends of the xy ranges; B's xy window starts at 289, two
    # cells below its first lane
    "vary0": dict(over=dict(varyNoiseScale=0.0, noiseSpeed=-0.05, varyNoiseSpeed=0.0), time0=740.0),
    "vary2": dict(over=dict(varyNoiseScale=2.0, noiseSpeed=0.05, varyNoiseSpeed=0.02), time0=9000.0),
    # refused: win_bound = 64 / 2.1e6 is no part of the view
    "huge_scale": dict(over=dict(noiseScale=1.4e6), time0=1000.0, refused=True),
    # refused: |iz| beyond 8958
    "large_cell": dict(over=dict(noiseSpeed=0.05, varyNoiseSpeed=0.001), time0=140000.0, refused=True),
}
WINDOWED = [k for k, c in CASES.items() if not c.get("refused")]


def uniforms(case):
    return dict(DEFAULTS, **CASES[case]["over"])


def bounds(u):
    """pos_bound (th_step.hip: plan_step) and win_bound = min(pos_bound, N / max|noiseScale'|) (hash_window)"""
    f = lambda name: float(np.float32(u[name]))
    nscale = abs(f("noiseScale")) * (1.0 + abs(f("varyNoiseScale"))) * 1.001
    pos_bound = np.float32(min(4194304.0 / nscale * 0.999, 999999.0))
    s0 = f("noiseScale")
    s1 = s0 + f("varyNoiseScale") * s0
    return pos_bound, np.float32(min(float(pos_bound), WIN_N / max(abs(s0), abs(s1))))


def launch_times(case):
    """the fp32 times of the steps of every fused launch, accumulated in double as the timer does"""
    t, out = CASES[case]["time0"], []
    for n in STEPS:
        ts = []
        for _ in range(n):
            t += DT
            ts.append(float(np.float32(t)))
        out.append(ts)
    return out


def window(u, times):
    """th_step.hip: hash_window - per evaluation (cxy, cz) and the ranges, or None where the host refuses"""
    f = lambda name: float(np.float32(u[name]))
    _, wb = bounds(u)
    if not float(wb) * min(VIEW_SIZE) >= WIN_MIN_VIEWS:
        return None
    v0 = f("noiseSpeed")
    v1 = v0 + f("varyNoiseSpeed") * v0
    nts = [t * v for t in times for v in (v0, v1)]
    tlo, thi = min(nts), max(nts)
    out = []
    for e in (0, 1):
        off = 1234.5678 if e else 0.0
        zlo, zhi = tlo + off, thi + 1.0 + off
        slo, shi = zlo / 3.0 - 2.0 * WIN_N / 3.0, zhi / 3.0 + 2.0 * WIN_N / 3.0
        lo = (math.floor(-WIN_N + slo) - 2, math.floor(zlo + slo) - 2)
        hi = (math.floor(WIN_N + shi) + 2, math.floor(zhi + shi) + 2)
        for a in (0, 1):
            if hi[a] - lo[a] > WIN_SPAN or max(abs(lo[a]), abs(hi[a])) + 1 > WIN_MAX_CELL:
                return None
        out.append(dict(c=(289 * (lo[0] // 289), 289 * (lo[1] // 289)), lo=lo, hi=hi))
    return out


def inputs(case):
    u = uniforms(case)
    pb, wb = bounds(u)
    wb = float(wb)
    rng = np.random.default_rng(289 + sorted(CASES).index(case))
    st = np.empty((N, N, 4), np.float32)
    mag = wb * 0.999 * 2.0 ** (-12.0 * rng.random((N, N, 2)) ** 2)          # (squared: half of them in the last octave and a half)
    st[..., :2] = mag * rng.choice([-1.0, 1.0], (N, N, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (N, N, 2))
    # the edge of the window: the last rows (index i near 1: the largest noise scale) within 0.1 % of +-win_bound,
    # the signs of the two components in all four combinations along a row
    edge = wb * (1.0 - 0.001 * rng.random((4, N, 2)))
    signs = np.array([[-1, -1], [1, 1], [-1, 1], [1, -1]], np.float64)[np.arange(N) % 4]
    st[-4:, :, :2] = edge * signs[None]
    st[N // 2, :, :2] = 50.0 * rng.choice([-1.0, 1.0], (N, 2))                # beyond win_bound, inside pos_bound
    st[N // 2 + 1, :, :2] = 3e6 * rng.choice([-1.0, 1.0], (N, 2))             # beyond pos_bound
    st[0, :16] = [-1e6, -1e6, 0, 0]                                            # inert
    st[1, :4, 0] = np.nan
    st[1, 4:8, 1] = np.nan
    fw, fh = VIEW
    fl = np.zeros((fh, fw, 4), np.float32)
    fl[..., :2] = rng.uniform(-.01, .01, (fh, fw, 2))
    fl[..., 2] = CASES[case]["time0"] + rng.uniform(-150, 16, (fh, fw))
    fl[..., 3] = 1
    return st, fl


def lattice(st, time, overrides, bound):
    """Lattice coordinates (ix, iy, iz), first-corner offsets x0 and the in-domain mask of both noise evaluations of one
    step, in the restatement's arithmetic (oracle/tendrils_oracle.c: logic_texel, to_snoise3), each operation rounded to
    fp32."""
    f = np.float32
    W = H = f(N)
    y, x = np.mgrid[0:N, 0:N]
    fcx, fcy = x.astype(f) + f(0.5), y.astype(f) + f(0.5)
    uvx, uvy = fcx / W, fcy / H
    i = (fcx + fcy * W) / (W * H)
    vary = lambda base, var: f(base) + (i * f(var)) * f(base)
    nscale = vary(overrides["noiseScale"], overrides["varyNoiseScale"])
    ntime = f(time) * vary(overrides["noiseSpeed"], overrides["varyNoiseSpeed"])
    px, py = st[..., 0], st[..., 1]
    live = (np.abs(px) < bound) & (np.abs(py) < bound)
    C3, C6 = f(1.0) / f(3.0), f(1.0) / f(6.0)
    out = []
    for vz in (uvx + ntime, (uvy + ntime) + f(1234.5678)):
        vx, vy = px * nscale, py * nscale
        s = (vx * C3 + vy * C3) + vz * C3
        ix, iy, iz = np.floor(vx + s), np.floor(vy + s), np.floor(vz + s)
        t = (ix * C6 + iy * C6) + iz * C6
        x0 = ((vx - ix) + t, (vy - iy) + t, (vz - iz) + t)
        out.append(((ix, iy, iz), x0))
    return out, live


def cells_of(case):
    """per launch: its window and the in-window lanes' cells and traversal orders at its first and its last time (the
    input state: a particle moves by less than a hundredth of a cell per step)"""
    u = uniforms(case)
    st, _ = inputs(case)
    _, wb = bounds(u)
    out = []
    for times in launch_times(case):
        win = window(u, times)
        for time in (times[0], times[-1]):
            with np.errstate(invalid="ignore"):
                evals, live = lattice(st, time, u, wb)
            out.append((win, [([c[live].astype(np.int64) for c in cells], [a[live] for a in x0]) for cells, x0 in evals]))
    return out


def test_refused_windows_are_refused_by_the_rule():
    for case in CASES:
        wins = [window(uniforms(case), ts) for ts in launch_times(case)]
        if CASES[case].get("refused"):
            assert all(w is None for w in wins), case
        else:
            assert all(w is not None for w in wins), case


def test_every_in_window_lane_stays_inside_its_launchs_window():
    for case in WINDOWED:
        for win, evals in cells_of(case):
            for w, (cells, _) in zip(win, evals):
                for axis, c in enumerate(cells):
                    a = 0 if axis < 2 else 1
                    assert w["lo"][a] <= c.min() and c.max() <= w["hi"][a], (case, axis)
                    assert 0 <= c.min() - w["c"][a] and c.max() - w["c"][a] + 1 <= 577, (case, axis)


def test_the_cases_cover_the_window():
    residues = [[set() for _ in range(3)] for _ in range(2)]
    signs = [[set() for _ in range(3)] for _ in range(2)]
    orders = [set(), set()]
    near_origin, near_top = set(), set()
    for case in WINDOWED:
        for win, evals in cells_of(case):
            for e, (w, (cells, x0)) in enumerate(zip(win, evals)):
                for axis, c in enumerate(cells):
                    a = 0 if axis < 2 else 1
                    residues[e][axis] |= set(np.unique(c % 289).tolist())
                    signs[e][axis] |= set(np.unique(np.sign(c)).tolist())
                    if (c - w["c"][a] <= 2).any():
                        near_origin.add(case)
                    if (w["hi"][a] - c <= 2).any():
                        near_top.add(case)
                l1, l2, l3 = x0[0] < x0[1], x0[1] < x0[2], x0[2] < x0[0]
                orders[e] |= set(np.unique(l1 + 2 * l2 + 4 * l3).tolist())
    bad = []
    for e in (0, 1):
        for axis in range(3):
            if len(residues[e][axis]) != 289:
                bad.append("evaluation %d axis %s: %d of 289 residues" % (e, "xyz"[axis], len(residues[e][axis])))
            if not {-1, 1} <= signs[e][axis]:
                bad.append("evaluation %d axis %s: one sign only" % (e, "xyz"[axis]))
        if not set(range(1, 7)) <= orders[e]:
            bad.append("evaluation %d: traversal orders %s" % (e, sorted(orders[e])))
    if not near_origin & near_top:
        bad.append("no case with a lane within 2 cells of its window's origin (%s) and one within 2 cells of its upper end (%s)"
                   % (sorted(near_origin), sorted(near_top)))
    assert not bad, "; ".join(bad)


def test_the_window_moves_between_two_launches():
    wins = [window(uniforms("edge"), ts) for ts in launch_times("edge")]
    assert wins[1][1]["c"][1] != wins[2][1]["c"][1]
    assert wins[1][1]["hi"][1] >= wins[2][1]["c"][1] > wins[1][1]["lo"][1]      # a multiple of 289 inside the earlier launch's range


PATHS = {
    "window": dict(bucket=1, fuse=1, rebucket_steps=4, hash_window=1),
    "no_window": dict(bucket=1, fuse=1, rebucket_steps=4, hash_window=0),
    "generic": dict(bucket=1, fuse=1, force_generic=1),
    "plain": dict(bucket=0, fuse=0),
}


def run_path(fmt, mode, path, case, st, fl):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts["mode"] = mode
    opts["stateFormat"] = ta.TH_STATE_F16 if fmt == "f16" else ta.TH_STATE_F32
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(N)
    assert tuple(t.viewSize) == VIEW_SIZE and t.timer.step * t.timer.rate == DT
    t.state.update(uniforms(case))
    for k, v in PATHS[path].items():
        t.particles.option(k, v)
    t.particles.upload_texels(st)
    t.flow.set_pixels(fl)
    t.timer.time = CASES[case]["time0"]
    outs = []
    for n in STEPS:
        t.step_n(n)
        outs.append((t.particles.read(0).copy(), t.particles.read(1).copy()))
    launches = t.particles.option("hash_window_launches")
    t.dispose()
    return outs, launches


@pytest.fixture(scope="module")
def runs():
    """every (case, format, mode, path) once, on demand; shared by the comparisons below and left unchanged"""
    cache, states = {}, {}

    def get(case, fmt, mode, path):
        if case not in states:
            st, fl = inputs(case)
            states[case] = ({"f32": st, "f16": unpack_state(pack_state(st))}, fl)
        if (case, fmt, mode, path) not in cache:
            cache[(case, fmt, mode, path)] = run_path(fmt, mode, path, case, states[case][0][fmt], states[case][1])
        return cache[(case, fmt, mode, path)]
    return get


def assert_same_bytes(a, b, what):
    """bit for bit, a NaN of any payload equal to a NaN (helpers.bits_equal: the reference does not pin NaN payloads, and
    the paths make the NaN of a NaN position in different ways)"""
    for n, (a0, a1), (b0, b1) in zip(STEPS, a, b):
        for name, x, y in (("state", a0, b0), ("previous state", a1, b1)):
            diff = ~bits_equal(x, y).all(-1)
            assert not diff.any(), "%s, step_n(%d) %s: %d of %d texels differ, first at %s" % (
                what, n, name, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_exact_mode_window_equals_the_paths_without_it(runs, case, fmt):
    import tendrils_amd as ta
    a, launches = runs(case, fmt, ta.TH_MODE_EXACT, "window")
    assert launches == (0 if CASES[case].get("refused") else len(STEPS)), "fused launches over the window"
    for other in ("generic", "plain", "no_window"):
        b, none = runs(case, fmt, ta.TH_MODE_EXACT, other)
        assert none == 0
        assert_same_bytes(a, b, "%s, %s exact: window against %s" % (case, fmt, other))


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_fast_mode_window_equals_the_texel_order_path(runs, case, fmt):
    import tendrils_amd as ta
    a, launches = runs(case, fmt, ta.TH_MODE_FAST, "window")
    assert launches == 0, "the window is an exact-mode path: between win_bound and pos_bound fast mode has its own arithmetic"
    b, _ = runs(case, fmt, ta.TH_MODE_FAST, "plain")
    assert_same_bytes(a, b, "%s, %s fast: window against plain" % (case, fmt))
