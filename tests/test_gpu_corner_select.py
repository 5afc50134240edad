"""The table path of the noise after its stage-y selects moved behind the reads, the falloff clamp into the subtract and the
z mask into the bias add (th_logic.hpp: snoise_corners_tab, snoise_finish): every kernel that runs it
against the CPU oracle, bit for bit.

64^2 and 48^2 (no power of two: the true divisions) particles over a 160 x 90 flow field, default uniforms.  256 particles
sit at position exactly (0, 0): there nx == ny, the lattice cell and the first corner's x and y offsets are equal, and the
first order compare (x0.x < x0.y) is false on a tie - the first two corner steps are decided by the compares against z
alone.  step_n(1), step_n(2) and step_n(20) from the same start are compared against as many oracle steps, both states the
ring keeps; on a packed ring against decode -> oracle step -> encode.  Paths: the fused launches over tile-sorted slots
with the window and without it, the single-step kernels over sorted slots, and fast mode within the one-step tolerance of
tests/test_gpu_logic_parity.py.  What the inputs cover - all six strict corner orders in both evaluations, the tie at
least 256 times - is computed in the restatement's fp32 arithmetic and asserted."""
import numpy as np
import pytest

from helpers import bits_equal, pack_state, unpack_state
from test_gpu_logic_parity import FAST_ATOL

pytestmark = pytest.mark.gpu

VIEW = (160, 90)
TIME0 = 4000.0
STEPS = (1, 2, 20)
SIZES = (64, 48)
TIES = 256
SEED = 20950


def inputs(n):
    rng = np.random.default_rng(SEED + n)
    st = np.empty((n, n, 4), np.float32)
    st[..., :2] = rng.uniform(-1.2, 1.2, (n, n, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (n, n, 2))
    st[rng.random((n, n)) < 0.03] = [-1e6, -1e6, 0, 0]
    flat = st.reshape(-1, 4)
    tie = rng.choice(n * n, TIES, replace=False)           # spread over the workgroups
    flat[tie, :2] = 0.0
    fw, fh = VIEW
    fl = np.zeros((fh, fw, 4), np.float32)
    fl[..., :2] = rng.uniform(-.01, .01, (fh, fw, 2))
    fl[..., 2] = TIME0 + rng.uniform(-150, 16, (fh, fw))
    fl[..., 3] = 1
    return st, fl


def first_corner_offsets(st, time, state):
    """x0 of both noise evaluations of one step and the live mask, in the restatement's arithmetic
    (oracle/tendrils_oracle.c: logic_texel, to_snoise3), each operation rounded to fp32"""
    f = np.float32
    n = st.shape[0]
    W = H = f(n)
    y, x = np.mgrid[0:n, 0:n]
    fcx, fcy = x.astype(f) + f(0.5), y.astype(f) + f(0.5)
    uvx, uvy = fcx / W, fcy / H
    i = (fcx + fcy * W) / (W * H)
    vary = lambda base, var: f(base) + (i * f(var)) * f(base)
    nscale = vary(state["noiseScale"], state["varyNoiseScale"])
    ntime = f(time) * vary(state["noiseSpeed"], state["varyNoiseSpeed"])
    px, py = st[..., 0], st[..., 1]
    live = (px != f(-1e6)) | (py != f(-1e6))
    C3, C6 = f(1.0) / f(3.0), f(1.0) / f(6.0)
    out = []
    for vz in (uvx + ntime, (uvy + ntime) + f(1234.5678)):
        vx, vy = px * nscale, py * nscale
        s = (vx * C3 + vy * C3) + vz * C3
        ix, iy, iz = np.floor(vx + s), np.floor(vy + s), np.floor(vz + s)
        t = (ix * C6 + iy * C6) + iz * C6
        out.append(((vx - ix) + t, (vy - iy) + t, (vz - iz) + t))
    return out, live


def coverage_failures(st, time, state):
    evals, live = first_corner_offsets(st, time, state)
    bad = []
    for e, (ax, ay, az) in enumerate(evals):
        ax, ay, az = ax[live], ay[live], az[live]
        strict = (ax != ay) & (ay != az) & (az != ax)
        orders = set(np.unique(((ax < ay) + 2 * (ay < az) + 4 * (az < ax))[strict]).tolist())
        if orders != set(range(1, 7)):
            bad.append("evaluation %d: strict corner orders %s" % (e, sorted(orders)))
        ties = int((ax == ay).sum())
        if ties < TIES:
            bad.append("evaluation %d: %d ties of the first two offsets" % (e, ties))
    return bad


# the library's paths that run the table chain
PATHS = {
    "window": dict(bucket=1, fuse=1, rebucket_steps=4, hash_window=1),      # logic_fused_kernel<.., WIN> on tile-sorted slots
    "no_window": dict(bucket=1, fuse=1, rebucket_steps=4, hash_window=0),   # the same launches over the unwindowed tables
    "sorted": dict(bucket=1, resort_steps=3),                               # single-step kernels over sorted slots
}


def make(n, fmt, mode, path):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts["mode"] = mode
    opts["stateFormat"] = ta.TH_STATE_F16 if fmt == "f16" else ta.TH_STATE_F32
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(n)
    for k, v in PATHS[path].items():
        t.particles.option(k, v)
    return t


def run(n, fmt, mode, path, st, fl, steps):
    """`steps` steps from the start state on a fresh context: the two states the ring keeps, and the fused launches over the window"""
    t = make(n, fmt, mode, path)
    t.particles.upload_texels(st)
    t.flow.set_pixels(fl)
    t.timer.time = TIME0
    if path == "sorted":            # single launches (th_step_n without fusion steps in texel order)
        for _ in range(steps):
            t.timer.tick()
            t.step()
    else:
        t.step_n(steps)
    out = t.particles.read(0).copy(), t.particles.read(1).copy()
    launches = t.particles.option("hash_window_launches")
    t.dispose()
    return out, launches


@pytest.fixture(scope="module")
def cases(oracle):
    """per (size, format), once and left unchanged: the start state, the flow field and the oracle's trajectory [0 .. 20]"""
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    cache = {}

    def get(n, fmt):
        if (n, fmt) not in cache:
            st, fl = inputs(n)
            quant = (lambda s: unpack_state(pack_state(s))) if fmt == "f16" else (lambda s: s)
            st = quant(st)
            t = ta.Tendrils(View(*VIEW))               # for its host side only: the uniforms and the timer a context steps with
            t.resize()
            t.setup(n)
            state = {k: v for k, v in t.state.items() if isinstance(v, (int, float))}
            view_size = list(t.viewSize)
            t.timer.time = TIME0
            traj, times = [st], []
            for _ in range(max(STEPS)):
                t.timer.tick()
                times.append(t.timer.time)
                u = oracle.logic_uniforms(n, n, t.timer.time, t.timer.dt, view_size=view_size, **state)
                traj.append(quant(oracle.logic_step(u, traj[-1], fl)))
            t.dispose()
            cache[(n, fmt)] = dict(st=st, fl=fl, traj=traj, state=state, first_time=times[0])
        return cache[(n, fmt)]
    return get


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_inputs_cover_the_corner_orders_and_the_tie(cases, n, fmt):
    c = cases(n, fmt)
    bad = coverage_failures(c["st"], c["first_time"], c["state"])
    assert not bad, "; ".join(bad)
    assert int(((c["st"][..., 0] == 0) & (c["st"][..., 1] == 0)).sum()) >= TIES


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_exact_mode_equals_the_oracle(cases, n, fmt, path):
    import tendrils_amd as ta
    c = cases(n, fmt)
    for steps in STEPS:
        (cur, prev), launches = run(n, fmt, ta.TH_MODE_EXACT, path, c["st"], c["fl"], steps)
        # (a call of one step is no fused launch: it runs the single-step kernel, which shares snoise_finish)
        assert launches == (1 if path == "window" and steps >= 2 else 0), "fused launches over the window"
        for name, got, want in (("state", cur, c["traj"][steps]), ("previous state", prev, c["traj"][steps - 1])):
            diff = ~bits_equal(got, want).all(-1)
            print("%d^2 %s %s step_n(%d) %s: %d of %d texels differ" % (n, fmt, path, steps, name, int(diff.sum()), diff.size))
            assert not diff.any(), "%d^2 %s %s, step_n(%d) %s: %d of %d texels differ, first at %s" % (
                n, fmt, path, steps, name, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


@pytest.mark.parametrize("path", ["window", "sorted"])      # (no fast launch takes the window: "no_window" is the same kernel)
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_fast_mode_within_its_one_step_tolerance(cases, n, fmt, path):
    import tendrils_amd as ta
    c = cases(n, fmt)
    # the state after ONE step: what a call of one step leaves (the single-step kernel), and what a fused launch of two
    # steps keeps as the previous state (the fused kernel's first step)
    (one, start), l1 = run(n, fmt, ta.TH_MODE_FAST, path, c["st"], c["fl"], 1)
    (_, first), l2 = run(n, fmt, ta.TH_MODE_FAST, path, c["st"], c["fl"], 2)
    assert l1 == 0 and l2 == 0, "the window is an exact-mode path"
    assert bits_equal(start, c["st"]).all()
    want = c["traj"][1]
    for what, got in (("step_n(1) state", one), ("step_n(2) previous state", first)):
        assert (np.isnan(got) == np.isnan(want)).all()
        d = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
        if fmt == "f32":
            print("%d^2 %s fast %s: max |delta| %.3g" % (n, path, what, d.max()))
            assert d.max() <= FAST_ATOL, "%s: max |delta| %.3g" % (what, d.max())
        else:
            # Both sides went through the ring's encoding q: |q(a) - q(b)| <= |a - b| + one step of the grid - 2^-14 for a
            # position, 2^-17 for an fp16 velocity component of at most speedLimit = 0.01 < 2^-6.
            live = np.abs(want[..., 0]) < 1e5
            pos, vel = d[live][:, :2], d[live][:, 2:]
            print("%d^2 %s fast packed %s: max |d pos| %.3g max |d vel| %.3g" % (n, path, what, pos.max(), vel.max()))
            assert np.abs(want[live][:, 2:]).max() < 2.0 ** -6
            assert pos.max() <= FAST_ATOL + 2.0 ** -14 and vel.max() <= FAST_ATOL + 2.0 ** -17, what
