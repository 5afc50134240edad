"""The hash index chain of the noise over its whole domain (th_logic.hpp: snoise_corners_tab - byte offsets read from the
bits of biased floats, LDS tables whose entries carry the bias away).

Inputs: 512^2 particles whose noise coordinates span the guarded domain - |pos| log-uniform from 2^-22 of pos_bound up to
pos_bound, a row within 0.1 % of +-pos_bound, a noise scale that puts pos_bound just inside the packed ring's [-2, 2) -
so that the lattice coordinates floor(v + s) of both evaluations take every residue mod 289 on every axis, in negative
and positive cells, multiples of 289 among them, and all six traversal orders of the simplex.  That coverage is computed
on the host (the restatement's arithmetic, fp32 operation by operation) and is a condition of the test.

Every kernel that runs the chain - the fused launches on tile-sorted slots, the single-step kernels over sorted slots -
must then give the bytes of the kernels that do not: the reference-order kernel and the texel-order path (snoise_corners)."""
import numpy as np
import pytest

from helpers import pack_state, unpack_state

pytestmark = pytest.mark.gpu

N = 512
VIEW = (96, 54)
NOISE_SCALE = 1.4e6            # pos_bound = 2^22 / (1.4e6 * 1.5 * 1.001) * 0.999 = 1.9933 (th_step.hip: plan_step)
NOISE_SPEED = 0.05             # noise time 200..220 at time 4000, 0.8 cells on per step
TIME0 = 4000.0
STEPS = (2, 3, 32)             # consecutive step_n calls of one context: 37 steps, launches of 2, 3 and 32 fused steps


def pos_bound():
    nscale = abs(NOISE_SCALE) * (1.0 + 0.5) * 1.001
    return np.float32(min(4194304.0 / nscale * 0.999, 999999.0))


def inputs():
    rng = np.random.default_rng(20289)
    pb = float(pos_bound())
    mag = pb * 0.9999 * 2.0 ** (-22.0 * rng.random((N, N, 2)))
    st = np.empty((N, N, 4), np.float32)
    st[..., :2] = mag * rng.choice([-1.0, 1.0], (N, N, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (N, N, 2))
    # the edge of the domain: the last rows (index i near 1: the largest noise scale) within 0.1 % of +-pos_bound
    edge = pb * (1.0 - 0.001 * rng.random((4, N, 2)))
    st[-4:, :, :2] = edge * rng.choice([-1.0, 1.0], (4, N, 2))
    st[0, :16] = [-1e6, -1e6, 0, 0]                        # a few inert texels pass through
    fw, fh = VIEW
    fl = np.zeros((fh, fw, 4), np.float32)
    fl[..., :2] = rng.uniform(-.01, .01, (fh, fw, 2))
    fl[..., 2] = TIME0 + rng.uniform(-150, 16, (fh, fw))
    fl[..., 3] = 1
    return st, fl


def lattice(st, time, overrides):
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
    live = (np.abs(px) < pos_bound()) & (np.abs(py) < pos_bound())
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


def mod289_int(x):
    """th_math.hpp: fma(-289, floor(x * (1/289)), x) - the product rounded to fp32, the fma exact on these integers"""
    q = np.floor(x.astype(np.float32) * (np.float32(1.0) / np.float32(289.0)))
    return x.astype(np.float64) - 289.0 * q.astype(np.float64)


def coverage_failures(st, time, overrides):
    evals, live = lattice(st, time, overrides)
    bad = []
    saw_289 = False
    for e, (cells, x0) in enumerate(evals):
        for axis, c in zip("xyz", cells):
            c = c[live]
            assert np.abs(c).max() < 2.0 ** 23
            ci = c.astype(np.int64)
            if len(np.unique(ci % 289)) != 289:
                bad.append("evaluation %d axis %s: %d of 289 residues" % (e, axis, len(np.unique(ci % 289))))
            if not ((ci < 0).any() and (ci > 0).any()):
                bad.append("evaluation %d axis %s: one sign only" % (e, axis))
            if not ((ci != 0) & (ci % 289 == 0)).any():
                bad.append("evaluation %d axis %s: no multiple of 289" % (e, axis))
            r = mod289_int(c)
            assert r.min() >= 0 and r.max() <= 289
            saw_289 = saw_289 or bool((r == 289).any())
        l1, l2, l3 = x0[0] < x0[1], x0[1] < x0[2], x0[2] < x0[0]
        orders = np.unique((l1 + 2 * l2 + 4 * l3)[live])
        if not set(range(1, 7)) <= set(orders.tolist()):
            bad.append("evaluation %d: traversal orders %s" % (e, orders.tolist()))
    if not saw_289:
        bad.append("mod289_int never returns 289")
    pb = float(pos_bound())
    for comp in (0, 1):
        for sign in (-1, 1):
            v = st[..., comp][live] * sign
            if not ((v > pb * 0.999) & (v < pb)).any():
                bad.append("no in-domain particle within 0.1 %% of %+d * pos_bound in component %d" % (sign, comp))
    return bad


OVERRIDES = dict(noiseScale=NOISE_SCALE, varyNoiseScale=0.5, noiseSpeed=NOISE_SPEED, varyNoiseSpeed=0.1)

# the library's paths: the chain under test first
PATHS = {
    "fused": dict(bucket=1, fuse=1, rebucket_steps=4),                  # logic_fused_kernel on tile-sorted slots
    "sorted": dict(bucket=1, resort_steps=3),                           # th_step over sorted slots (logic_kernel, logic_sorted_kernel)
    "generic": dict(bucket=1, fuse=1, force_generic=1),                 # the reference-order kernel
    "plain": dict(bucket=0, fuse=0),                                    # texel order, snoise_corners: no table
}


def run_path(fmt, mode, path, st, fl):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts["mode"] = mode
    opts["stateFormat"] = ta.TH_STATE_F16 if fmt == "f16" else ta.TH_STATE_F32
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(N)
    t.state.update(OVERRIDES)
    for k, v in PATHS[path].items():
        t.particles.option(k, v)
    t.particles.upload_texels(st)
    t.flow.set_pixels(fl)
    t.timer.time = TIME0
    first_time = TIME0 + t.timer.step * t.timer.rate
    outs = []
    for n in STEPS:
        if path == "sorted":                                # single launches: th_step_n without fusion steps in texel order
            for _ in range(n):
                t.timer.tick()
                t.step()
        else:
            t.step_n(n)
        outs.append((t.particles.read(0).copy(), t.particles.read(1).copy()))
    t.dispose()
    return outs, first_time


@pytest.fixture(scope="module")
def case():
    st, fl = inputs()
    return {"f32": st, "f16": unpack_state(pack_state(st))}, fl


@pytest.fixture(scope="module")
def runs(case):
    """every (format, mode, path) once, on demand; shared by the comparisons below and left unchanged"""
    states, fl = case
    cache = {}

    def get(fmt, mode, path):
        if (fmt, mode, path) not in cache:
            cache[(fmt, mode, path)] = run_path(fmt, mode, path, states[fmt], fl)
        return cache[(fmt, mode, path)]
    return get


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_inputs_cover_the_hash_domain(case, runs, fmt):
    import tendrils_amd as ta
    states, _ = case
    _, first_time = runs(fmt, ta.TH_MODE_EXACT, "fused")
    bad = coverage_failures(states[fmt], first_time, OVERRIDES)
    assert not bad, "; ".join(bad)


def assert_same_bytes(a, b, what):
    for k, (n, (a0, a1), (b0, b1)) in enumerate(zip(STEPS, a, b)):
        for name, x, y in (("state", a0, b0), ("previous state", a1, b1)):
            diff = (x.view(np.uint32) != y.view(np.uint32)).any(-1)
            assert not diff.any(), "%s, step_n(%d) %s: %d of %d texels differ, first at %s" % (
                what, n, name, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("path,other", [("fused", "generic"), ("fused", "plain"), ("sorted", "plain")])
def test_exact_mode_chain_equals_the_paths_without_it(runs, fmt, path, other):
    import tendrils_amd as ta
    a, _ = runs(fmt, ta.TH_MODE_EXACT, path)
    b, _ = runs(fmt, ta.TH_MODE_EXACT, other)
    assert_same_bytes(a, b, "%s exact: %s against %s" % (fmt, path, other))


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_fast_mode_fused_equals_unfused(runs, fmt):
    import tendrils_amd as ta
    a, _ = runs(fmt, ta.TH_MODE_FAST, "fused")
    b, _ = runs(fmt, ta.TH_MODE_FAST, "plain")
    assert_same_bytes(a, b, "%s fast: fused against plain" % fmt)
