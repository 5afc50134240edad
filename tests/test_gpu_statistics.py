"""th_stats against a numpy reference written from the description of th_counters (tests/prims.py: stats_reference), through
the public ABI: (a) the pass over the state (stats_kernel + stats_fold_kernel), (b) the statistics a fused launch takes while
the state is in registers (stats_take, folded by stats_fold_parts_kernel / stats_fold_kernel).  Counts and the maximum
exactly; sum_speed within N * 2^-53 * sum (prims.sum_speed_bound: derived from the additions, not measured).

The states hold every class of texel a known number of times: inert, inert with a NaN velocity, a NaN in each component
alone, infinite velocities, velocities whose squares overflow float32 (live, not NaN, not finite: counted in `live` only),
speeds exactly at the cap, one ulp below and above it, denormal velocities, particles at rest.

Not covered: the second level of launch_stats_fold (more than 4096 * 256 partials: above 2^26 particles) - a state larger
than a test should allocate."""
import numpy as np
import pytest

import prims

pytestmark = pytest.mark.gpu

f32 = np.float32
LIMIT = 0.01            # the default speedLimit
CLASSES = 21


def cap_of(limit):
    return f32(f32(limit) * f32(1.0 - 2.0 ** -20))


def crafted_state(n, limit, seed):
    """[n, n, 4]: live particles slower than 0.4 * limit, and k texels of each class scattered over them (k = n * n // 50, at
    least 1).  Returns the state and what `limit` must count in it: known, not computed from the state."""
    rng = np.random.default_rng(seed)
    N = n * n
    st = np.empty((N, 4), f32)
    st[:, :2] = rng.uniform(-1, 1, (N, 2))
    mag, ang = rng.uniform(0, 0.4 * limit, N), rng.uniform(0, 2 * np.pi, N)
    st[:, 2], st[:, 3] = mag * np.cos(ang), mag * np.sin(ang)
    cap, cap2 = cap_of(limit), cap_of(limit / 4)
    nan, inf, up, down = f32(np.nan), f32(np.inf), f32(np.inf), f32(0)
    k = max(1, N // 50)
    order = rng.permutation(N)
    taken = [0]

    def put(x, y, z, w):
        rows = order[taken[0]:taken[0] + k]
        taken[0] += k
        for c, v in enumerate((x, y, z, w)):
            if v is not None:               # (None: the random value stays)
                st[rows, c] = v

    put(-1e6, -1e6, 0, 0)                                       # inert
    put(-1e6, -1e6, nan, 0.001)                                 # inert, NaN velocity: `nan` alone
    put(nan, None, None, None)                                  # a NaN in each component alone: live and nan
    put(None, nan, None, None)
    put(None, None, nan, None)
    put(None, None, None, nan)
    put(None, None, inf, None)                                  # infinite: live, not nan, not finite
    put(None, None, None, -inf)
    put(None, None, 2e19, 0)                                    # the square overflows
    put(None, None, 1.5e19, -1.5e19)                            # the squares do not, their sum does
    put(None, None, cap, 0)                                     # exactly at the cap, along either axis
    put(None, None, 0, -cap)
    put(None, None, np.nextafter(cap, down), 0)                 # one ulp below
    put(None, None, 0, np.nextafter(cap, up))                   # one ulp above: the fastest finite particle
    put(None, None, 1e-42, -1e-43)                              # denormal velocity: speed 0
    put(None, None, 1e-20, 0)                                   # the square is denormal
    put(None, None, 0, 0)                                       # at rest
    put(-1e6, 0.3, None, None)                                  # x alone at the inert value: live
    put(None, None, cap2, 0)                                    # the same three around the cap of the second limit
    put(None, None, 0, np.nextafter(cap2, down))
    put(None, None, -np.nextafter(cap2, up), 0)
    assert taken[0] == CLASSES * k <= N
    known = dict(particles=N, live=N - 2 * k, nan=5 * k, capped=3 * k, max_speed=float(np.nextafter(cap, up)))
    return st.reshape(n, n, 4), known


def make_tendrils(n, packed=False, overrides=None):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    if packed:
        opts["stateFormat"] = ta.TH_STATE_F16
    t = ta.Tendrils(View(96, 54), opts)
    t.resize()
    t.setup(n)
    t.state.update(overrides or {})
    return t


# ---- (a) the pass over the state ------------------------------------------------------------------------------------------
# particles: 100 (below one workgroup), 2500 (not a multiple of 64), 110 889 (nor of 256), 1 046 529 (above 1024 blocks x 256:
# the grid-stride loop of stats_kernel runs more than once)
@pytest.mark.parametrize("n", [10, 50, 333, 1023])
def test_statistics_pass_counts_every_class(n):
    st, known = crafted_state(n, LIMIT, 1000 + n)
    t = make_tendrils(n)
    t.particles.upload_texels(st)
    for limit in (LIMIT, LIMIT / 4):
        got = t.particles.stats(limit)
        want = prims.stats_reference(st, limit)
        if limit == LIMIT:
            assert {k: want[k] for k in known} == known
        prims.assert_counters(got, want, "%d x %d, limit %g" % (n, n, limit))
    t.dispose()


def test_statistics_pass_over_velocities_whose_squares_are_denormal():
    """Every speed lies near 1e-20: z * z and w * w are float32 denormals, the maximum and every term of the sum depend on them."""
    n = 50
    rng = np.random.default_rng(7)
    st = np.zeros((n, n, 4), f32)
    st[..., :2] = rng.uniform(-1, 1, (n, n, 2))
    st[..., 2:] = rng.uniform(-3e-20, 3e-20, (n, n, 2))
    st[::7, ::3, 2:] = 0
    t = make_tendrils(n)
    t.particles.upload_texels(st)
    want = prims.stats_reference(st, LIMIT)
    assert 0 < want["max_speed"] < 1e-19 and want["capped"] == 0
    prims.assert_counters(t.particles.stats(LIMIT), want, "denormal squares")
    prims.assert_counters(t.particles.stats(1e-20), prims.stats_reference(st, 1e-20), "denormal squares, limit 1e-20")
    t.dispose()


# ---- (b) the statistics taken by the fused launch -------------------------------------------------------------------------
# 50^2, 333^2, 1023^2: the last wave is partly filled in texel order (and the eighths of the bucketed launch end inside waves);
# 1023^2 = 1 046 529 particles leave more than 4096 partials: launch_stats_fold takes its stats_fold_parts_kernel level
@pytest.mark.parametrize("packed", [False, True], ids=["f32", "packed"])
@pytest.mark.parametrize("bucket", [0, 1])
@pytest.mark.parametrize("n", [50, 333, 1023])
def test_statistics_taken_by_the_fused_launch_equal_the_reference(n, bucket, packed):
    """NaN and infinite inputs stay in: they propagate through the steps and must be counted, not summed.  The inert texels
    with a NaN velocity pass through every step as they are: `nan` must see them by their velocity alone."""
    st, _ = crafted_state(n, LIMIT, 2000 + n)
    rng = np.random.default_rng(n)
    fl = np.zeros((54, 96, 4), f32)
    fl[..., :2] = rng.uniform(-.01, .01, (54, 96, 2))
    fl[..., 2] = 4000 + rng.uniform(-150, 16, (54, 96))
    fl[..., 3] = 1
    t = make_tendrils(n, packed, {"forceWeight": 0.2, "noiseWeight": 0.02})      # forces that drive many particles into the limit
    assert t.particles.option("bucket", bucket) == bucket and t.particles.option("fuse") == 1
    t.particles.upload_texels(st)
    t.flow.set_pixels(fl)
    t.timer.time = 4000.0
    limit = t.state["speedLimit"]
    assert limit == LIMIT
    for steps in (3, 4):                 # (both ring parities)
        t.step_n(steps)
        got = t.particles.stats(limit)   # the launch's own speedLimit: its partials, folded
        state = t.particles.read(0)
        want = prims.stats_reference(state, limit)
        inert = (state[..., 0] == prims.INERT) & (state[..., 1] == prims.INERT)
        assert (inert & np.isnan(state[..., 2])).sum() > 0 and 0 < want["capped"] < want["live"] and want["nan"] > 0
        prims.assert_counters(got, want, "%d x %d, bucket %d, %s, after %d fused steps" % (n, n, bucket, "packed" if packed else "f32", steps))
    t.dispose()
