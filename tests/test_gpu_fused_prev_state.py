"""The two states a fused launch leaves (th_kernels.hip: TH_LOGIC_FUSED_LOOP).  The state before the last step is stored from
inside the step loop, under the test for the last step, and the new state overwrites the old one in registers; nothing is carried
from step to step.  step_n(n) must leave in BOTH ring buffers what n single step() calls leave, bit for bit - for launches of one
step (the previous state is the input), of two and three, of 31 and 32 (the longest launch) and of 33 (32 + a one-step trailing
launch) - on rings that are no multiple of a wave or a workgroup (300 x 1: a full workgroup and a partial wave of a second one;
17 x 19 = 323), in both storage formats, in texel order and over tile-sorted slots, with the windowed lattice hash and without.
The state holds the particles that leave the hot path: an inert one, a NaN position, a position outside the window's bound but
inside the domain, a particle at rest (0/0 in its first step) and one whose speed underflows in its second step: after
step_n(2) the previous state is the finite one, the newest is NaN."""
import numpy as np
import pytest

from helpers import bits_equal, pack_state, unpack_state

pytestmark = pytest.mark.gpu

VIEW = (12, 10)                          # (a ring is sorted only over a field of at most half as many texels: 120 <= 300 / 2)
TIME0 = 1000.0
NS = (1, 2, 3, 31, 32, 33)
SHAPES = {"300x1": (300, 1), "17x19": (17, 19)}
NOISE = dict(noiseScale=2.125, varyNoiseScale=0.5, noiseSpeed=0.00025, varyNoiseSpeed=0.1)      # (a window the host accepts)
UNIFORMS = {
    "default": dict(NOISE),
    # no force: newVel = (vel * damping) * dt alone, so a speed can be made to underflow at a chosen step (the noise is still
    # evaluated - the kernels are the same - and multiplied by a zero weight)
    "still": dict(NOISE, forceWeight=0.0, varyForce=0.0),
}
INERT, NAN, OUTSIDE, REST, FADING = 0, 1, 2, 3, 4          # texels (first row) of the special particles


def state_of(shape, fading_speed):
    w, h = shape
    rng = np.random.default_rng(w * 31 + h)
    st = np.empty((h, w, 4), np.float32)
    st[..., :2] = rng.uniform(-1.0, 1.0, (h, w, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (h, w, 2))
    st[0, INERT] = [-1e6, -1e6, 0, 0]
    st[0, NAN] = [np.nan, 0.25, 0.001, 0.001]
    st[0, OUTSIDE, :2] = [50.0, -50.0]                      # win_bound = 64 / (2.125 * 1.5) = 20.08 < 50 < pos_bound
    st[0, REST, 2:] = 0.0
    st[0, FADING, 2:] = [fading_speed, 0.0]
    return st


def flow_field():
    rng = np.random.default_rng(7)
    fl = np.zeros((VIEW[1], VIEW[0], 4), np.float32)
    fl[..., :2] = rng.uniform(-.01, .01, (VIEW[1], VIEW[0], 2))
    fl[..., 2] = TIME0 - 10.0
    return fl


def make(shape, fmt, uniforms, **options):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts.update(stateFormat=ta.TH_STATE_F16 if fmt == "f16" else ta.TH_STATE_F32, rows=shape[1], globalHeight=shape[1])
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(shape[0])
    assert t.particles.shape == list(shape)
    t.state.update(UNIFORMS[uniforms])
    for k, v in options.items():
        t.particles.option(k, v)
    t.flow.set_pixels(flow_field())
    return t


def oracle_steps(oracle, t, shape, uniforms, st, n):
    """[state after k steps for k = 0..n] by the restatement, f32"""
    import tendrils_amd as ta
    tm = ta.Timer(0, 0)
    tm.step, tm.time = t.timer.step, TIME0
    out, fl = [st], flow_field()
    for _ in range(n):
        tm.tick()
        u = oracle.logic_uniforms(shape[0], shape[1], tm.time, tm.dt, view_size=t.viewSize,
                                  **{k: v for k, v in t.state.items() if isinstance(v, (int, float))})
        out.append(oracle.logic_step(u, out[-1], fl))
    return out


@pytest.fixture(scope="module")
def fading(oracle):
    """per shape: an x velocity whose particle is finite after one step of the "still" uniforms and NaN after two (its squared
    speed underflows to zero in the second step: min(0, limit) / 0), found with the restatement"""
    found = {}
    for name, shape in SHAPES.items():
        t = make(shape, "f32", "still")
        for v in np.arange(2.0e-23, 9.0e-23, 0.25e-23):
            s = oracle_steps(oracle, t, shape, "still", state_of(shape, np.float32(v)), 2)
            if np.isfinite(s[1][0, FADING]).all() and np.isnan(s[2][0, FADING]).all():
                found[name] = np.float32(v)
                break
        t.dispose()
        assert name in found, "no speed between 2e-23 and 9e-23 underflows in its second step"
    return found


@pytest.fixture(scope="module")
def single_steps(fading):
    """(shape, format, uniforms) -> [state after k single step() calls in texel order, unfused, k = 0..33], computed once"""
    cache = {}

    def get(shape_name, fmt, uniforms):
        key = (shape_name, fmt, uniforms)
        if key not in cache:
            shape = SHAPES[shape_name]
            st = state_of(shape, fading[shape_name])
            if fmt == "f16":
                st = unpack_state(pack_state(st))
            t = make(shape, fmt, uniforms, bucket=0, fuse=0, graph=0)
            t.particles.upload_texels(st)
            t.timer.time = TIME0
            states = [st]
            for k in range(max(NS)):
                t.timer.tick()
                t.step()
                states.append(t.particles.read(0).copy())
                assert bits_equal(t.particles.read(1), states[-2]).all(), "single steps: the ring's previous state"
            t.dispose()
            cache[key] = states
        return cache[key]
    return get


def same(got, want, what):
    diff = ~bits_equal(got, want).all(-1)
    assert not diff.any(), "%s: %d of %d texels differ, first at %s" % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


@pytest.mark.parametrize("uniforms", list(UNIFORMS))
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_both_ring_buffers_after_a_fused_call_equal_single_steps(single_steps, oracle, shape_name, fmt, uniforms):
    import ctypes as C
    from tendrils_amd import _capi
    shape = SHAPES[shape_name]
    want = single_steps(shape_name, fmt, uniforms)
    for bucket in (0, 1):
        for window in (0, 1):
            t = make(shape, fmt, uniforms, bucket=bucket, fuse=1, hash_window=window)
            if fmt == "f32" and bucket == 0 and window == 1:
                by_oracle = oracle_steps(oracle, t, shape, uniforms, want[0], max(NS))
            fused = 0
            for n in NS:
                t.particles.upload_texels(want[0])
                t.timer.time = TIME0
                t.step_n(n)
                fused += (n + 31) // 32 if n > 1 else 0          # (step_n(1) is a single step)
                what = "%s %s %s, TH_BUCKET=%d, window %d, step_n(%d)" % (shape_name, fmt, uniforms, bucket, window, n)
                cur, prev = t.particles.read(0).copy(), t.particles.read(1).copy()
                same(cur, want[n], what + ", newest state")
                same(prev, want[n - 1], what + ", previous state")
                if fmt == "f32" and bucket == 0 and window == 1:
                    same(cur, by_oracle[n], what + ", newest state against the restatement")
                    same(prev, by_oracle[n - 1], what + ", previous state against the restatement")
            launches = t.particles.option("hash_window_launches")
            info = _capi.SlotOrderInfo()
            _capi.call("th_slot_order", t.particles._ctx, C.byref(info))
            t.dispose()
            assert launches == (fused if window else 0), "fused launches over the window"
            assert (info.sorts > 0) == bool(bucket), "TH_BUCKET=1: the fused launches ran over tile-sorted slots"


def test_the_previous_state_of_a_particle_that_turns_nan_is_the_state_before(single_steps):
    """what the cases above compare, spelled out for the particles it is about: after step_n(2) the fading particle's previous
    state is finite and its newest state NaN; the particle at rest is NaN in both; the inert one is untouched in both"""
    for shape_name, shape in SHAPES.items():
        want = single_steps(shape_name, "f32", "still")
        assert np.isfinite(want[1][0, FADING]).all() and np.isnan(want[2][0, FADING]).all()
        assert np.isnan(want[1][0, REST]).all() and np.isnan(want[1][0, NAN]).all()
        for bucket in (0, 1):
            t = make(shape, "f32", "still", bucket=bucket, fuse=1)
            t.particles.upload_texels(want[0])
            t.timer.time = TIME0
            t.step_n(2)
            cur, prev = t.particles.read(0), t.particles.read(1)
            t.dispose()
            assert np.isfinite(prev[0, FADING]).all() and bits_equal(prev[0, FADING], want[1][0, FADING]).all()
            assert np.isnan(cur[0, FADING]).all()
            assert np.isnan(prev[0, REST]).all() and np.isnan(cur[0, REST]).all()
            for b in (cur, prev):
                assert bits_equal(b[0, INERT], want[0][0, INERT]).all()
