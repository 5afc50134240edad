"""Step programs on the packed ring (TH_STATE_F16, 8 bytes a texel; th_step_prelude.inc: th_step_packed_kernel; th_stepprog.hip):
on a two-buffer packed ring with `fuse` on, a call runs its steps fused and in place on the packed texels - at most 32 steps a
launch, no f32 staging - and leaves, bit for bit, what the staged single-step path leaves (unpack, one f32 step, pack, once per
step): the state is quantised after EVERY step inside the launch.  Held against that path (`fuse` = 0), against the numpy codec
of helpers.py, against n calls of one step; the times, the step index and the split at 32; the particle's identity, whole and
on a row band; the taps; a ring the built-in integrator left tile-sorted; the Python host.  Every comparison is on the bits
(bits_equal: NaN equals NaN whatever its payload) and over every texel.

Shapes: those of test_gpu_step_program.py - 50 x 30 (1500 texels: no multiple of 64 or 256) and 1024 x 513 (the first size at
which lanes take two texels).  Each program is compiled once for the module; the numpy trajectories are computed once."""
import ctypes as C
import os

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import StepProgram, run_step_program
from tendrils_amd.tendrils import View

from helpers import GOLDEN, bits_equal, load, pack_state, unpack_state
from test_gpu_step_program import BANDS, BIG, DRIFT, DT, H, STEP_FLOW_ONLY, TIMES, W, context, device_ptrs, drift_ref, state, steps
import test_gpu_step_program_slots as slots

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (1, 2, 3, 32, 33, 70)      # odd / even routing and the in-place case; the split at 32; a third launch

# texels planted in row 0: the codec's edges (helpers.py's numpy codec handles every one of them)
EDGES = np.array([
    [2.5, -2.5, 70000.0, -70000.0],                      # clamp; fp16 overflow to +-inf
    [-2.0, 1.99997, 1e-8, -1e-8],                        # underflow to +-0
    [np.nan, 0.3, 0.01, 0.01],                           # NaN position
    [0.1, np.nan, 0.0, -0.0],                            # NaN position; signed zero
    [3.5 / 16384, 4.5 / 16384, 6e-8, 6.1e-5],            # rint ties; fp16 subnormals
    [-1e6, -1e6, 0.01, 0.02],                            # inert
    [-1e6, 0.5, 0.01, 0.01],                             # half-inert
    [0.5, 0.5, np.inf, -np.inf],                         # infinite velocity
    [1.9999, -1.9999, 0.5, -0.5],                        # clamp near the edge
], F)

# values that survive the codec: +-0.5 and dt = 0.3125 (5120 quanta) as positions, small integers as fp16 velocities
ECHO = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4(s.time > 0.0f ? 0.5f : -0.5f, s.dt, (float)s.step, s.self.w + 1.0f);
}
"""
IDENTITY = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4(0.0f, 0.0f, (float)s.x, (float)s.y);
}
"""
TARGETS = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return th_targets(s);
}
"""


@pytest.fixture(scope="module")
def programs():
    progs = dict(drift=StepProgram.from_source(DRIFT, name="drift"), echo=StepProgram.from_source(ECHO, name="packed_echo"),
                 identity=StepProgram.from_source(IDENTITY, name="identity"), targets=StepProgram.from_source(TARGETS, name="targets"),
                 flow_only=StepProgram.from_source(STEP_FLOW_ONLY, _capi.LogicUniforms, name="step_flow_only"))
    yield progs
    for p in progs.values():
        p.dispose()


def quantised(st):
    """what a packed ring holds of a state"""
    return unpack_state(pack_state(st))


def start(w=W, h=H, seed=31):
    st = state(w, h, seed)
    st[0, :len(EDGES)] = EDGES
    return st


@pytest.fixture(scope="module")
def drifted():
    """per shape: (the states 0 .. n a packed ring holds under the drift program, the unquantised fp32 states), in numpy:
    computed once, never written"""
    out = {}
    with np.errstate(all="ignore"):
        for key, (w, h), n in (("small", (W, H), 70), ("big", BIG, 33)):
            plain = [start(w, h)]
            traj = [quantised(plain[0])]
            for _ in range(n):
                plain.append(drift_ref(plain[-1], DT))
                traj.append(quantised(drift_ref(traj[-1], DT)))
            for t in plain + traj:
                t.setflags(write=False)
            out[key] = (traj, plain)
    return out


def launches(p):
    ms, count = C.c_float(-1.0), C.c_int32(-1)
    call("th_kernel_timing_read", p._ctx, C.byref(ms), C.byref(count))
    return count.value, ms.value


def both(p):
    return p.read(0), p.read(1)


def same(a, b):
    return all(bits_equal(x, y).all() for x, y in zip(a, b))


# ---- 1. launch count ----------------------------------------------------------------------------------------------------------
def test_a_packed_call_takes_one_launch_per_32_steps(programs, drifted):
    traj, _ = drifted["small"]
    for n, want in ((20, 1), (33, 2), (1, 1)):
        p = context(packed=True)
        p.upload_texels(traj[0], -1)
        call("th_kernel_timing", p._ctx, 1)
        steps(p, programs["drift"], n)
        count, ms = launches(p)
        assert count == want and ms > 0.0, (n, count, ms)
        p.dispose()
    # the rings that keep the single-step path: n launches
    for kw in (dict(buffers=3), dict(fuse=0)):
        p = context(packed=True, **kw)
        p.upload_texels(traj[0], -1)
        call("th_kernel_timing", p._ctx, 1)
        steps(p, programs["drift"], 20)
        count, ms = launches(p)
        assert count == 20 and ms > 0.0, (kw, count, ms)
        p.dispose()


# ---- 2. against the staged path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [("small", n) for n in COUNTS] + [("big", 2), ("big", 33)])
def test_fused_equals_the_staged_single_steps(programs, drifted, shape, n):
    traj, _ = drifted[shape]
    h, w = traj[0].shape[:2]
    a, b = context(w, h, packed=True), context(w, h, packed=True, fuse=0)
    for c in (a, b):
        c.upload_texels(traj[0], -1)
        steps(c, programs["drift"], n)
    for k in range(2):
        got, want = a.read(k), b.read(k)
        assert got.shape == (h, w, 4) and bits_equal(got, want).all(), (k, int((~bits_equal(got, want)).sum()))
    a.dispose(), b.dispose()


# ---- 3. against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [("small", n) for n in COUNTS] + [("big", 2), ("big", 33)])
def test_fused_equals_the_numpy_codec_after_every_step(programs, drifted, shape, n):
    traj, plain = drifted[shape]
    h, w = traj[0].shape[:2]
    p = context(w, h, packed=True)
    p.upload_texels(plain[0], -1)                            # (the upload packs: the ring holds traj[0])
    steps(p, programs["drift"], n)
    cur, prev = both(p)
    assert bits_equal(cur, traj[n]).all(), int((~bits_equal(cur, traj[n])).sum())
    if n >= 2:
        assert bits_equal(prev, traj[n - 1]).all(), int((~bits_equal(prev, traj[n - 1])).sum())
    else:
        assert bits_equal(prev, traj[0]).all()
    assert (~bits_equal(cur, plain[n])).any()                # (the unquantised result: not what a packed ring holds)
    if n == 33:
        # a kernel that quantised at the end of a launch alone would leave this
        assert (~bits_equal(cur, quantised(plain[n]))).any()
    p.dispose()


# ---- 4. n calls of one step = one call of n -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 3, 33))
def test_n_calls_of_one_step_equal_one_call_of_n(programs, drifted, n):
    traj, _ = drifted["small"]
    a, b = context(packed=True), context(packed=True)
    before = {}
    for c in (a, b):
        c.upload_texels(traj[0], -1)
        before[c] = device_ptrs(c)
    steps(a, programs["drift"], n)
    for k in range(n):
        run_step_program(b, programs["drift"], {}, TIMES[k:k + 1], DT, 1)
    assert same(both(a), both(b))
    for c in (a, b):
        assert device_ptrs(c) == (before[c] if n % 2 == 0 else before[c][::-1])
    a.dispose(), b.dispose()


# ---- 5. times, step index, the split at 32 --------------------------------------------------------------------------------------
def echo_state(n):
    """what ECHO leaves after its n-th step (n >= 1) everywhere"""
    out = np.empty((H, W, 4), F)
    out[...] = [0.5 if TIMES[n - 1] > 0 else -0.5, DT, n - 1, n]
    return out


@pytest.mark.parametrize("n", (1, 33, 70))
def test_times_step_index_and_the_split_at_32(programs, n):
    assert TIMES[0] == 0 and TIMES[32] > 0 and TIMES[69] < 0     # (both signs, and a zero: the sign test's other side)
    st = state(seed=2)
    st[..., 3] = 0
    p = context(packed=True)
    p.upload_texels(st, -1)
    steps(p, programs["echo"], n)
    assert bits_equal(p.read(0), echo_state(n)).all()
    assert bits_equal(p.read(1), echo_state(n - 1) if n > 1 else quantised(st)).all()
    p.dispose()


# ---- 6. identity ----------------------------------------------------------------------------------------------------------------
def test_every_particle_sees_its_own_texel_whole_and_on_a_row_band(programs):
    w, h = BIG
    y, x = np.mgrid[0:h, 0:w]
    want = np.zeros((h, w, 4), F)
    want[..., 2], want[..., 3] = x, y                        # (fp16 holds integers up to 2048)
    p = context(w, h, packed=True)
    p.upload_texels(np.zeros((h, w, 4), F), -1)              # (the program reads nothing of its own state)
    steps(p, programs["identity"], 2)
    assert bits_equal(p.read(0), want).all() and bits_equal(p.read(1), want).all()
    p.dispose()
    # a packed row band: y is the whole texture's, th_targets the band's own texel
    y, x = np.mgrid[0:H, 0:W]
    want = np.zeros((H, W, 4), F)
    want[..., 2], want[..., 3] = x, y
    tg = np.empty((H, W, 4), F)
    tg[..., 0], tg[..., 1], tg[..., 2], tg[..., 3] = x / F(64.0), -y / F(32.0), x, y      # exact through the codec
    assert bits_equal(quantised(tg), tg).all()
    for name, n, ref in (("identity", 1, want), ("identity", 33, want), ("targets", 3, tg)):
        parts, parts_prev = [], []
        for row0, rows in BANDS:
            band = context(h=rows, row0=row0, global_height=H, packed=True)
            band.upload_texels(np.zeros((rows, W, 4), F), -1)
            call("th_targets_upload", band._ctx, np.ascontiguousarray(tg[row0:row0 + rows]).ctypes.data_as(_capi._fp))
            call("th_kernel_timing", band._ctx, 1)
            steps(band, programs[name], n)
            assert launches(band)[0] == (n + 31) // 32
            parts.append(band.read(0))
            parts_prev.append(band.read(1))
            band.dispose()
        assert bits_equal(np.concatenate(parts), ref).all(), name
        if n > 1:
            assert bits_equal(np.concatenate(parts_prev), ref).all(), name


# ---- 7. taps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (20, 33))
def test_the_flow_only_integrator_fused_equals_the_staged_path(programs, n):
    st = start()
    flow = slots.flow_field((24, 24))
    got = []
    for fuse in (None, 0):
        p = context(packed=True, fuse=fuse)
        p.upload_texels(st, -1)
        call("th_flow_resize", p._ctx, 24, 24)
        call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
        call("th_kernel_timing", p._ctx, 1)
        slots.run_flow_only(p, programs, n)
        assert launches(p)[0] == ((n + 31) // 32 if fuse is None else n)
        got.append(both(p))
        p.dispose()
    assert same(got[0], got[1])
    moved = (got[0][0][..., :2] != quantised(st)[..., :2]).any(-1)
    assert moved.sum() > W * H // 4                          # (the steps did integrate)
    assert (~bits_equal(got[0][0], got[0][1])).any()


# ---- 8. a ring the built-in integrator left tile-sorted ----------------------------------------------------------------------------
def test_a_tile_sorted_packed_ring_goes_to_texel_order_first(programs):
    got = {}
    for bucket in (1, 0):
        p = slots.context(bucket=bucket, packed=True)
        p.upload_texels(slots.fast_state(), -1)
        slots.builtin_steps(p)
        before = slots.slot_order(p)[0]
        call("th_kernel_timing", p._ctx, 1)
        launches(p)                                          # (from here on)
        slots.run(p, programs["drift"], 33)
        count = launches(p)[0]
        got[bucket] = (before, slots.slot_order(p)[0], count, both(p))
        p.dispose()
    assert got[1][0] > 0 and got[0][0] == 0                  # the built-in steps did sort the one ...
    assert got[1][1] == 0 and got[0][1] == 0                 # ... and the call leaves texel order
    assert got[1][2] == 2 and got[0][2] == 2
    assert same(got[1][3], got[0][3])
    assert (~bits_equal(got[1][3][0], got[1][3][1])).any()


# ---- 9. the Python host -----------------------------------------------------------------------------------------------------------
def test_tendrils_step_n_on_a_packed_ring_equals_tick_and_step_in_one_launch(programs):
    fx = load(os.path.join(GOLDEN, "logic_flow_only_64.npz"))
    n = fx["meta"]["N"]
    fw, fh = fx["meta"]["flowShape"]
    out = []
    for fused in (False, True):
        t = ta.Tendrils(View(fw, fh), dict(stateFormat=_capi.TH_STATE_F16, logicShader=programs["flow_only"]))
        t.resize()
        t.setup(n)
        t.state.update({k: v for k, v in fx["meta"]["state"].items() if k in t.state})
        t.particles.upload_texels(fx["state"])
        t.flow.set_pixels(np.ascontiguousarray(fx["flow"], F))
        t.timer.time = 5000.0
        t.timer.step = 1000.0 / 60.0
        call("th_kernel_timing", t.particles._ctx, 1)
        if fused:
            t.step_n(20)
        else:
            for _ in range(20):
                t.timer.tick()
                t.step()
        count = launches(t.particles)[0]
        out.append((t.particles.read(0), t.particles.read(1), t.timer.time, count))
        t.dispose()
    (a0, a1, at, acount), (b0, b1, bt, bcount) = out
    assert bits_equal(a0, b0).all() and bits_equal(a1, b1).all()
    assert (~bits_equal(a0, a1)).any() and (a0[..., :2] != quantised(fx["state"])[..., :2]).any(-1).sum() > n * n // 4
    assert at == bt
    assert bcount == 1 and acount == 20                      # one fused launch; a launch per step()
