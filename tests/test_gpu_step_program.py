"""Step programs on the GPU (include/tendrils_hip.h "step programs"; tendrils_amd/csrc/th_stepprog.hip): n steps of a caller's
integrator in one call.  The defining property - a call with n steps leaves the bits and the ring order of n calls with one -
on the fused path and on every ring that takes the single-step path; the times, the step index and the output routing of the
fused launches; the taps against a state program's; row bands; tile-sorted slots and the rest of a frame; errors, the life cycle,
the release library, the Python host.  Every comparison is on the bits unless it says otherwise.  Each program is compiled once
for the module."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import LOGIC, Particles, Program, StepProgram, run_pass, run_step_program
from tendrils_amd.tendrils import View

from helpers import GOLDEN, ROOT, bits_equal, hashed_state, load
from test_gpu_program import FLOW_ONLY          # the state-program form of this repository's flow-only integrator

pytestmark = pytest.mark.gpu

W, H = 50, 30               # 1500 texels: no multiple of 64 or 256
BIG = (1024, 513)           # 525 312 texels: the first size past grid_for's cap of 2048 x 256 lanes - some lanes take two texels
BANDS = ((0, 13), (13, 17))  # rows 0-12 and 13-29
COUNTS = (1, 2, 3, 32, 33, 70)      # odd / even routing and the in-place case; the split at 32; a third launch
F = np.float32

# an arbitrary, non-arithmetic sequence of fp32 values: whatever the library hands a step as `time` is the caller's value
TIMES = (np.sin(np.arange(70, dtype=np.float64) * 12.9898) * 43758.5453).astype(F)
DT = F(0.3125)

ECHO = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4(s.time, s.dt, (float)s.step, s.self.w + 1.0f);
}
"""

DRIFT = """__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self;
    p.x = p.x + p.z * s.dt;
    p.y = p.y + p.w * s.dt;
    return p;
}
"""

COORDS = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4((float)s.x, (float)s.y, s.uv.x, s.uv.y);
}
"""

INDEX = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4((float)s.index, s.dataRes.x, s.dataRes.y, s.geomRes.y);
}
"""

# the taps, at the coordinates the particle's own texel holds - as a step program and as a state program
TAPS = dict(
    flow="return th_flow(%s, %s.self.x, %s.self.y);",
    data="return th_data(%s, %s.self.x, %s.self.y);",
    res="const float2 d = th_data_res(%s), f = th_flow_res(%s); return make_float4(d.x, d.y, f.x, f.y);",
    targets="return th_targets(%s);",
)
STEP_FORM = "__device__ float4 th_step_main(const th_step_pass &s)\n{\n    %s\n}\n"
STATE_FORM = "__device__ float4 th_main(const th_pass &p)\n{\n    %s\n}\n"

STEP_FLOW_ONLY = FLOW_ONLY.replace("th_main(const th_pass &p)", "th_step_main(const th_step_pass &p)").replace("u.time", "p.time").replace("u.dt", "p.dt")
assert "p.time" in STEP_FLOW_ONLY and "p.dt" in STEP_FLOW_ONLY and "th_step_main" in STEP_FLOW_ONLY and "u.time" not in STEP_FLOW_ONLY

STATE_DRIFT = """struct Drift { float k; };
__device__ float4 th_main(const th_pass &p)
{
    const Drift &u = th_uniforms<Drift>(p);
    float4 s = p.self;
    s.x = s.x + s.z * u.k;
    s.y = s.y + s.w * u.k;
    return s;
}
"""


class DriftU(C.Structure):
    _fields_ = [("k", C.c_float)]


def fill(form, body, name):
    return form % (body % ((name,) * body.count("%s")))


@pytest.fixture(scope="module")
def programs():
    progs = dict(
        echo=StepProgram.from_source(ECHO, name="echo"),
        drift=StepProgram.from_source(DRIFT, name="drift"),
        coords=StepProgram.from_source(COORDS, name="coords"),
        index=StepProgram.from_source(INDEX, name="index"),
        flow_only=StepProgram.from_source(STEP_FLOW_ONLY, _capi.LogicUniforms, name="step_flow_only"),
        state_flow_only=Program.from_source(FLOW_ONLY, _capi.LogicUniforms, name="flow_only"),
        state_drift=Program.from_source(STATE_DRIFT, DriftU, name="state_drift"),
    )
    for k, body in TAPS.items():
        progs["step_" + k] = StepProgram.from_source(fill(STEP_FORM, body, "s"), name="step_" + k)
        progs["state_" + k] = Program.from_source(fill(STATE_FORM, body, "p"), name="state_" + k)
    yield progs
    for p in progs.values():
        p.dispose()


def context(w=W, h=H, buffers=2, row0=0, global_height=0, packed=False, fuse=None):
    p = Particles(None, dict(shape=[w, h], row0=row0, globalHeight=global_height,
                             stateFormat=_capi.TH_STATE_F16 if packed else _capi.TH_STATE_F32))
    p.setup(buffers)
    if fuse is not None:
        p.option("fuse", fuse)
    return p


def state(w=W, h=H, seed=1):
    """positions in [-1, 1), velocities of +-0.01, a few inert texels"""
    n = max(w, h)
    return np.ascontiguousarray(hashed_state(n, seed, inert_mod=17)[:h, :w])


def steps(p, program, n, uniforms=None, times=TIMES, dt=DT):
    run_step_program(p, program, uniforms or {}, times[:max(n, 0)], dt, n)


def drift_ref(st, k):
    out = st.copy()
    out[..., 0] = st[..., 0] + st[..., 2] * F(k)          # float32 multiply, float32 add: what -ffp-contract=off leaves
    out[..., 1] = st[..., 1] + st[..., 3] * F(k)
    return out


@pytest.fixture(scope="module")
def drifted():
    """states 0 .. n of the drift program from the module's two start states, in numpy fp32: computed once, never written"""
    out = {}
    for key, (w, h), n in (("small", (W, H), 70), ("big", BIG, 33)):
        traj = [state(w, h, seed=31)]
        for _ in range(n):
            traj.append(drift_ref(traj[-1], DT))
        for t in traj:
            t.setflags(write=False)
        out[key] = traj
    return out


def device_ptrs(p):
    out = []
    for k in range(len(p.buffers)):
        d = C.c_void_p()
        call("th_state_device_ptr", p._ctx, k, C.byref(d))
        out.append(d.value)
    return out


# ---- 1. routing, times, step index ----------------------------------------------------------------------------------------
def echo_state(n, texels=(H, W)):
    """what ECHO leaves after its n-th step (n >= 1) everywhere"""
    out = np.empty(texels + (4,), F)
    out[...] = [TIMES[n - 1], DT, n - 1, n]
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_times_step_index_and_output_routing(programs, n):
    st = state(seed=2)
    st[..., 3] = 0
    p = context()
    p.upload_texels(st, -1)
    before = device_ptrs(p)
    steps(p, programs["echo"], n)
    assert bits_equal(p.read(0), echo_state(n)).all()
    assert bits_equal(p.read(1), echo_state(n - 1) if n > 1 else st).all()
    # n rotations of a two-buffer ring
    assert device_ptrs(p) == (before if n % 2 == 0 else before[::-1])
    p.dispose()


@pytest.mark.parametrize("n", (3, 33))
def test_a_three_buffer_ring_holds_the_last_three_states(programs, n):
    st = state(seed=3)
    st[..., 3] = 0
    p = context(buffers=3)
    p.upload_texels(st, -1)
    before = device_ptrs(p)
    steps(p, programs["echo"], n)
    for k in range(3):
        assert bits_equal(p.read(k), echo_state(n - k)).all(), k
    after = device_ptrs(p)
    assert [after[(k + n) % 3] for k in range(3)] == before
    p.dispose()


# ---- 2. fused = single steps, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_fused_drift_equals_the_steps_one_by_one(programs, drifted, n):
    traj = drifted["small"]
    p = context()
    p.upload_texels(traj[0], -1)
    steps(p, programs["drift"], n)
    assert bits_equal(p.read(0), traj[n]).all()
    assert bits_equal(p.read(1), traj[n - 1]).all()
    p.dispose()


def test_fused_drift_past_the_grid_cap(programs, drifted):
    traj = drifted["big"]
    w, h = BIG
    p = context(w, h)
    p.upload_texels(traj[0], -1)
    steps(p, programs["drift"], 33)                     # a launch of 32 (in place) and one of 1
    assert bits_equal(p.read(0), traj[33]).all()
    assert bits_equal(p.read(1), traj[32]).all()
    steps(p, programs["drift"], 0)
    q = context(w, h, fuse=0)
    q.upload_texels(traj[0], -1)
    steps(q, programs["drift"], 3)
    assert bits_equal(q.read(0), traj[3]).all() and bits_equal(q.read(1), traj[2]).all()
    p.dispose(), q.dispose()


@pytest.mark.parametrize("variant", ("no-fuse", "three-buffers"))
@pytest.mark.parametrize("n", (2, 3, 33))
def test_the_single_step_path_leaves_the_same_bits(programs, drifted, variant, n):
    traj = drifted["small"]
    p = context(fuse=0) if variant == "no-fuse" else context(buffers=3)
    p.upload_texels(traj[0], -1)
    steps(p, programs["drift"], n)
    for k in range(len(p.buffers)):
        assert bits_equal(p.read(k), traj[n - k]).all(), k
    p.dispose()


@pytest.mark.parametrize("n", (2, 3, 33))
def test_a_packed_ring_is_quantised_after_every_step(programs, drifted, n):
    traj = drifted["small"]
    a, b = context(packed=True), context(packed=True)
    for c in (a, b):
        c.upload_texels(traj[0], -1)
    steps(a, programs["drift"], n)
    for k in range(n):
        run_step_program(b, programs["drift"], {}, TIMES[k:k + 1], DT, 1)
    for k in range(2):
        assert bits_equal(a.read(k), b.read(k)).all(), k
    assert (a.read(0) != traj[n]).any()                   # (the unquantised result: not what a packed ring holds)
    a.dispose(), b.dispose()


# ---- 3. against the reference's integrator ----------------------------------------------------------------------------------
def same_values(a, b):
    """equal as VALUES: NaN where NaN, and a zero's sign is free (the built-in adds its zero-weighted noise and target terms)"""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_flow_only_integrator_fused_equals_the_oracle_the_builtin_and_the_state_program(programs, oracle):
    fx = load(os.path.join(GOLDEN, "logic_flow_only_64.npz"))
    meta = fx["meta"]
    n, steps_n = meta["N"], 5
    uniforms = dict(meta["state"])
    uniforms.update(viewSize=meta["viewSize"])
    assert uniforms["noiseWeight"] == 0
    dt = meta["dts"][0]
    t0 = meta["times"][0] - dt
    times, t = [], t0
    for _ in range(steps_n):
        t += dt                                            # in double, as th_step_n and the timer accumulate it
        times.append(t)
    flow = np.ascontiguousarray(fx["flow"], F)
    # the CPU oracle, step by step
    want = [fx["state"]]
    for t in times:
        u = oracle.logic_uniforms(n, n, t, dt, view_size=meta["viewSize"],
                                  **{k: v for k, v in meta["state"].items() if isinstance(v, (int, float)) and not isinstance(v, bool)})
        want.append(oracle.logic_step(u, want[-1], flow))

    def ctx():
        p = context(n, n)
        p.upload_texels(fx["state"], -1)
        call("th_flow_resize", p._ctx, *meta["flowShape"])
        call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
        return p

    results = {}
    p = ctx()                                              # one fused call of the step program, through the host's step_n
    p.logic = programs["flow_only"]
    p.step_n(dict(uniforms), t0, dt, steps_n)
    results["step program"] = (p.read(0), p.read(1))
    p.dispose()
    p = ctx()                                              # the built-in fused integrator
    p.logic = Program(LOGIC)
    p.step_n(dict(uniforms), t0, dt, steps_n)
    results["th_step_n"] = (p.read(0), p.read(1))
    p.dispose()
    p = ctx()                                              # the state-program form, one th_program_run per step
    for t in times:
        run_pass(p, programs["state_flow_only"], dict(uniforms, time=t, dt=dt), _capi.TH_TARGET_RING)
    results["state program"] = (p.read(0), p.read(1))
    p.dispose()
    for name, (cur, prev) in results.items():
        for got, ref in ((cur, want[steps_n]), (prev, want[steps_n - 1])):
            same = same_values(got, ref)
            assert same.all(), (name, int((~same).sum()))
    moved = (results["step program"][0][..., :2] != fx["state"][..., :2]).any(-1)
    assert moved.sum() > n * n // 4                                       # (the steps did integrate)


# ---- 4. taps --------------------------------------------------------------------------------------------------------------
def uv_state():
    """uv values in the texels' xy: texel boundaries of the textures below, the edges, beyond them, NaN and the infinities"""
    st = state(seed=5)
    st[..., :2] = st[..., :2] * F(0.75) + F(0.5)                        # [-0.25, 1.25)
    edge = np.array([0.0, 1.0, -0.0, 1.25, -0.25, 0.5, 2.0, -1.0, 1.0 - 2.0 ** -24, 2.0 ** -30, np.nan, np.inf, -np.inf,
                     1.0 + 2.0 ** -23, -2.0 ** -30, 3e38, -3e38], F)
    st[0, :edge.size, 0] = edge
    st[0, :edge.size, 1] = edge[::-1]
    st[1, :edge.size, 0] = edge
    st[1, :edge.size, 1] = edge
    st[2, :edge.size, 0] = 0.25
    st[2, :edge.size, 1] = edge
    # exact texel boundaries k / n of the widths and heights tapped below
    for row, size in ((3, 97), (4, 61), (5, 37), (6, 23)):
        k = np.arange(W) % (size + 1)
        st[row, :, 0] = (k.astype(F) / F(size))
        st[row, :, 1] = (k[::-1].astype(F) / F(size))
    return st


def test_taps_land_where_a_state_programs_land(programs):
    st = uv_state()
    rng = np.random.default_rng(11)
    image = rng.standard_normal((23, 37, 4)).astype(F)
    flow = rng.standard_normal((61, 97, 4)).astype(F)
    tg = state(seed=9)
    a, b = context(), context()
    for c in (a, b):
        call("th_spawn_image_upload", c._ctx, image.ctypes.data_as(_capi._fp), 37, 23)
        call("th_flow_resize", c._ctx, 97, 61)
        call("th_flow_upload", c._ctx, flow.ctypes.data_as(_capi._fp))
        call("th_targets_upload", c._ctx, tg.ctypes.data_as(_capi._fp))
    cases = [("flow", None), ("targets", None)]
    cases += [(k, s) for k in ("data", "res") for s in (_capi.TH_SOURCE_FLOW, _capi.TH_SOURCE_IMAGE, None)]
    for kind, source in cases:
        uniforms = {} if source is None else dict(spawnData=source)
        for c in (a, b):
            c.upload_texels(st, -1)
        steps(a, programs["step_" + kind], 1, uniforms)
        run_pass(b, programs["state_" + kind], dict(uniforms), _capi.TH_TARGET_RING)
        got, want = a.read(0), b.read(0)
        assert bits_equal(got, want).all(), (kind, source)
        assert bits_equal(a.read(1), st).all()
        if kind == "data" and source is None:
            assert not got.any()                                       # no spawnData reads as zeros
        elif kind in ("flow", "data"):
            assert got.any()
            data = image if source == _capi.TH_SOURCE_IMAGE else flow
            assert np.isnan(st[1, 10, :2]).all() and bits_equal(got[1, 10], data[0, 0]).all()      # a NaN coordinate reads texel 0
    a.dispose(), b.dispose()


# ---- 5. coordinates on row bands --------------------------------------------------------------------------------------------
def coords_ref():
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((H, W, 4), F)
    out[..., 0], out[..., 1] = x, y
    out[..., 2] = (x.astype(F) + F(0.5)) / F(W)
    out[..., 3] = (y.astype(F) + F(0.5)) / F(H)
    index = np.empty((H, W, 4), F)
    index[..., 0] = y * W + x
    index[..., 1], index[..., 2], index[..., 3] = W, H, 2 * H
    return out, index


def test_coordinates_and_drift_whole_and_in_row_bands(programs, drifted):
    want_coords, want_index = coords_ref()
    traj = drifted["small"]
    for name, n, want, prev in (("coords", 2, want_coords, want_coords), ("index", 1, want_index, None),
                                ("drift", 3, traj[3], traj[2])):
        whole = context()
        whole.upload_texels(traj[0], -1)
        steps(whole, programs[name], n)
        assert bits_equal(whole.read(0), want).all(), name
        whole.dispose()
        # two plain contexts holding the bands, no communicator: each sees the coordinates of the unsharded run
        parts, parts_prev = [], []
        for row0, rows in BANDS:
            band = context(h=rows, row0=row0, global_height=H)
            band.upload_texels(traj[0][row0:row0 + rows], -1)
            steps(band, programs[name], n)
            parts.append(band.read(0))
            parts_prev.append(band.read(1))
            band.dispose()
        assert bits_equal(np.concatenate(parts), want).all(), name
        if prev is not None:
            assert bits_equal(np.concatenate(parts_prev), prev).all(), name


# ---- 6. around sorted slots and the rest of the frame ---------------------------------------------------------------------------
def test_step_program_between_steps_over_tile_sorted_slots(programs):
    # (a step only runs over sorted slots when the state has at least twice the flow's texels: 64 x 64 over 40 x 40)
    n, view = 64, (40, 40)
    st = hashed_state(n, 12, inert_mod=13)
    rng = np.random.default_rng(13)
    flow = np.zeros((view[1], view[0], 4), F)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (view[1], view[0], 2))
    flow[..., 2] = 990.0
    out = []
    for bucket in (1, 0):
        t = ta.Tendrils(View(*view))
        t.resize()
        t.setup(n)
        t.particles.option("bucket", bucket)
        t.particles.option("resort_steps", 2)
        t.particles.upload_texels(st)
        t.flow.set_pixels(flow)
        t.timer.time = 1000.0
        t.timer.step = 1000.0 / 60.0
        limit = F(t.state["speedLimit"])
        for _ in range(2):
            t.timer.tick()
            t.step()
        info = _capi.SlotOrderInfo()
        call("th_slot_order", t.particles._ctx, C.byref(info))
        t.step_n(2)                                         # a fused built-in launch: it takes the statistics of what it wrote
        t.particles.stats(limit)
        # three steps of the step program in between
        t.particles.logic = programs["drift"]
        t.particles.step_n({}, t.timer.time, 0.25, 3)
        t.particles.logic = t.logicShader
        stats = t.particles.stats(limit)
        cur, prev = t.particles.read(0), t.particles.read(1)
        fresh = context(n, n)
        fresh.upload_texels(cur, 0)
        fresh.upload_texels(prev, 1)
        want = fresh.stats(limit)
        fresh.dispose()
        assert {k: v for k, v in stats.items() if k != "respawned"} == {k: v for k, v in want.items() if k != "respawned"}
        t.timer.tick()
        t.step()
        t.step_n(2)
        t.draw()
        out.append((info.sorted_buffers, cur, prev, t.particles.read(0), t.particles.read(1), t.flow.read(), t.read_view()))
        t.dispose()
    (was_sorted, *sorted_run), (never_sorted, *plain_run) = out
    assert was_sorted > 0 and never_sorted == 0
    for a, b in zip(sorted_run[:5], plain_run[:5]):
        assert bits_equal(a, b).all()
    assert (sorted_run[5] == plain_run[5]).all() and sorted_run[5].any()


# ---- 7. errors and life cycle ---------------------------------------------------------------------------------------------------
def test_errors_name_their_cause_and_write_nothing(programs):
    st = state(seed=14)
    other = state(seed=15)
    p = context()
    p.upload_texels(st, 0)
    p.upload_texels(other, 1)
    before = device_ptrs(p)
    times = TIMES.ctypes.data_as(_capi._fp)
    drift, state_drift = programs["drift"].handle, programs["state_drift"].handle
    block = (C.c_uint8 * 1025)()
    none = _capi.TH_SOURCE_NONE
    cases = [
        (("th_step_program_run", p._ctx, drift, None, 0, 1, times, DT, 2), "the ring is what the call writes"),
        (("th_step_program_run", p._ctx, drift, None, 0, none, times, DT, -1), "-1 steps"),
        (("th_step_program_run", p._ctx, drift, block, 1025, none, times, DT, 2), "1025"),
        (("th_step_program_run", p._ctx, state_drift, None, 0, none, times, DT, 2), "state program"),
        (("th_program_run", p._ctx, drift, None, 0, none, _capi.TH_TARGET_RING), "step program"),
        (("th_step_program_run", p._ctx, drift, None, 0, none, None, DT, 2), "null times"),
        (("th_step_program_run", p._ctx, drift, None, 0, 99, times, DT, 2), "99"),
    ]
    for args, cause in cases:
        with pytest.raises(ta.TendrilsHipError) as e:
            call(*args)
        assert e.value.status == _capi.TH_ERR_INVALID and cause in str(e.value), (cause, str(e.value))
        assert bits_equal(p.read(0), st).all() and bits_equal(p.read(1), other).all(), cause
        assert device_ptrs(p) == before, cause
    lone = context(buffers=1)
    with pytest.raises(ta.TendrilsHipError) as e:
        call("th_step_program_run", lone._ctx, drift, None, 0, none, times, DT, 1)
    assert e.value.status == _capi.TH_ERR_INVALID and "2 state buffers" in str(e.value)
    lone.dispose()
    # no steps: the ring and its order stay; a block of 1024 bytes is fine
    call("th_step_program_run", p._ctx, drift, None, 0, none, None, DT, 0)
    assert bits_equal(p.read(0), st).all() and bits_equal(p.read(1), other).all() and device_ptrs(p) == before
    call("th_step_program_run", p._ctx, drift, block, 1024, none, times, DT, 1)
    assert bits_equal(p.read(0), drift_ref(st, DT)).all() and bits_equal(p.read(1), st).all()
    # the pass leaves the respawned counter alone
    assert p.stats(0.01)["respawned"] == 0
    p.dispose()


def test_a_destroyed_step_program_keeps_running_where_it_was_loaded(drifted):
    traj = drifted["small"]
    prog = StepProgram.from_source(DRIFT, name="drift_once")
    p, q = context(), context()
    for c in (p, q):
        c.upload_texels(traj[0], -1)
        steps(c, prog, 2)                                                   # two contexts share one program
        assert bits_equal(c.read(0), traj[2]).all()
    handle = C.c_void_p(prog.handle.value)
    prog.dispose()                                                          # th_program_destroy
    for c in (p, q):
        call("th_step_program_run", c._ctx, handle, None, 0, _capi.TH_SOURCE_NONE, TIMES.ctypes.data_as(_capi._fp), DT, 3)
        assert bits_equal(c.read(0), traj[5]).all() and bits_equal(c.read(1), traj[4]).all()
    p.dispose(), q.dispose()


def test_query_reports_no_scratch_for_the_drift_program(programs):
    p = context()
    info = programs["drift"].query(p)
    assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0
    assert 0 < info["vgprs"] <= 512 and 0 < info["sgprs"] <= 128 and 0 < info["code_bytes"] < 4096
    p.dispose()


def test_kernel_timing_puts_events_round_every_launch(programs, drifted):
    traj = drifted["small"]
    p = context()
    p.upload_texels(traj[0], -1)
    call("th_kernel_timing", p._ctx, 1)
    steps(p, programs["drift"], 70)                                         # 32 + 32 + 6
    ms, launches = C.c_float(-1.0), C.c_int32(-1)
    call("th_kernel_timing_read", p._ctx, C.byref(ms), C.byref(launches))
    assert launches.value == 3 and ms.value > 0.0
    assert bits_equal(p.read(0), traj[70]).all()
    p.dispose()


RELEASE = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
CHILD = r'''
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tendrils_amd import _capi
from tendrils_amd.particles import Particles, StepProgram, run_step_program
from helpers import bits_equal, hashed_state
lib = _capi.load()
assert os.path.realpath(lib._name) == os.path.realpath(RELEASE), lib._name
assert not hasattr(lib, "th_comm_loopback_id")
prog = StepProgram.from_source(SOURCE, name="drift")
st = np.ascontiguousarray(hashed_state(50, 21, inert_mod=17)[:30])
p = Particles(None, dict(shape=[50, 30]))
p.setup(2)
p.upload_texels(st, -1)
times = np.arange(33, dtype=np.float32)
run_step_program(p, prog, {}, times, np.float32(0.75), 33)
want = [st]
for _ in range(33):
    s = want[-1].copy()
    s[..., 0] = s[..., 0] + s[..., 2] * np.float32(0.75)
    s[..., 1] = s[..., 1] + s[..., 3] * np.float32(0.75)
    want.append(s)
assert bits_equal(p.read(0), want[33]).all() and bits_equal(p.read(1), want[32]).all()
assert prog.query(p)["scratch_bytes"] == 0
p.dispose(); prog.dispose()
print("release ok")
'''


def test_release_library_runs_a_step_program():
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", os.path.join(ROOT, "tendrils_amd", "csrc"), "release"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, TH_LIB=RELEASE)
    code = "ROOT = %r\nRELEASE = %r\nSOURCE = %r\n" % (ROOT, RELEASE, DRIFT) + CHILD
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "release ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


# ---- 8. the host ------------------------------------------------------------------------------------------------------------------
def test_tendrils_step_n_equals_tick_and_step(programs):
    fx = load(os.path.join(GOLDEN, "logic_flow_only_64.npz"))
    n = fx["meta"]["N"]
    fw, fh = fx["meta"]["flowShape"]
    out = []
    for fused in (False, True):
        t = ta.Tendrils(View(fw, fh), dict(logicShader=programs["flow_only"]))
        t.resize()
        t.setup(n)
        t.state.update({k: v for k, v in fx["meta"]["state"].items() if k in t.state})
        t.particles.upload_texels(fx["state"])
        t.flow.set_pixels(np.ascontiguousarray(fx["flow"], F))
        t.timer.time = 5000.0
        t.timer.step = 1000.0 / 60.0
        ids = [b.id for b in t.particles.buffers]
        if fused:
            t.step_n(4)
        else:
            for _ in range(4):
                t.timer.tick()
                t.step()
        out.append((t.particles.read(0), t.particles.read(1), t.timer.time, [ids.index(b.id) for b in t.particles.buffers]))
        moved = (out[-1][0][..., :2] != fx["state"][..., :2]).any(-1)
        assert moved.sum() > n * n // 4
        t.dispose()
    (a0, a1, at, aorder), (b0, b1, bt, border) = out
    assert bits_equal(a0, b0).all() and bits_equal(a1, b1).all()
    assert (a0 != a1).any()
    assert at == bt and aorder == border == [0, 1]
    # three steps: the ring ends up rotated, alike
    orders = []
    for fused in (False, True):
        t = ta.Tendrils(View(fw, fh), dict(logicShader=programs["drift"]))
        t.resize()
        t.setup(8)
        t.timer.step = 1.0
        ids = [b.id for b in t.particles.buffers]
        if fused:
            t.step_n(3)
        else:
            for _ in range(3):
                t.timer.tick()
                t.step()
        orders.append([ids.index(b.id) for b in t.particles.buffers])
        t.dispose()
    assert orders[0] == orders[1] == [1, 0]


def test_particles_step_n_still_refuses_a_state_program(programs):
    p = context()
    p.logic = programs["state_drift"]
    with pytest.raises(ValueError, match="logic program only"):
        p.step_n(dict(k=1.0), 0.0, 1.0, 2)
    with pytest.raises(ValueError, match="no other target"):
        run_pass(p, programs["drift"], dict(time=1.0, dt=1.0), 0)
    p.dispose()
