"""Step programs over tile-sorted slots (tendrils_amd/csrc/th_stepprog.hip, th_step_prelude.inc: th_step_args::perm;
th_step_program_view_size): the fused path runs a caller's integrator over whatever slot order the ring is held in and leaves
it there, and with a key it lays that order out and refreshes it itself.  Nothing a program computes may depend on the slot, so
every comparison here is on the bits (bits_equal; the view image with ==), against the same program on a context with
bucket = 0 - texel order - and, for the drift program, against the numpy fp32 trajectory.

Reading a ring buffer back (Particles.read) or asking for its device pointer takes the ring to texel order through the spare
buffer, so th_slot_order is always read BEFORE a read-back, and the n rotations of a call over a sorted ring are checked by what
the two buffers hold (state n, state n - 1) - the addresses of a sorted ring cannot be looked at without un-sorting it.

Shapes: the smallest at which the sorted path exists (sorting_possible: texels >= 2 x flow texels, bucket = 1).  Each program
is compiled once for the module."""
import ctypes as C

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import LOGIC, Particles, Program, StepProgram, run_step_program
from tendrils_amd.tendrils import View, defaults

from helpers import bits_equal, hashed_state
from test_gpu_program import FLOW_ONLY          # the state-program form of this repository's flow-only integrator

pytestmark = pytest.mark.gpu

F = np.float32
N, FLOW = 64, (40, 40)          # 4096 texels over 1600: 2 x 2 flow tiles
ODD, ODD_FLOW = (50, 37), (24, 24)      # 1850 texels: no power of two, count % 8 = 2, an eighth (232) < 256
BAND = (16, 32)                 # rows 16 .. 47 of the 64
BAND_FLOW = (40, 24)            # 960 flow texels: the band's 2048 texels may sort over it (two tiles)
DT = F(0.3125)
TIMES = (np.sin(np.arange(40, dtype=np.float64) * 12.9898) * 43758.5453).astype(F)
COUNTS = (1, 2, 3, 32, 33)
TIME0, STEP_MS = 1000.0, 1000.0 / 60.0

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
TARGETS = """__device__ float4 th_step_main(const th_step_pass &s)
{
    return th_targets(s);
}
"""
STEP_FLOW_ONLY = FLOW_ONLY.replace("th_main(const th_pass &p)", "th_step_main(const th_step_pass &p)").replace("u.time", "p.time").replace("u.dt", "p.dt")
assert "th_step_main" in STEP_FLOW_ONLY and "u.time" not in STEP_FLOW_ONLY and "u.dt" not in STEP_FLOW_ONLY


@pytest.fixture(scope="module")
def programs():
    progs = dict(drift=StepProgram.from_source(DRIFT, name="drift"), coords=StepProgram.from_source(COORDS, name="coords"),
                 index=StepProgram.from_source(INDEX, name="index"), targets=StepProgram.from_source(TARGETS, name="targets"),
                 flow_only=StepProgram.from_source(STEP_FLOW_ONLY, _capi.LogicUniforms, name="step_flow_only"))
    yield progs
    for p in progs.values():
        p.dispose()


def logic_uniforms(view_size=(1.0, 1.0)):
    u = {k: v for k, v in defaults()["state"].items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
    u.update(noiseWeight=0, viewSize=view_size, time=TIME0, dt=STEP_MS)
    return u


def flow_field(shape, seed=13):
    w, h = shape
    flow = np.zeros((h, w, 4), F)
    flow[..., :2] = np.random.default_rng(seed).uniform(-0.01, 0.01, (h, w, 2))
    flow[..., 2] = TIME0 - 10.0
    return flow


def fast_state(w=N, h=N, seed=31):
    """positions in [-1, 1), velocities of +-0.32: a drift step of DT carries a particle a tenth of the view, across a flow tile
    within a few steps; a few inert texels (the sort's class of their own)"""
    st = np.ascontiguousarray(hashed_state(max(w, h), seed, inert_mod=17)[:h, :w])
    st[..., 2:] *= F(32.0)
    return st


def context(shape=(N, N), flow=FLOW, bucket=1, buffers=2, packed=False, fuse=None, row0=0, global_height=0, rebucket=None):
    w, h = shape
    p = Particles(None, dict(shape=[w, h], row0=row0, globalHeight=global_height,
                             stateFormat=_capi.TH_STATE_F16 if packed else _capi.TH_STATE_F32))
    p.setup(buffers)
    p.option("bucket", bucket)
    if fuse is not None:
        p.option("fuse", fuse)
    if rebucket is not None:
        p.option("rebucket_steps", rebucket)
    field = flow_field(flow)
    call("th_flow_resize", p._ctx, *flow)
    call("th_flow_upload", p._ctx, field.ctypes.data_as(_capi._fp))
    return p


def slot_order(p):
    info = _capi.SlotOrderInfo()
    call("th_slot_order", p._ctx, C.byref(info))
    return info.sorted_buffers, info.sorts


def builtin_steps(p, n=2):
    """n single steps of the built-in integrator: with bucket = 1 they leave the ring tile-sorted"""
    p.logic = Program(LOGIC)
    u, t = logic_uniforms(), TIME0
    for _ in range(n):
        t += STEP_MS
        p.step(dict(u, time=t))


def run(p, program, n, uniforms=None, first=0):
    run_step_program(p, program, uniforms or {}, TIMES[first:first + n], DT, n)


def run_flow_only(p, programs, n):
    p.logic = programs["flow_only"]
    p.step_n(logic_uniforms(), TIME0, STEP_MS, n)          # (Particles.step_n sets no key)


def drift_ref(st):
    out = st.copy()
    out[..., 0] = st[..., 0] + st[..., 2] * DT          # float32 multiply, float32 add: what -ffp-contract=off leaves
    out[..., 1] = st[..., 1] + st[..., 3] * DT
    return out


@pytest.fixture(scope="module")
def drifted():
    """states 0 .. 33 of the drift program from fast_state() at the module's two shapes, in numpy fp32: computed once, read-only"""
    out = {}
    for key, (w, h) in (("square", (N, N)), ("odd", ODD)):
        traj = [fast_state(w, h)]
        for _ in range(33):
            traj.append(drift_ref(traj[-1]))
        for t in traj:
            t.setflags(write=False)
        out[key] = traj
    return out


def coords_ref(w, h):
    y, x = np.mgrid[0:h, 0:w]
    coords, index = np.empty((h, w, 4), F), np.empty((h, w, 4), F)
    coords[..., 0], coords[..., 1] = x, y
    coords[..., 2] = (x.astype(F) + F(0.5)) / F(w)
    coords[..., 3] = (y.astype(F) + F(0.5)) / F(h)
    index[..., 0] = y * w + x
    index[..., 1], index[..., 2], index[..., 3] = w, h, 2 * h
    return coords, index


# ---- 1. in place over an order found ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped_twice():
    """what two built-in steps leave of fast_state() - on a bucket = 0 context; the sorted contexts of the tests hold the same bits"""
    p = context(bucket=0)
    p.upload_texels(fast_state(), -1)
    builtin_steps(p)
    out = p.read(0), p.read(1)
    p.dispose()
    for t in out:
        t.setflags(write=False)
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_a_call_without_a_key_runs_in_place_over_the_order_it_finds(programs, stepped_twice, n):
    got = {}
    for bucket in (1, 0):
        p = context(bucket=bucket)
        p.upload_texels(fast_state(), -1)
        builtin_steps(p)
        before = slot_order(p)
        run(p, programs["drift"], n)
        after = slot_order(p)                               # (before the read-backs: they take the ring to texel order)
        got[bucket] = (before, after, p.read(0), p.read(1))
        p.dispose()
    (before, after, cur, prev), (plain_before, plain_after, plain_cur, plain_prev) = got[1], got[0]
    assert before[0] > 0 and plain_before[0] == 0 and plain_after == (0, 0)
    assert after[1] == before[1]                            # no sort, no un-sort ...
    assert after[0] == 2                                    # ... and both outputs sit at the input's slots
    assert bits_equal(cur, plain_cur).all() and bits_equal(prev, plain_prev).all()
    # n rotations: buffers[0] is state n, buffers[1] state n - 1 of the drift from what the built-in steps left
    want = [stepped_twice[0]]
    for _ in range(n):
        want.append(drift_ref(want[-1]))
    assert bits_equal(cur, want[n]).all() and bits_equal(prev, want[n - 1]).all()
    assert (cur != prev).any()


# ---- 2. identity of the particle ----------------------------------------------------------------------------------------------
def test_every_particle_sees_its_own_texel_over_sorted_slots(programs):
    want_coords, want_index = coords_ref(N, N)
    ramp = np.arange(N * N * 4, dtype=F).reshape(N, N, 4)
    for name, n, want in (("coords", 2, want_coords), ("index", 1, want_index), ("targets", 3, ramp), ("coords", 33, want_coords)):
        p = context()
        p.upload_texels(fast_state(), -1)
        call("th_targets_upload", p._ctx, ramp.ctypes.data_as(_capi._fp))
        builtin_steps(p)
        assert slot_order(p)[0] > 0
        run(p, programs[name], n)
        assert slot_order(p)[0] == 2
        assert bits_equal(p.read(0), want).all(), name
        if n > 1:
            assert bits_equal(p.read(1), want).all(), name
        p.dispose()


# ---- 3. awkward counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 33))
def test_counts_that_divide_by_nothing(programs, drifted, n):
    traj = drifted["odd"]
    got = {}
    for bucket in (1, 0):
        for name in ("drift", "flow_only"):
            p = context(ODD, ODD_FLOW, bucket=bucket)
            p.upload_texels(traj[0], -1)
            builtin_steps(p)
            order = slot_order(p)[0]
            assert (order > 0) == (bucket == 1)
            if name == "drift":
                run(p, programs["drift"], n)
            else:
                run_flow_only(p, programs, n)
            assert slot_order(p)[0] == (2 if bucket else 0)
            got[bucket, name] = (p.read(0), p.read(1))
            p.dispose()
    for name in ("drift", "flow_only"):
        for a, b in zip(got[1, name], got[0, name]):
            assert bits_equal(a, b).all(), name
        assert (got[1, name][0] != got[1, name][1]).any()
    # ... and from texel order, keyed: the call's own sort at this shape, against the numpy trajectory
    p = context(ODD, ODD_FLOW)
    p.step_view_size((1.0, 1.0))
    p.upload_texels(traj[0], -1)
    run(p, programs["drift"], n)
    assert slot_order(p)[0] == 2
    assert bits_equal(p.read(0), traj[n]).all() and bits_equal(p.read(1), traj[n - 1]).all()
    p.dispose()


# ---- 4. the call's own order --------------------------------------------------------------------------------------------------
def test_a_keyed_call_lays_out_and_refreshes_its_own_order(programs, drifted):
    traj = drifted["square"]
    # read back after every call (each read-back un-sorts: every call sorts from texel order) ...
    p = context(rebucket=2)
    p.step_view_size((1.0, 1.0))
    p.upload_texels(traj[0], -1)
    plain = context(bucket=0)
    plain.upload_texels(traj[0], -1)
    assert slot_order(p) == (0, 0)
    for k in range(5):
        run(p, programs["drift"], 3, first=3 * k)
        run(plain, programs["drift"], 3, first=3 * k)
        assert slot_order(p)[0] > 0
        for b in (0, 1):
            got = p.read(b)
            assert bits_equal(got, plain.read(b)).all() and bits_equal(got, traj[3 * k + 3 - b]).all(), (k, b)
    p.dispose(), plain.dispose()
    # ... and never in between: the second call on re-sorts FROM a sorted order (rebucket_steps = 2 < 3 steps a call)
    p = context(rebucket=2)
    p.step_view_size((1.0, 1.0))
    p.upload_texels(traj[0], -1)
    sorts = []
    for k in range(5):
        run(p, programs["drift"], 3, first=3 * k)
        order, count = slot_order(p)
        assert order == 2
        sorts.append(count)
    assert sorts[0] == 1 and sorts[-1] - sorts[0] > 1, sorts
    assert bits_equal(p.read(0), traj[15]).all() and bits_equal(p.read(1), traj[14]).all()
    p.dispose()
    # a longer period: the order laid out by the first call serves the next ones
    p = context(rebucket=100)
    p.step_view_size((1.0, 1.0))
    p.upload_texels(traj[0], -1)
    for k in range(3):
        run(p, programs["drift"], 3, first=3 * k)
    assert slot_order(p) == (2, 1)
    assert bits_equal(p.read(0), traj[9]).all() and bits_equal(p.read(1), traj[8]).all()
    p.dispose()
    # without the key, and with the key where the layout is off: no order
    for keyed, bucket in ((False, 1), (True, 0)):
        p = context(bucket=bucket, rebucket=2)
        if keyed:
            p.step_view_size((1.0, 1.0))
        p.upload_texels(traj[0], -1)
        for k in range(2):
            run(p, programs["drift"], 3, first=3 * k)
            assert slot_order(p) == (0, 0), (keyed, bucket)
        assert bits_equal(p.read(0), traj[6]).all() and bits_equal(p.read(1), traj[5]).all()
        p.dispose()


# ---- 5. row band --------------------------------------------------------------------------------------------------------------
def test_a_sorted_row_band_sees_the_whole_textures_coordinates(programs):
    row0, rows = BAND
    st = fast_state()
    want_coords, want_index = coords_ref(N, N)
    whole = context(flow=BAND_FLOW, bucket=0)
    whole.upload_texels(st, -1)
    run_flow_only(whole, programs, 3)
    want_flow = whole.read(0), whole.read(1)
    whole.dispose()
    for name, n, want in (("coords", 2, (want_coords, want_coords)), ("index", 1, (want_index, None)), ("flow_only", 3, want_flow)):
        band = context((N, rows), BAND_FLOW, row0=row0, global_height=N)
        band.step_view_size((1.0, 1.0))
        band.upload_texels(st[row0:row0 + rows], -1)
        if name == "flow_only":
            run_flow_only(band, programs, n)
        else:
            run(band, programs[name], n)
        assert slot_order(band)[0] > 0, name
        for b in (0, 1):
            if want[b] is not None:
                assert bits_equal(band.read(b), want[b][row0:row0 + rows]).all(), (name, b)
        band.dispose()


# ---- 6. the rest of the frame -------------------------------------------------------------------------------------------------
BINS = 1                         # th_draw_info.pipeline: TH_DRAW_BINS


def pipeline(t):
    q = _capi.DrawInfo()
    call("th_draw_query", t.particles._ctx, C.byref(q))
    return q.pipeline


def frames(logic, bucket, st, flow):
    t = ta.Tendrils(View(*FLOW), dict(logicShader=logic) if logic is not None else None)
    t.resize()
    t.setup(N)
    t.particles.option("bucket", bucket)
    t.state["noiseWeight"] = 0
    t.particles.upload_texels(st)
    t.flow.set_pixels(flow)
    t.timer.time = TIME0
    t.timer.step = STEP_MS
    pipes, orders = [], []
    for _ in range(3):
        t.timer.tick()
        t.step()
        t.draw()
        pipes.append(pipeline(t))
        orders.append(slot_order(t.particles)[0])
    t.step_n(3)
    orders.append(slot_order(t.particles)[0])
    limit = F(t.state["speedLimit"])
    stats = t.particles.stats(limit)
    cur, prev = t.particles.read(0), t.particles.read(1)
    fresh = context(bucket=0)
    fresh.upload_texels(cur, 0)
    fresh.upload_texels(prev, 1)
    want = fresh.stats(limit)
    fresh.dispose()
    assert {k: v for k, v in stats.items() if k != "respawned"} == {k: v for k, v in want.items() if k != "respawned"}
    out = dict(pipes=pipes, orders=orders, ring=(cur, prev), flow=t.flow.read(), view=t.read_view())
    t.dispose()
    return out


def test_a_frame_loop_with_a_step_program_stays_on_sorted_slots(programs):
    st = hashed_state(N, 12, inert_mod=13)
    flow = flow_field(FLOW)
    flow[..., 2] = 990.0
    a, b = (frames(programs["flow_only"], bucket, st, flow) for bucket in (1, 0))
    builtin = frames(None, 1, st, flow)
    for x, y in zip(a["ring"], b["ring"]):
        assert bits_equal(x, y).all()
    assert (a["ring"][0] != st).any()
    assert bits_equal(a["flow"], b["flow"]).all()
    assert (a["view"] == b["view"]).all() and a["view"].any()
    # the binned pipeline where the built-in integrator's frames have it, and the ring sorted throughout
    assert BINS in builtin["pipes"] and a["pipes"] == builtin["pipes"]
    assert all(o == 2 for o in a["orders"]) and all(o == 0 for o in b["orders"])


# ---- 7. other rings unchanged -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("three-buffers", "packed", "no-fuse"))
def test_the_other_rings_step_in_texel_order(programs, variant):
    kw = dict(buffers=3) if variant == "three-buffers" else dict(packed=True) if variant == "packed" else dict(fuse=0)
    got = {}
    for bucket in (1, 0):
        p = context(bucket=bucket, **kw)
        p.step_view_size((1.0, 1.0))                        # (a key changes nothing for these rings)
        p.upload_texels(fast_state(), -1)
        builtin_steps(p)
        before = slot_order(p)[0]
        run(p, programs["drift"], 3)
        got[bucket] = (before, slot_order(p)[0], [p.read(k) for k in range(len(p.buffers))])
        p.dispose()
    assert got[1][0] > 0 and got[1][1] == 0 and got[0][:2] == (0, 0)
    for a, b in zip(got[1][2], got[0][2]):
        assert bits_equal(a, b).all()
    assert (got[1][2][0] != got[1][2][1]).any()


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_a_bad_view_size_is_refused_and_the_key_in_force_stays(programs, drifted):
    traj = drifted["square"]
    p = context()
    p.step_view_size((1.0, 1.0))
    for bad, named in (((float("nan"), 1.0), "nan"), ((1.0, 0.0), "= 0"), ((-2.5, 1.0), "-2.5"), ((1.0, float("inf")), "inf")):
        with pytest.raises(ta.TendrilsHipError) as e:
            p.step_view_size(bad)
        assert e.value.status == _capi.TH_ERR_INVALID and named in str(e.value).lower(), str(e.value)
    p.upload_texels(traj[0], -1)
    run(p, programs["drift"], 2)
    assert slot_order(p) == (2, 1)                          # the key of before the refused calls governs
    assert bits_equal(p.read(0), traj[2]).all()             # (texel order again)
    p.step_view_size(None)
    with pytest.raises(ta.TendrilsHipError):
        p.step_view_size((0.0, 0.0))
    run(p, programs["drift"], 2, first=2)
    assert slot_order(p) == (0, 1)                          # cleared, and a refused call does not bring a key back
    assert bits_equal(p.read(0), traj[4]).all() and bits_equal(p.read(1), traj[3]).all()
    p.dispose()
