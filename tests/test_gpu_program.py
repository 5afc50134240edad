"""User programs on the GPU (include/tendrils_hip.h "user programs"; tendrils_amd/csrc/th_program.hip): a pass the caller wrote,
compiled through hiprtc, run with the ring semantics of th_step and the spawn passes - over f32 and packed rings, whole
textures and row bands, tile-sorted slots, from the testing and the release library.  Every comparison is on the bits unless
it says otherwise.  The programs read through the accessors alone; each is compiled once for the module."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import LOGIC, Particles, Program, run_pass
from tendrils_amd.tendrils import View

from helpers import GOLDEN, ROOT, bits_equal, hashed_state, load

pytestmark = pytest.mark.gpu

W, H = 50, 30               # 1500 texels: no multiple of 64 or 256
BANDS = ((0, 13), (13, 17))  # rows 0-12 and 13-29
F = np.float32


class DriftU(C.Structure):
    _fields_ = [("k", C.c_float)]


DRIFT = """struct Drift { float k; };
__device__ float4 th_main(const th_pass &p)
{
    const Drift &u = th_uniforms<Drift>(p);
    float4 s = p.self;
    s.x = s.x + s.z * u.k;
    s.y = s.y + s.w * u.k;
    return s;
}
"""

COORDS = """__device__ float4 th_main(const th_pass &p)
{
    return make_float4((float)p.x, (float)p.y, p.uv.x, p.uv.y);
}
"""

INDEX = """__device__ float4 th_main(const th_pass &p)
{
    return make_float4((float)p.index, p.dataRes.x, p.dataRes.y, p.geomRes.y);
}
"""

# spawnData at the uv the particle's own texel names, mirrored; its resolution goes out with a second program
DATA = """__device__ float4 th_main(const th_pass &p)
{
    return th_data(p, 1.0f - p.self.x, 1.0f - p.self.y);
}
"""

DATA_RES = """__device__ float4 th_main(const th_pass &p)
{
    const float2 d = th_data_res(p), f = th_flow_res(p);
    return make_float4(d.x, d.y, f.x, f.y);
}
"""

# the row above, through the accessor (row 0 reads itself: clamped) - on a band whose first row is not 0 this leaves the band
ROW_ABOVE = """__device__ float4 th_main(const th_pass &p)
{
    return th_particles(p, p.x, p.y - 1);
}
"""

TARGETS = """__device__ float4 th_main(const th_pass &p)
{
    const float4 t = th_targets(p), r = th_particles(p, p.x + 1, p.y);
    return make_float4(t.x, t.y, r.x, r.y);
}
"""

# This repository's flow-only integrator (tendrils_amd/csrc/th_logic.hpp: logic_texel_ref without its noise and target terms):
# flow tap, decay, force, damping, speed clamp, Euler step.  The uniform block is th_logic_uniforms.
FLOW_ONLY = """struct Logic {
    float viewSize[2];
    float time, dt, speedLimit, damping, forceWeight, flowWeight, noiseWeight, flowDecay, noiseSpeed, noiseScale, target;
    float varyForce, varyFlow, varyNoise, varyNoiseScale, varyNoiseSpeed, varyTarget;
};
__device__ float vary(float base, float offset, float variance) { return base + (offset * variance * base); }
__device__ float4 th_main(const th_pass &p)
{
    const Logic &u = th_uniforms<Logic>(p);
    const float4 st = p.self;
    if (!(st.x != -1000000.0f || st.y != -1000000.0f)) return st;
    const float fcx = (float)p.x + 0.5f, fcy = (float)p.y + 0.5f;
    const float i = (fcx + (fcy * p.dataRes.x)) / (p.dataRes.x * p.dataRes.y);
    const float sx = st.x * u.viewSize[0], sy = st.y * u.viewSize[1];
    const float4 ft = th_flow(p, 0.0f + (1.0f * (sx + 1.0f)) / 2.0f, 0.0f + (1.0f * (sy + 1.0f)) / 2.0f);
    const float k = fmaxf(0.0f, 1.0f - ((u.time - ft.z) * u.flowDecay));
    const float ffx = (0.0f + ft.x * k * 1.0f) / 1.0f, ffy = (0.0f + ft.y * k * 1.0f) / 1.0f;
    const float force = vary(u.forceWeight, i, u.varyForce), flow = vary(u.flowWeight, i, u.varyFlow);
    float vx = (st.z * u.damping * u.dt) + (force * (ffx * u.dt * flow));
    float vy = (st.w * u.damping * u.dt) + (force * (ffy * u.dt * flow));
    const float speed = sqrtf(vx * vx + vy * vy);
    const float r = fminf(speed, u.speedLimit) / speed;
    vx *= r; vy *= r;
    return make_float4(st.x + vx, st.y + vy, vx, vy);
}
"""


@pytest.fixture(scope="module")
def programs():
    progs = dict(
        drift=Program.from_source(DRIFT, DriftU, name="drift"),
        coords=Program.from_source(COORDS, name="coords"),
        index=Program.from_source(INDEX, name="index"),
        data=Program.from_source(DATA, name="data"),
        data_res=Program.from_source(DATA_RES, name="data_res"),
        row_above=Program.from_source(ROW_ABOVE, name="row_above"),
        targets=Program.from_source(TARGETS, name="targets"),
        flow_only=Program.from_source(FLOW_ONLY, _capi.LogicUniforms, name="flow_only"),
    )
    yield progs
    for p in progs.values():
        p.dispose()


def context(w=W, h=H, buffers=2, row0=0, global_height=0, packed=False):
    p = Particles(None, dict(shape=[w, h], row0=row0, globalHeight=global_height,
                             stateFormat=_capi.TH_STATE_F16 if packed else _capi.TH_STATE_F32))
    p.setup(buffers)
    return p


def state(w=W, h=H, seed=1):
    """positions in [-1, 1), velocities of +-0.01, a few inert texels"""
    n = max(w, h)
    return np.ascontiguousarray(hashed_state(n, seed, inert_mod=17)[:h, :w])


def drift_ref(st, k):
    out = st.copy()
    out[..., 0] = st[..., 0] + st[..., 2] * F(k)          # float32 multiply, float32 add: what -ffp-contract=off leaves
    out[..., 1] = st[..., 1] + st[..., 3] * F(k)
    return out


def device_ptrs(p):
    out = []
    for k in range(len(p.buffers)):
        d = C.c_void_p()
        call("th_state_device_ptr", p._ctx, k, C.byref(d))
        out.append(d.value)
    return out


def logic_dict(meta):
    u = dict(meta["state"])
    u.update(viewSize=meta["viewSize"], time=meta["times"][0], dt=meta["dts"][0])
    return u


def nearest(u, n):
    """NEAREST + CLAMP_TO_EDGE in fp32: clamp(floor(u * n), 0, n - 1)"""
    return np.clip(np.floor(u.astype(F) * F(n)), 0, n - 1).astype(np.int64)


# ---- the drift program: ring semantics ------------------------------------------------------------------------------------
def test_drift_rotates_the_ring_as_a_step_does(programs):
    a, b = state(seed=1), state(seed=2)
    p, twin = context(), context()
    for c in (p, twin):
        c.upload_texels(a, 0)
        c.upload_texels(b, 1)
    before, twin_before = device_ptrs(p), device_ptrs(twin)
    run_pass(p, programs["drift"], dict(k=0.75), _capi.TH_TARGET_RING)
    s = _capi.LogicUniforms()
    call("th_step", twin._ctx, C.byref(s), _capi.TH_TARGET_RING)
    after, twin_after = device_ptrs(p), device_ptrs(twin)
    # utils.step: the last buffer comes first, and the pass writes it from what was buffers[0]
    assert [after.index(d) for d in before] == [twin_after.index(d) for d in twin_before] == [1, 0]
    assert bits_equal(p.read(0), drift_ref(a, 0.75)).all()
    assert bits_equal(p.read(1), a).all()
    p.dispose(), twin.dispose()


def test_drift_into_a_ring_index_and_into_targets(programs):
    a, b = state(seed=3), state(seed=4)
    p = context()
    p.upload_texels(a, 0)
    p.upload_texels(b, 1)
    before = device_ptrs(p)
    run_pass(p, programs["drift"], dict(k=-2.5), 0)                       # buffers[0] from buffers[1], no rotation
    assert device_ptrs(p) == before
    assert bits_equal(p.read(0), drift_ref(b, -2.5)).all() and bits_equal(p.read(1), b).all()
    run_pass(p, programs["drift"], dict(k=3.0), _capi.TH_TARGET_TARGETS)
    got = np.empty((H, W, 4), F)
    call("th_targets_download", p._ctx, got.ctypes.data_as(_capi._fp))
    assert device_ptrs(p) == before
    assert bits_equal(got, drift_ref(b, 3.0)).all()
    assert bits_equal(p.read(0), drift_ref(b, -2.5)).all() and bits_equal(p.read(1), b).all()
    # the pass leaves the respawned counter alone
    assert p.stats(0.01)["respawned"] == 0
    p.dispose()


# ---- coordinates: whole texture and row bands -------------------------------------------------------------------------------
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


def test_coordinates_whole_and_in_row_bands(programs):
    want_coords, want_index = coords_ref()
    p = context()
    run_pass(p, programs["coords"], {}, _capi.TH_TARGET_RING)
    assert bits_equal(p.read(0), want_coords).all()
    run_pass(p, programs["index"], {}, _capi.TH_TARGET_RING)
    assert bits_equal(p.read(0), want_index).all()
    p.dispose()
    # two plain contexts holding the bands, no communicator: each sees the coordinates of the unsharded run
    for name, want in (("coords", want_coords), ("index", want_index)):
        parts = []
        for row0, rows in BANDS:
            band = context(h=rows, row0=row0, global_height=H)
            run_pass(band, programs[name], {}, _capi.TH_TARGET_RING)
            parts.append(band.read(0))
            band.dispose()
        assert bits_equal(np.concatenate(parts), want).all(), name


# ---- spawnData ------------------------------------------------------------------------------------------------------------
def uv_state():
    """uv values in the texels' xy: on the edges, beyond them, and everywhere between"""
    st = state(seed=5)
    st[..., :2] = st[..., :2] * F(0.75) + F(0.5)                        # [-0.25, 1.25)
    edge = np.array([0.0, 1.0, -0.0, 1.25, -0.25, 0.5, 2.0, -1.0, 1.0 - 2.0 ** -24, 2.0 ** -30], F)
    st[0, :edge.size, 0] = edge
    st[0, :edge.size, 1] = edge[::-1]
    st[1, :edge.size, 0] = edge
    st[1, :edge.size, 1] = edge
    return st


def data_ref(st, data):
    dh, dw = data.shape[:2]
    return data[nearest(F(1.0) - st[..., 1], dh), nearest(F(1.0) - st[..., 0], dw)]


def test_spawn_data_from_the_image_the_flow_and_the_ring(programs):
    st = uv_state()
    rng = np.random.default_rng(11)
    image = rng.standard_normal((23, 37, 4)).astype(F)
    flow = rng.standard_normal((61, 97, 4)).astype(F)
    other = state(seed=6)
    p = context(buffers=3)
    p.upload_texels(st, -1)
    p.upload_texels(other, 2)
    call("th_spawn_image_upload", p._ctx, image.ctypes.data_as(_capi._fp), 37, 23)
    call("th_flow_resize", p._ctx, 97, 61)
    call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
    for source, data in ((_capi.TH_SOURCE_IMAGE, image), (_capi.TH_SOURCE_FLOW, flow), (2, other)):
        run_pass(p, programs["data"], dict(spawnData=source), 0)
        assert bits_equal(p.read(0), data_ref(st, data)).all(), source
        run_pass(p, programs["data_res"], dict(spawnData=source), 0)
        assert (p.read(0) == np.array([data.shape[1], data.shape[0], 97, 61], F)).all(), source
    # through the ring: the host names the buffer as it stands BEFORE the rotation, the pass sees it one place on
    texture = state(seed=7)
    p.upload_texels(st, 0)                                              # `particles` of the pass: buffers[1] once rotated
    p.upload_texels(texture, 1)
    chosen = p.buffers[1]                                               # spawnData; after the rotation it is buffers[2]
    p.upload_texels(other, 2)                                           # rotates to buffers[0]: the render target
    p.logic = programs["data"]
    p.step(dict(spawnData=chosen))
    assert chosen.index == 2
    assert bits_equal(p.read(0), data_ref(st, texture)).all()
    assert bits_equal(p.read(1), st).all() and bits_equal(p.read(2), texture).all()
    # no spawnData at all reads as zeros
    run_pass(p, programs["data"], {}, 0)
    assert not p.read(0).any()
    p.dispose()


def test_targets_and_neighbours_through_the_accessors(programs):
    st, tg = state(seed=8), state(seed=9)
    p = context()
    p.upload_texels(st, -1)
    call("th_targets_upload", p._ctx, tg.ctypes.data_as(_capi._fp))
    run_pass(p, programs["targets"], {}, _capi.TH_TARGET_RING)
    right = st[:, np.minimum(np.arange(W) + 1, W - 1)]                   # the last column reads itself: clamped
    want = np.concatenate([tg[..., :2], right[..., :2]], -1)
    assert bits_equal(p.read(0), want).all()
    p.dispose()


# ---- the seam is real: this repository's flow-only integrator as a user program ------------------------------------------------
def test_flow_only_integrator_as_a_user_program_equals_th_step(programs):
    fx = load(os.path.join(GOLDEN, "logic_flow_only_64.npz"))
    meta = fx["meta"]
    uniforms = logic_dict(meta)
    assert uniforms["noiseWeight"] == 0
    n = meta["N"]
    results = []
    for program in (programs["flow_only"], Program(LOGIC)):
        p = context(n, n)
        p.upload_texels(fx["state"], -1)
        call("th_flow_resize", p._ctx, *meta["flowShape"])
        call("th_flow_upload", p._ctx, np.ascontiguousarray(fx["flow"], F).ctypes.data_as(_capi._fp))
        run_pass(p, program, dict(uniforms), _capi.TH_TARGET_RING)
        results.append(p.read(0))
        p.dispose()
    got, want = results
    mask = fx["valid"][0]
    assert mask.sum() > n * n // 2
    # as VALUES: NaN where NaN, and a zero's sign is free (the built-in adds its zero-weighted noise and target terms)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same[mask].all(), int((~same[mask]).sum())
    moved = (got[..., :2] != fx["state"][..., :2]).any(-1)
    assert moved[mask].sum() > n * n // 4                                 # (the pass did integrate)


# ---- packed ring ------------------------------------------------------------------------------------------------------------
def test_drift_over_a_packed_ring(programs):
    w, h = 64, 16
    st = state(w, h, seed=10)
    a, b = context(w, h, packed=True), context(w, h, packed=True)
    a.upload_texels(st, -1)
    quantised = a.read(1)                                                # what the pass reads: the stored state, decoded
    run_pass(a, programs["drift"], dict(k=0.5), _capi.TH_TARGET_RING)
    b.upload_texels(drift_ref(quantised, 0.5), 0)
    assert (quantised != st).any()
    assert bits_equal(a.read(0), b.read(0)).all()
    assert bits_equal(a.read(1), quantised).all()
    a.dispose(), b.dispose()


# ---- tile-sorted slots ------------------------------------------------------------------------------------------------------
def test_program_between_steps_over_tile_sorted_slots(programs):
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
        sorted_buffers = []
        for k in range(4):
            if k == 2:
                info = _capi.SlotOrderInfo()
                call("th_slot_order", t.particles._ctx, C.byref(info))
                sorted_buffers.append(info.sorted_buffers)
                t.spawnShader(programs["drift"], dict(k=0.25))
            else:
                t.timer.tick()
                t.step()
        t.draw()
        out.append((sorted_buffers[0], t.particles.read(0), t.particles.read(1), t.flow.read(), t.read_view()))
        t.dispose()
    (was_sorted, *sorted_run), (never_sorted, *plain_run) = out
    assert was_sorted > 0 and never_sorted == 0
    for a, b in zip(sorted_run[:3], plain_run[:3]):
        assert bits_equal(a, b).all()
    assert (sorted_run[3] == plain_run[3]).all() and sorted_run[3].any()


# ---- errors, life cycle, query ------------------------------------------------------------------------------------------------
def test_a_uniform_block_of_1025_bytes_fails(programs):
    p = context()
    block = (C.c_uint8 * 1025)()
    with pytest.raises(ta.TendrilsHipError) as e:
        call("th_program_run", p._ctx, programs["drift"].handle, block, 1025, _capi.TH_SOURCE_NONE, 0)
    assert e.value.status == _capi.TH_ERR_INVALID and "1025" in str(e.value)
    call("th_program_run", p._ctx, programs["drift"].handle, block, 1024, _capi.TH_SOURCE_NONE, 0)
    with pytest.raises(ta.TendrilsHipError):
        call("th_program_run", p._ctx, programs["drift"].handle, None, 0, 99, 0)          # no such spawnData
    p.dispose()


def test_reading_particles_outside_a_band_is_unsupported_and_the_next_run_works(programs):
    st = state(seed=14)
    row0, rows = BANDS[1]
    band = context(h=rows, row0=row0, global_height=H)
    band.upload_texels(st[row0:], -1)
    with pytest.raises(ta.TendrilsHipError) as e:
        run_pass(band, programs["row_above"], {}, 0)
    assert e.value.status == _capi.TH_ERR_UNSUPPORTED and "row %d " % (row0 - 1) in str(e.value)
    run_pass(band, programs["drift"], dict(k=1.5), 0)
    assert bits_equal(band.read(0), drift_ref(st[row0:], 1.5)).all()
    band.dispose()
    # the first band holds row 0: there the row above clamps to the row itself and nothing leaves the band
    row0, rows = BANDS[0]
    band = context(h=rows, row0=row0, global_height=H)
    band.upload_texels(st[:rows], -1)
    run_pass(band, programs["row_above"], {}, 0)
    assert bits_equal(band.read(0), np.concatenate([st[:1], st[:rows - 1]])).all()
    band.dispose()


def test_a_destroyed_program_keeps_running_where_it_was_loaded():
    st = state(seed=15)
    prog = Program.from_source(DRIFT, DriftU, name="drift_once")
    p, q = context(), context()
    for c in (p, q):
        c.upload_texels(st, -1)
        run_pass(c, prog, dict(k=2.0), 0)                                  # two contexts share one program
        assert bits_equal(c.read(0), drift_ref(st, 2.0)).all()
    handle = C.c_void_p(prog.handle.value)
    prog.dispose()                                                          # th_program_destroy
    block = DriftU(k=-1.0)
    for c in (p, q):
        call("th_program_run", c._ctx, handle, C.byref(block), C.sizeof(block), _capi.TH_SOURCE_NONE, 0)
        assert bits_equal(c.read(0), drift_ref(st, -1.0)).all()
    p.dispose(), q.dispose()


def test_query_reports_no_scratch_for_the_drift_program(programs):
    p = context()
    info = programs["drift"].query(p)
    assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0
    assert 0 < info["vgprs"] <= 512 and 0 < info["sgprs"] <= 128 and 0 < info["code_bytes"] < 4096
    p.dispose()


# ---- the library a product host ships -----------------------------------------------------------------------------------------
RELEASE = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
CHILD = r'''
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tendrils_amd import _capi
from tendrils_amd.particles import Particles, Program, run_pass
from helpers import bits_equal, hashed_state
lib = _capi.load()
assert os.path.realpath(lib._name) == os.path.realpath(RELEASE), lib._name
assert not hasattr(lib, "th_comm_loopback_id")
class DriftU(C.Structure):
    _fields_ = [("k", C.c_float)]
prog = Program.from_source(SOURCE, DriftU, name="drift")
st = np.ascontiguousarray(hashed_state(50, 21, inert_mod=17)[:30])
p = Particles(None, dict(shape=[50, 30]))
p.setup(2)
p.upload_texels(st, -1)
run_pass(p, prog, dict(k=0.75), _capi.TH_TARGET_RING)
want = st.copy()
want[..., 0] = st[..., 0] + st[..., 2] * np.float32(0.75)
want[..., 1] = st[..., 1] + st[..., 3] * np.float32(0.75)
assert bits_equal(p.read(0), want).all()
assert prog.query(p)["scratch_bytes"] == 0
p.dispose(); prog.dispose()
print("release ok")
'''


def test_release_library_runs_a_user_program():
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", os.path.join(ROOT, "tendrils_amd", "csrc"), "release"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, TH_LIB=RELEASE)
    code = "ROOT = %r\nRELEASE = %r\nSOURCE = %r\n" % (ROOT, RELEASE, DRIFT) + CHILD
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "release ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
