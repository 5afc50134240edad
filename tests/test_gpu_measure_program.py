"""Measure programs on the GPU (include/tendrils_hip.h "measure programs"; tendrils_amd/csrc/th_measure.hip,
th_measure_prelude.inc): a caller's per-particle sample function under the library's reduction.  The reference is numpy over the
state in TEXEL order - what was uploaded, or Particles.read() - never the code under test.

Shapes: 5 x 3 (one partial wave: 15 of 64 lanes hold a particle), 48 x 48 (nine whole workgroups), 100 x 37 (a ragged last
workgroup: 3700 = 14 x 256 + 116) and 1024 x 600 (614 400 texels over the grid's 2048 x 256 lanes: lanes take a second slot).

Exact channels - counts and integers - have exact partial sums in double whatever the order, so they are compared bit for bit
with numpy's integer sums.  A general channel's sum is compared under |sum - numpy float64 sum| <= n 2^-53 sum|v|: the bound of
ANY order of n float64 additions of exactly converted values (each addition rounds by at most 2^-53 of a partial sum, which is at
most sum|v|)."""
import ctypes as C

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import MeasureProgram, Particles
from tendrils_amd.tendrils import View

from helpers import bits_equal, hashed_state, pack_state, unpack_state

pytestmark = pytest.mark.gpu

F = np.float32
INERT = F(-1e6)
SHAPES = [(5, 3), (48, 48), (100, 37), (1024, 600)]
RECT = (-0.5, -0.25, 0.75, 0.5)          # x0, y0, x1, y1: exact in fp32


class Rect(C.Structure):
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


class Which(C.Structure):
    _fields_ = [("which", C.c_uint32)]


EXACT = """struct Rect { float x0, y0, x1, y1; };
__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    const Rect &r = th_uniforms<Rect>(m);
    const bool live = m.self.x != -1000000.0f || m.self.y != -1000000.0f;
    const bool inside = live && m.self.x >= r.x0 && m.self.x < r.x1 && m.self.y >= r.y0 && m.self.y < r.y1;
    th_sample s = th_sample_zero();
    s.v[0] = live ? 1.0f : 0.0f;
    s.v[1] = (float)(m.index % 7u);
    s.v[2] = inside ? rintf(m.self.x * 16384.0f) : 0.0f;
    return s;
}
"""
GENERAL = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = m.self.z * m.self.z + m.self.w * m.self.w;
    return s;
}
"""
LIVE_ONLY = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    if (m.self.x == -1000000.0f && m.self.y == -1000000.0f) return th_no_sample();
    th_sample s = th_sample_zero();
    s.v[0] = 1.0f;
    s.v[1] = m.self.z;
    return s;
}
"""
NOBODY = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    return th_no_sample();
}
"""
ONE_NAN = """struct Which { unsigned which; };
__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = m.index == th_uniforms<Which>(m).which ? __builtin_nanf("") : m.self.z;
    s.v[1] = m.self.w;
    return s;
}
"""
# particles selected by their STATE report their texel's coordinates: over sorted slots a slot's `self` must meet its own texel
SELECTED = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    const bool live = m.self.x != -1000000.0f || m.self.y != -1000000.0f;
    if (!(live && m.self.x > 0.0f)) return th_no_sample();
    th_sample s = th_sample_zero();
    s.v[0] = (float)m.index;
    s.v[1] = (float)m.x;
    s.v[2] = (float)m.y;
    s.v[3] = (float)(m.index % 7u);
    return s;
}
"""
WHERE = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = (float)m.y;
    s.v[1] = (float)(m.index % 7u);
    s.v[2] = m.dataRes.y;
    s.v[3] = (float)m.x;
    return s;
}
"""
TAP = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    const float2 r = th_flow_res(m);
    s.v[0] = th_flow(m, m.uv.x, m.uv.y).w;
    s.v[1] = r.x * 1024.0f + r.y;
    return s;
}
"""
OTHER_KINDS = dict(
    state=("th_program_compile", "__device__ float4 th_main(const th_pass &p) { return p.self; }\n"),
    screen=("th_screen_program_compile", "__device__ float4 th_screen(const th_screen_pass &s) { return make_float4(s.uv.x, s.uv.y, 0.5f, 1.0f); }\n"),
    draw=("th_draw_program_compile", "__device__ th_vertex th_vertex_main(const th_vertex_pass &v)\n{\n    th_vertex o;\n"
          "    o.position = make_float2(v.state.x, v.state.y);\n    o.color = v.state;\n    return o;\n}\n"),
    step=("th_step_program_compile", "__device__ float4 th_step_main(const th_step_pass &s) { return s.self; }\n"),
    fragment=("th_fragment_program_compile", "__device__ float4 th_fragment_main(const th_fragment_pass &f) { return f.color; }\n"))
KIND_NAMES = dict(state="state program (th_program_compile)", screen="screen program (th_screen_program_compile)",
                  draw="draw program (th_draw_program_compile)", step="step program (th_step_program_compile)",
                  fragment="fragment program (th_fragment_program_compile)", measure="measure program (th_measure_program_compile)")


@pytest.fixture(scope="module")
def programs():
    progs = dict(exact=MeasureProgram.from_source(EXACT, Rect, channels=3, name="exact"),
                 general=MeasureProgram.from_source(GENERAL, channels=1, name="general"),
                 live_only=MeasureProgram.from_source(LIVE_ONLY, channels=2, name="live_only"),
                 nobody=MeasureProgram.from_source(NOBODY, channels=8, name="nobody"),
                 one_nan=MeasureProgram.from_source(ONE_NAN, Which, channels=2, name="one_nan"),
                 selected=MeasureProgram.from_source(SELECTED, channels=4, name="selected"),
                 where=MeasureProgram.from_source(WHERE, channels=4, name="where"),
                 tap=MeasureProgram.from_source(TAP, channels=2, name="tap"))
    yield progs
    for p in progs.values():
        p.dispose()


@pytest.fixture(scope="module")
def states():
    """the hashed state of every shape (positions in [-1, 1), velocities in [-0.01, 0.01), one texel in seven inert): computed
    once, read-only"""
    out = {}
    for w, h in SHAPES:
        st = np.ascontiguousarray(hashed_state(w, 17 + w, inert_mod=7, rows=(0, h)))
        assert st.shape == (h, w, 4)
        st.setflags(write=False)
        out[(w, h)] = st
    return out


def context(shape, st=None, packed=False, buffers=2, row0=0, global_height=0, flow=(8, 6)):
    w, h = shape
    p = Particles(None, dict(shape=[w, h], row0=row0, globalHeight=global_height,
                             stateFormat=_capi.TH_STATE_F16 if packed else _capi.TH_STATE_F32))
    p.setup(buffers)
    field = np.zeros((flow[1], flow[0], 4), F)
    field[..., 3] = (np.arange(flow[0] * flow[1], dtype=F) % 5).reshape(flow[1], flow[0])
    call("th_flow_resize", p._ctx, *flow)
    call("th_flow_upload", p._ctx, field.ctypes.data_as(_capi._fp))
    if st is not None:
        p.upload_texels(st, 0)
    return p


def live_of(st):
    return (st[..., 0] != INERT) | (st[..., 1] != INERT)


def index_of(st, row0=0):
    h, w = st.shape[:2]
    return (np.arange(h, dtype=np.int64)[:, None] + row0) * w + np.arange(w, dtype=np.int64)[None, :]


def exact_channels(st, row0=0):
    """the EXACT program's three channels per particle, in numpy fp32 (every value an integer)"""
    x, y = st[..., 0], st[..., 1]
    live = live_of(st)
    with np.errstate(invalid="ignore"):
        inside = live & (x >= F(RECT[0])) & (x < F(RECT[2])) & (y >= F(RECT[1])) & (y < F(RECT[3]))
        snapped = np.rint(x * F(16384.0))
    return np.stack([live.astype(F), (index_of(st, row0) % 7).astype(F), np.where(inside, snapped, F(0)).astype(F)], -1)


def same_exact(got, values, taken=None):
    """`got` against the per-particle integer `values` [..., channels] of the samples taken: sums equal to numpy's INTEGER
    sums, min and max equal as values"""
    v = values.reshape(-1, values.shape[-1])
    assert got.taken == (len(v) if taken is None else taken)
    for c in range(v.shape[1]):
        assert np.all(v[:, c] == np.rint(v[:, c]))
        want = int(v[:, c].astype(np.int64).sum())
        assert abs(want) < 2 ** 53 and got.sum[c] == float(want), (c, got.sum[c], want)
        if len(v):
            assert got.min[c] == v[:, c].min() and got.max[c] == v[:, c].max(), (c, got.min[c], got.max[c])


def general_values(st):
    z, w = st[..., 2].astype(F), st[..., 3].astype(F)
    return (z * z + w * w).astype(F).reshape(-1)


def within_bound(total, v):
    """|total - numpy's float64 sum| <= n 2^-53 sum|v| (see the module's docstring); returns the two sides for the message"""
    v64 = v.astype(np.float64)
    err, bound = abs(total - v64.sum()), len(v64) * 2.0 ** -53 * np.abs(v64).sum()
    print("general sum: error %.3e, bound %.3e, n = %d" % (err, bound, len(v64)))
    return err <= bound


def slot_order_read(p, buffer=0, packed=False):
    """(sorted, perm, the raw slots) of a ring buffer, as th_slot_order_read hands them out - the ring stays where it lies"""
    n = p.shape[0] * p.shape[1]
    perm = np.zeros(n, np.uint32)
    slots = np.zeros((n, 2 if packed else 4), np.uint32)      # 8 bytes a slot of a packed ring, 16 of an f32 one
    is_sorted, nchunks = C.c_int32(0), C.c_uint32(0)
    call("th_slot_order_read", p._ctx, int(buffer), perm.ctypes.data_as(C.POINTER(C.c_uint32)), None, 0, C.byref(nchunks),
         slots.ctypes.data_as(C.c_void_p), C.byref(is_sorted))
    return bool(is_sorted.value), perm, slots


def sorted_buffers(p):
    info = _capi.SlotOrderInfo()
    call("th_slot_order", p._ctx, C.byref(info))
    return int(info.sorted_buffers)


# ---- 1, 2: exact and general channels in texel order ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_exact_channels_equal_numpys_integer_sums(programs, states, shape):
    st = states[shape]
    p = context(shape, st)
    got = p.measure(programs["exact"], dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3]))
    values = exact_channels(st)
    assert values[..., 0].sum() < st.shape[0] * st.shape[1] and (values[..., 2] != 0).any()      # some inert, some inside
    assert got.particles == shape[0] * shape[1]
    same_exact(got, values)
    assert bits_equal(p.read(0), st).all()                    # (the reference is the ring's own content, and the measure left it)
    p.dispose()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_general_sum_is_within_the_bound_of_any_order_and_reproducible(programs, states, shape):
    st = states[shape]
    p = context(shape, st)
    a = p.measure(programs["general"])
    b = p.measure(programs["general"])
    v = general_values(st)
    assert a.taken == v.size and a.particles == v.size
    assert within_bound(a.sum[0], v)
    assert a.min[0] == v.min() and a.max[0] == v.max()
    assert a.raw == b.raw                                     # the same ring, the same order: the same bits
    p.dispose()


# ---- 3: th_no_sample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3), (100, 37)], ids=lambda s: "%dx%d" % s)
def test_no_sample_contributes_nothing(programs, states, shape):
    st = states[shape]
    p = context(shape, st)
    live = live_of(st)
    got = p.measure(programs["live_only"])
    assert got.taken == p.stats(0.01)["live"] == int(live.sum()) < live.size
    assert got.sum[0] == float(live.sum()) and got.min[0] == got.max[0] == 1.0
    z = st[..., 2][live]
    assert within_bound(got.sum[1], z) and got.min[1] == z.min() and got.max[1] == z.max()
    none = p.measure(programs["nobody"])
    assert none.taken == 0 and none.particles == live.size
    assert (none.sum == 0.0).all() and (none.min == np.inf).all() and (none.max == -np.inf).all()
    assert len(none.sum) == 8
    # channels at and beyond the program's own hold the identities as well
    raw = _capi.MeasureResult.from_buffer_copy(got.raw)
    assert list(raw.sum[2:]) == [0.0] * 6 and list(raw.min[2:]) == [np.inf] * 6 and list(raw.max[2:]) == [-np.inf] * 6
    p.dispose()


# ---- 4: a NaN sample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,which", [((5, 3), 14), ((100, 37), 3699), ((100, 37), 64), ((1024, 600), 600000)])
def test_one_nan_sample_poisons_its_sum_alone(programs, states, shape, which):
    st = states[shape]
    p = context(shape, st)
    got = p.measure(programs["one_nan"], dict(which=which))
    z, w = st[..., 2].reshape(-1), st[..., 3].reshape(-1)
    others = np.delete(z, which)
    assert got.taken == z.size
    assert np.isnan(got.sum[0])
    assert got.min[0] == others.min() and got.max[0] == others.max()
    assert within_bound(got.sum[1], w) and got.min[1] == w.min() and got.max[1] == w.max()
    clean = p.measure(programs["one_nan"], dict(which=0xffffffff))
    assert within_bound(clean.sum[0], z) and clean.min[0] == z.min() and clean.max[0] == z.max()
    p.dispose()


# ---- 5, 6: tile-sorted slots, f32 and packed -----------------------------------------------------------------------------------
def tendrils(shape, view, st, fmt="f32"):
    w, h = shape
    opts = ta.defaults()
    opts.update(rows=h, globalHeight=h, stateFormat=_capi.TH_STATE_F16 if fmt == "f16" else _capi.TH_STATE_F32)
    t = ta.Tendrils(View(*view), opts)
    t.resize()
    t.setup(w)
    assert t.particles.shape == [w, h]
    t.particles.option("bucket", 1)
    t.particles.draw_pipeline("bins")
    t.particles.upload_texels(st)
    rng = np.random.default_rng(3)
    flow = np.zeros((view[1], view[0], 4), F)
    flow[..., :2] = rng.uniform(-0.01, 0.01, (view[1], view[0], 2))
    flow[..., 2] = 2990.0
    flow[..., 3] = 1.0
    t.flow.set_pixels(flow)
    t.timer.time = 3000.0
    t.renderView = True
    return t


def step_until_sorted(t):
    for _ in range(4):
        t.step_n(3)
        if sorted_buffers(t.particles) > 0:
            return
    raise AssertionError("step_n left no buffer in sorted slots")


SORTED_SHAPES = [((48, 48), (32, 24)), ((100, 37), (40, 30))]      # (sorted slots need twice as many particles as flow texels)


def selected_channels(st):
    live = live_of(st)
    with np.errstate(invalid="ignore"):
        sel = live & (st[..., 0] > 0)
    idx = index_of(st)
    w = st.shape[1]
    return np.stack([idx, idx % w, idx // w, idx % 7], -1).astype(F)[sel], int(sel.sum())


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_tile_sorted_slots_measure_like_texel_order_and_stay_sorted(programs, states, shape, view, fmt):
    t = tendrils(shape, view, states[shape], fmt)
    p = t.particles
    step_until_sorted(t)
    rect = dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3])
    is_sorted, perm_before, slots_before = slot_order_read(p, 0, fmt == "f16")
    assert is_sorted and not (perm_before == np.arange(perm_before.size)).all()
    got = {b: (p.measure(programs["exact"], rect, buffer=b), p.measure(programs["selected"], buffer=b),
               p.measure(programs["general"], buffer=b), p.measure(programs["general"], buffer=b)) for b in (0, 1)}
    again, perm_after, slots_after = slot_order_read(p, 0, fmt == "f16")
    assert again and (perm_after == perm_before).all() and (slots_after == slots_before).all()
    assert sorted_buffers(p) > 0
    if fmt == "f16":
        # the packed texels themselves, put back into texel order by the table, decoded by the numpy mirror of the codec
        texels = np.zeros_like(slots_before)
        texels[perm_before] = slots_before
        decoded = unpack_state(texels).reshape(shape[1], shape[0], 4)
    for b in (0, 1):
        st = p.read(b)                                        # (texel order: from here on the ring is no longer sorted)
        if fmt == "f16" and b == 0:
            assert bits_equal(st, decoded).all()
        exact, selected, general, general2 = got[b]
        same_exact(exact, exact_channels(st))
        values, count = selected_channels(st)
        assert 0 < count < st.shape[0] * st.shape[1]
        same_exact(selected, values, taken=count)
        v = general_values(st)
        assert within_bound(general.sum[0], v) and general.min[0] == v.min() and general.max[0] == v.max()
        assert general.raw == general2.raw
    t.dispose()


@pytest.mark.parametrize("shape", [(5, 3), (100, 37), (1024, 600)], ids=lambda s: "%dx%d" % s)
def test_packed_ring_in_texel_order(programs, states, shape):
    st = states[shape]
    p = context(shape, st, packed=True)
    decoded = unpack_state(pack_state(st))                    # what the 8-byte texels hold, by the numpy mirror of the codec
    assert bits_equal(p.read(0), decoded).all() and not bits_equal(decoded, st).all()
    got = p.measure(programs["exact"], dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3]))
    same_exact(got, exact_channels(decoded))
    assert got.particles == shape[0] * shape[1]
    general = p.measure(programs["general"])
    v = general_values(decoded)
    assert within_bound(general.sum[0], v) and general.min[0] == v.min() and general.max[0] == v.max()
    assert general.raw == p.measure(programs["general"]).raw
    p.dispose()


@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_step_measure_draw_leaves_the_bits_of_step_draw(programs, states, shape, view):
    a, b = tendrils(shape, view, states[shape]), tendrils(shape, view, states[shape])
    rect = dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3])
    for frame in range(3):
        for t in (a, b):
            t.timer.tick()
            t.step()
        a.measure(programs["exact"], rect)
        a.particles.measure(programs["general"], buffer=1)
        for t in (a, b):
            t.draw()
        qa, qb = _capi.DrawInfo(), _capi.DrawInfo()
        call("th_draw_query", a.particles._ctx, C.byref(qa))
        call("th_draw_query", b.particles._ctx, C.byref(qb))
        assert (qa.pipeline, qa.fragments, qa.crowded_fragments) == (qb.pipeline, qb.fragments, qb.crowded_fragments)
        assert a.fragments == b.fragments > 0
        assert sorted_buffers(a.particles) == sorted_buffers(b.particles)
    assert sorted_buffers(a.particles) > 0
    assert a.particles.stats(0.01) == b.particles.stats(0.01)          # (the respawned counter among them)
    assert bits_equal(a.flow.read(), b.flow.read()).all()
    assert (a.read_view() == b.read_view()).all() and a.read_view().any()
    for k in (0, 1):
        assert bits_equal(a.particles.read(k), b.particles.read(k)).all()
    a.dispose(); b.dispose()


# ---- 7: a row band --------------------------------------------------------------------------------------------------------------
def test_a_row_band_sees_the_whole_textures_coordinates(programs):
    from test_gpu_loopback import inputs, make
    n, view, band = 64, (40, 24), (16, 32)
    cur, prev, base = inputs(n, view, 23)
    t = make(n, view, cur, prev, base, band=band)
    p = t.particles
    assert p.shape == [n, band[1]] and p._row0 == band[0] and p._global_height == n
    got = p.measure(programs["where"])
    rows = np.arange(band[0], band[0] + band[1])
    y = np.repeat(rows, n)
    idx = (rows[:, None] * n + np.arange(n)[None, :]).reshape(-1)
    values = np.stack([y, idx % 7, np.full(y.size, n), idx % n], -1).astype(F)
    assert got.particles == n * band[1]
    same_exact(got, values)
    assert (got.min[0], got.max[0]) == (band[0], band[0] + band[1] - 1)
    exact = p.measure(programs["exact"], dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3]))
    same_exact(exact, exact_channels(cur[band[0]:band[0] + band[1]], row0=band[0]))
    # everywhere=True without a communicator is the local measure
    assert p.measure(programs["where"], everywhere=True).raw == got.raw
    t.dispose()


def test_flow_taps_are_the_clamped_nearest_texels(programs, states):
    shape, flow = (100, 37), (8, 6)
    p = context(shape, states[shape], flow=flow)
    got = p.measure(programs["tap"])
    h, w = shape[1], shape[0]
    u = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    v = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    fx = np.clip(np.floor(u * F(flow[0])), 0, flow[0] - 1).astype(np.int64)
    fy = np.clip(np.floor(v * F(flow[1])), 0, flow[1] - 1).astype(np.int64)
    field = (np.arange(flow[0] * flow[1]) % 5).reshape(flow[1], flow[0])
    taps = field[fy[:, None], fx[None, :]].astype(F)
    same_exact(got, np.stack([taps, np.full(taps.shape, flow[0] * 1024 + flow[1], F)], -1))
    p.dispose()


# ---- 8: errors and plumbing -----------------------------------------------------------------------------------------------------
def refused(name, args):
    lib = _capi.load()
    status = getattr(lib, name)(*args)
    assert status == _capi.TH_ERR_INVALID, (name, status)
    return lib.th_last_error().decode()


def test_every_wrong_kind_is_refused_in_both_directions_by_name(programs, states):
    lib = _capi.load()
    p = context((48, 48), states[(48, 48)])
    ctx, measure = p._ctx, programs["exact"]
    out, n, dev = _capi.MeasureResult(), C.c_uint64(0), C.c_void_p()
    others = {}
    for kind, (entry, source) in OTHER_KINDS.items():
        handle = C.c_void_p()
        assert getattr(lib, entry)(source.encode(), kind.encode(), C.byref(handle)) == _capi.TH_OK, lib.th_program_log()
        others[kind] = handle
    for kind, handle in others.items():
        for entry, last in (("th_measure_run", C.byref(out)), ("th_measure_async", C.byref(dev)), ("th_measure_global", C.byref(out))):
            text = refused(entry, (ctx, handle, None, 0, 0, last))
            assert text == "%s runs a %s: '%s' is a %s" % (entry, KIND_NAMES["measure"], kind, KIND_NAMES[kind]), text
    times = (C.c_float * 1)(0.0)
    stages = _capi.DrawStages()
    stages.fragment = measure.handle
    builtin = _capi.DepositUniforms()
    stages.builtin = C.cast(C.pointer(builtin), C.c_void_p)
    for kind, entry, args in (
            ("state", "th_program_run", (ctx, measure.handle, None, 0, _capi.TH_SOURCE_NONE, 0)),
            ("screen", "th_screen_run", (ctx, measure.handle, None, 0, None, 0, 0, 0, 1)),
            ("draw", "th_draw_program_run", (ctx, measure.handle, None, 0, _capi.TH_PASS_FLOW, C.byref(n))),
            ("step", "th_step_program_run", (ctx, measure.handle, None, 0, _capi.TH_SOURCE_NONE, times, C.c_float(0.0), 1)),
            ("fragment", "th_draw_stages_run", (ctx, C.byref(stages), _capi.TH_PASS_FLOW, C.byref(n)))):
        text = refused(entry, args)
        assert KIND_NAMES[kind] in text and "'exact' is a " + KIND_NAMES["measure"] in text, text
    # ... and nothing of it has hurt the context
    same_exact(p.measure(measure, dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3])), exact_channels(states[(48, 48)]))
    for handle in others.values():
        lib.th_program_destroy(handle)
    p.dispose()


def test_bad_arguments_are_refused_and_the_plumbing_serves_the_new_kind(programs, states):
    shape = (100, 37)
    st = states[shape]
    p = context(shape, st)
    ctx, prog = p._ctx, programs["general"]
    out, dev = _capi.MeasureResult(), C.c_void_p()
    for buffer in (-1, 2, 7):
        assert "buffer %d out of range" % buffer in refused("th_measure_run", (ctx, prog.handle, None, 0, buffer, C.byref(out)))
    block = (C.c_uint8 * 1025)()
    assert refused("th_measure_run", (ctx, prog.handle, block, 1025, 0, C.byref(out))) == "uniform block of 1025 bytes (at most 1024)"
    assert refused("th_measure_run", (ctx, prog.handle, None, 16, 0, C.byref(out))) == "null uniforms"
    assert "null" in refused("th_measure_run", (ctx, prog.handle, None, 0, 0, None))
    assert "null" in refused("th_measure_global", (ctx, prog.handle, None, 0, 0, None))
    assert refused("th_measure_run", (ctx, None, None, 0, 0, C.byref(out))) == "null program"
    call("th_measure_run", ctx, prog.handle, block, 1024, 0, C.byref(out))
    # registers and the LDS of the four-wave fold (4 x 144 bytes), for both channel counts' kernels
    for name in ("general", "nobody"):
        info = programs[name].query(p)
        print(name, info)
        assert info["vgprs"] > 0 and info["sgprs"] > 0 and info["code_bytes"] > 0 and info["lds_bytes"] == 4 * 144
    # enqueue only, then the stream's end, then the 144 bytes where they landed
    want = p.measure(prog)
    address = p.measure_async(prog)
    assert address
    p.sync()
    from tendrils_amd import sharding
    landed = sharding.device_view(address, (144,), "|u1").cpu().numpy().tobytes()
    assert landed == want.raw
    assert within_bound(want.sum[0], general_values(st))
    # a program destroyed after a run: the context that loaded it still runs it
    mine = MeasureProgram.from_source(GENERAL, channels=1, name="mine")
    first = p.measure(mine)
    handle = mine.handle
    call("th_program_destroy", handle)
    mine.handle = None
    call("th_measure_run", ctx, handle, None, 0, 0, C.byref(out))
    assert bytes(out) == first.raw == want.raw
    fresh = context(shape, st)                                # ... and one that had not cannot load it any more
    assert "was destroyed" in refused("th_measure_run", (fresh._ctx, handle, None, 0, 0, C.byref(out)))
    fresh.dispose()
    p.dispose()
