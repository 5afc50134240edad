"""Select on the GPU (include/tendrils_hip.h "select"; tendrils_amd/csrc/th_select.hip): the particles of a ring buffer that match
a box, a band of squared speeds and a thinning, as 32-byte records in TEXEL order.  The reference is numpy over the state in
texel order - what was uploaded, Particles.read(), or for packed rings the numpy codec of tests/helpers.py - evaluating the
header's expressions in np.float32 and np.flatnonzero; never the code under test.  Everything the library decides with is an
integer or a float compare, so records are compared bit for bit and the four counts exactly, whatever order the ring is held in.

Shapes: 5 x 3 (15 of 64 lanes: one partial wave under the ballot), 100 x 37 (3 700 = 57 mask words and 52 bits: a ragged last
word and workgroup), 1024 x 600 (614 400 slots = 9 600 count words: ten blocks of the 1 024-word scan, and more workgroups than
the 2 048 of the grid, whose stride loop takes a second turn); SORTED_SHAPES give tile-sorted slots.  Every test asserts ON THE
NUMPY REFERENCE that its selection is non-trivial - 0 < matched < live < particles - unless the case is about the trivial one."""
import ctypes as C

import numpy as np
import pytest

from tendrils_amd import _capi, sharding
from tendrils_amd._capi import call
from tendrils_amd.particles import SELECTED, Selection

from helpers import bits_equal, hashed_state, pack_state, unpack_state
from test_gpu_measure_program import SORTED_SHAPES, context, slot_order_read, sorted_buffers, step_until_sorted, tendrils

pytestmark = pytest.mark.gpu

F = np.float32
INERT = F(-1e6)
SHAPES = [(5, 3), (100, 37), (1024, 600)]
SEEDS = {(5, 3): 36, (100, 37): 131, (1024, 600): 1055, (48, 48): 79}
BOX = (-0.75, -0.5, 0.875, 0.75)           # x0, y0, x1, y1: exact in fp32
SPEED = (1.0, 3.5)                         # lo, hi in speed units (the velocities' components span about +-3)
CLAUSES = dict(box=dict(box=BOX), speed=dict(speed=SPEED), stride=dict(stride=3, phase=1),
               all=dict(box=BOX, speed=SPEED, stride=2, phase=1))
COUNTS = ("particles", "live", "matched", "written")
GUARD = 0xA5


# ---- the reference -------------------------------------------------------------------------------------------------------------
def square(v):
    with np.errstate(over="ignore"):
        return F(v) * F(v)


def matching(st, box=None, speed=None, stride=1, phase=0, inert=False, row0=0):
    """(mask over the texels of `st` [h, w, 4], live, global index) by the header's clauses in np.float32"""
    st = np.asarray(st, F)
    h, w = st.shape[:2]
    s = st.reshape(-1, 4)
    x, y, vz, vw = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    live = ~((x == INERT) & (y == INERT))
    m = live | bool(inert)
    with np.errstate(invalid="ignore", over="ignore"):
        if box is not None:
            x0, y0, x1, y1 = (F(v) for v in box)
            m = m & (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
        if speed is not None:
            q = (vz * vz) + (vw * vw)
            assert q.dtype == F
            m = m & (q >= square(speed[0])) & (q <= square(speed[1]))
    index = np.arange(h * w, dtype=np.int64) + row0 * w
    m = m & (index % stride == phase)
    return m, live, index


def reference(st, capacity=None, **kw):
    """what select() must return for `st` in texel order: dict(index, x, y, state, particles, live, matched, written)"""
    st = np.asarray(st, F)
    w = st.shape[1]
    m, live, index = matching(st, **kw)
    at = np.flatnonzero(m)
    written = len(at) if capacity is None else min(len(at), capacity)
    at = at[:written]
    return dict(index=index[at].astype(np.uint32), x=(index[at] % w).astype(np.uint32), y=(index[at] // w).astype(np.uint32),
                state=st.reshape(-1, 4)[at], particles=st.shape[0] * w, live=int(live.sum()), matched=int(m.sum()), written=written)


def nontrivial(want):
    return 0 < want["matched"] < want["live"] < want["particles"]


def same(got, want):
    assert isinstance(got, Selection)
    print("select: %r" % (got,))
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    for k in ("index", "x", "y"):
        assert getattr(got, k).dtype == np.uint32 and (getattr(got, k) == want[k]).all(), k
    assert got.state.shape == (want["written"], 4) and got.state.dtype == F
    wrong = ~bits_equal(got.state, want["state"])
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4])
    return want


def spread_state(w, h, seed):
    """hashed_state (positions in [-1, 1), one texel in seven inert) with the live positions scaled to about +-1.2 and the
    velocities to about +-3"""
    st = np.ascontiguousarray(hashed_state(w, seed, inert_mod=7, rows=(0, h)))
    live = ~((st[..., 0] == INERT) & (st[..., 1] == INERT))
    st[..., :2] = np.where(live[..., None], st[..., :2] * F(1.2), st[..., :2])
    st[..., 2:] = st[..., 2:] * F(300.0)
    return st


@pytest.fixture(scope="module")
def states():
    out = {}
    for (w, h), seed in SEEDS.items():
        st = spread_state(w, h, seed)
        st.setflags(write=False)
        out[(w, h)] = st
    return out


def uniforms(box=None, speed=None, stride=1, phase=0, inert=False, flags=None, reserved=0):
    u = _capi.SelectUniforms()
    u.stride, u.phase, u.reserved = stride, phase, reserved
    if box is not None:
        u.flags |= _capi.SELECT_BOX
        u.box[:] = box
    if speed is not None:
        u.flags |= _capi.SELECT_SPEED
        u.speed2[0], u.speed2[1] = float(square(speed[0])), float(square(speed[1]))
    if inert:
        u.flags |= _capi.SELECT_INERT
    if flags is not None:
        u.flags = flags
    return u


def raw_select(p, u, capacity, room=None, buffer=0):
    """th_select into `room` records (capacity + 3 by default) filled with GUARD: (info, the records' bytes [room, 32])"""
    room = capacity + 3 if room is None else room
    out = np.full((room, 32), GUARD, np.uint8)
    info = _capi.SelectInfo()
    call("th_select", p._ctx, C.byref(u), buffer, out.ctypes.data_as(C.POINTER(_capi.Selected)), capacity, C.byref(info))
    return info, out


def records_of(want):
    """the reference's records as the library lays them out: [written] SELECTED"""
    rec = np.zeros(want["written"], SELECTED)
    rec["state"], rec["index"], rec["x"], rec["y"] = want["state"], want["index"], want["x"], want["y"]
    return rec.view(np.uint8).reshape(-1, 32)


# ---- 1: texel order, f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clause", list(CLAUSES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_ring_in_texel_order_gives_numpys_records(states, shape, clause):
    st, kw = states[shape], CLAUSES[clause]
    want = reference(st, **kw)
    assert nontrivial(want), want
    p = context(shape, st)
    same(p.select(**kw), want)
    again = p.select(**kw)                                        # again: the same bits
    same(again, want)
    assert bits_equal(p.read(0), st).all()                        # (the ring is as it was)
    p.dispose()


# ---- 2: values planted on every boundary ---------------------------------------------------------------------------------------
def test_planted_boundary_values_fall_on_their_side(states):
    shape = (100, 37)
    st = np.array(states[shape])
    flat = st.reshape(-1, 4)
    x0, y0, x1, y1 = (F(v) for v in BOX)
    lo, hi = F(0.5), F(2.0)                                       # q in [0.25, 4.0]: z alone carries the speed below
    nan, inf = F(np.nan), F(np.inf)
    planted = [
        (x0, 0.0, 1.0, 0.0), (0.0, y0, 1.0, 0.0),                 # 0, 1: on x0, on y0 - inside
        (x1, 0.0, 1.0, 0.0), (0.0, y1, 1.0, 0.0),                 # 2, 3: on x1, on y1 - outside
        (np.nextafter(x1, F(-2)), np.nextafter(y1, F(-2)), 1.0, 0.0),      # 4: the last floats below both - inside
        (np.nextafter(x0, F(-2)), 0.0, 1.0, 0.0),                 # 5: the first float left of x0 - outside
        (0.0, 0.0, lo, 0.0), (0.0, 0.0, 0.0, -hi),                # 6, 7: q exactly lo * lo, hi * hi - match
        (0.0, 0.0, np.nextafter(lo, F(0)), 0.0), (0.0, 0.0, np.nextafter(hi, F(3)), 0.0),      # 8, 9: just outside both
        (nan, 0.0, 1.0, 0.0), (0.0, nan, 1.0, 0.0),               # 10, 11: a NaN position - live, fails under BOX
        (0.0, 0.0, nan, 1.0), (0.0, 0.0, 1.0, nan),               # 12, 13: a NaN velocity: q is NaN
        (0.0, 0.0, inf, 0.0), (0.0, 0.0, 1.0, -inf),              # 14, 15: q is +inf
        (INERT, INERT, 1.0, 0.0),                                 # 16: inert, with a speed inside the band
        (INERT, 0.0, 1.0, 0.0),                                   # 17: one coordinate alone does not make it inert
    ]
    at = 1000
    flat[at:at + len(planted)] = np.array(planted, F)
    k = lambda *which: [at + i for i in which]
    cases = [
        (dict(box=BOX), k(0, 1, 4, 6, 7, 8, 9, 12, 13, 14, 15), k(2, 3, 5, 10, 11, 16, 17)),
        (dict(speed=(lo, hi)), k(0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 17), k(8, 9, 12, 13, 14, 15, 16)),
        (dict(speed=(lo, inf)), k(6, 7, 9, 10, 11, 14, 15, 17), k(8, 12, 13, 16)),
        (dict(speed=(lo, hi), inert=True), k(16, 17, 10), k(12, 14)),
        (dict(box=BOX, speed=(lo, hi), inert=True), k(0, 1, 4, 6, 7), k(2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)),
        (dict(inert=True), k(*range(len(planted))), []),
    ]
    p = context(shape, st)
    for kw, inside, outside in cases:
        want = reference(st, **kw)
        chosen = set(want["index"].tolist())
        assert set(inside) <= chosen and not (set(outside) & chosen), (kw, sorted(set(inside) - chosen), sorted(set(outside) & chosen))
        assert "inert" in kw or nontrivial(want)
        same(p.select(**kw), want)
    # the NaN positions are live and match where no box is asked; the inert one only under TH_SELECT_INERT without a box
    assert p.select(inert=True).matched == 3700 and p.select().matched == reference(st)["live"]
    p.dispose()


# ---- 3: the thinning -----------------------------------------------------------------------------------------------------------
def test_the_phases_of_a_stride_partition_the_selection(states):
    shape = (100, 37)
    st = states[shape]
    p = context(shape, st)
    whole = same(p.select(box=BOX), reference(st, box=BOX))
    assert nontrivial(whole)
    parts = [p.select(box=BOX, stride=7, phase=k) for k in range(7)]
    for k, part in enumerate(parts):
        same(part, reference(st, box=BOX, stride=7, phase=k))
        assert part.matched > 0 and (part.index % 7 == k).all() and (np.diff(part.index.astype(np.int64)) > 0).all()
    joined = np.concatenate([part.index for part in parts])
    assert len(joined) == len(set(joined.tolist())) == whole["matched"]          # pairwise disjoint ...
    assert (np.sort(joined) == whole["index"]).all()                             # ... and their union is the whole
    # no clause: every live particle; with the inert ones: every particle
    live = same(p.select(), reference(st))
    assert live["matched"] == live["live"] < live["particles"]
    everyone = same(p.select(inert=True), reference(st, inert=True))
    assert everyone["matched"] == everyone["particles"] == 3700 and (everyone["index"] == np.arange(3700)).all()
    big = (1024, 600)
    q = context(big, states[big])
    everyone = same(q.select(inert=True), reference(states[big], inert=True))    # (every bit of 9 600 words set)
    assert everyone["matched"] == big[0] * big[1]
    q.dispose()
    p.dispose()


# ---- 4: nothing matches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_an_empty_box_matches_nothing_and_writes_nothing(states, shape):
    st = states[shape]
    empty = (0.25, -2.0, 0.25, 2.0)                               # x0 == x1: half-open, nobody
    want = reference(st, box=empty)
    assert want["matched"] == 0 < want["live"] < want["particles"]
    p = context(shape, st)
    info, out = raw_select(p, uniforms(box=empty), 8)
    assert (info.particles, info.live, info.matched, info.written) == (want["particles"], want["live"], 0, 0)
    assert (out == GUARD).all()
    same(p.select(box=empty), want)
    p.dispose()


# ---- 5: capacity ---------------------------------------------------------------------------------------------------------------
def test_capacity_truncates_to_the_first_records_and_the_guard_stays(states):
    shape = (100, 37)
    st, kw = states[shape], CLAUSES["all"]
    full = reference(st, **kw)
    assert nontrivial(full) and full["matched"] > 3
    all_bytes = records_of(full)
    p = context(shape, st)
    u = uniforms(**kw)
    # out null: counts only, whatever the capacity says
    info = _capi.SelectInfo()
    call("th_select", p._ctx, C.byref(u), 0, None, 1 << 40, C.byref(info))
    assert (info.particles, info.live, info.matched, info.written) == (full["particles"], full["live"], full["matched"], 0)
    for capacity in (full["matched"] - 1, 1, 0, full["matched"], full["matched"] + 5, 1 << 16):
        info, out = raw_select(p, u, capacity)                    # (the caller's buffer: `capacity` records, and three of guard behind them)
        written = min(capacity, full["matched"])
        assert (info.particles, info.live, info.matched, info.written) == (full["particles"], full["live"], full["matched"], written), capacity
        assert (out[:written] == all_bytes[:written]).all(), capacity              # the FIRST `written` of the full selection
        assert len(out) == capacity + 3 and (out[capacity:] == GUARD).all(), capacity      # past `capacity` records: untouched
    same(p.select(capacity=5, **kw), reference(st, capacity=5, **kw))
    p.dispose()


# ---- 6: tile-sorted slots, f32 and packed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_tile_sorted_slots_give_the_records_of_texel_order_and_stay_sorted(states, shape, view, fmt):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)                    # (velocities the integrator keeps: about +-0.01)
    t = tendrils(shape, view, st, fmt)
    p = t.particles
    step_until_sorted(t)
    assert sorted_buffers(p) > 0
    is_sorted, perm_before, slots_before = slot_order_read(p, 0, fmt == "f16")
    assert is_sorted and not (perm_before == np.arange(perm_before.size)).all()
    # the slots put back into texel order through the table - and, packed, decoded by the numpy mirror of the codec
    texels = np.zeros_like(slots_before)
    texels[perm_before] = slots_before
    back = (unpack_state(texels) if fmt == "f16" else texels.view(F)).reshape(shape[1], shape[0], 4)
    q = (back[..., 2] * back[..., 2]) + (back[..., 3] * back[..., 3])
    live = ~((back[..., 0] == INERT) & (back[..., 1] == INERT))
    middle = F(np.sqrt(np.median(q[live].astype(np.float64))))    # a speed that parts the live particles, whatever the steps left
    picks = [dict(box=BOX), dict(speed=(0.0, middle)), dict(box=BOX, speed=(0.0, middle), stride=2, phase=1), dict(stride=5, phase=3, inert=True)]
    got = [p.select(**kw) for kw in picks]
    forwarded = t.select(box=BOX)                                 # Tendrils.select: buffers[0]
    again, perm_after, slots_after = slot_order_read(p, 0, fmt == "f16")
    assert again and (perm_after == perm_before).all() and (slots_after == slots_before).all()
    assert sorted_buffers(p) > 0
    for kw, sel in zip(picks, got):
        want = same(sel, reference(back, **kw))
        assert nontrivial(want) or kw.get("inert"), (kw, want["matched"])
    same(forwarded, reference(back, box=BOX))
    other = p.select(box=BOX, buffer=1)                           # the other buffer, in whatever order it is held
    assert bits_equal(p.read(0), back).all()                      # (texel order: from here on the ring is no longer sorted)
    same(other, reference(p.read(1), box=BOX))
    same(p.select(box=BOX), reference(back, box=BOX))             # ... and now through the texel-order path
    t.dispose()


# ---- 7: a packed ring in texel order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_packed_ring_in_texel_order(states, shape):
    st = states[shape]
    p = context(shape, st, packed=True)
    decoded = unpack_state(pack_state(st))                        # what the 8-byte texels hold, by the numpy mirror of the codec
    assert bits_equal(p.read(0), decoded).all() and not bits_equal(decoded, st).all()
    for kw in CLAUSES.values():
        want = reference(decoded, **kw)
        assert nontrivial(want)
        same(p.select(**kw), want)
    p.dispose()


# ---- 8: read-only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_step_select_draw_leaves_the_bits_of_step_draw(states, shape, view):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)
    a, b = tendrils(shape, view, st), tendrils(shape, view, st)
    for frame in range(3):
        for t in (a, b):
            t.timer.tick()
            t.step()
        before = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]      # (the twin is read as well: both take the same calls but the select)
        assert a.select(box=BOX).matched > 0
        a.particles.select(speed=(0.0, 0.01), stride=3, phase=2, buffer=1, capacity=7)
        a.particles.select_async(100, box=BOX, inert=True)
        after = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]
        for (s0, perm0, slots0), (s1, perm1, slots1) in zip(before, after):
            assert s0 == s1 and (perm0 == perm1).all() and (slots0 == slots1).all()
        for t in (a, b):
            t.draw()
        qa, qb = _capi.DrawInfo(), _capi.DrawInfo()
        call("th_draw_query", a.particles._ctx, C.byref(qa))
        call("th_draw_query", b.particles._ctx, C.byref(qb))
        assert (qa.pipeline, qa.fragments, qa.crowded_fragments) == (qb.pipeline, qb.fragments, qb.crowded_fragments)
        assert a.fragments == b.fragments > 0
        assert sorted_buffers(a.particles) == sorted_buffers(b.particles)
    assert sorted_buffers(a.particles) > 0
    assert any(s0 for s0, _perm, _slots in before)
    assert a.particles.stats(0.01) == b.particles.stats(0.01)          # (the respawned counter among them)
    assert bits_equal(a.flow.read(), b.flow.read()).all()
    assert (a.read_view() == b.read_view()).all() and a.read_view().any()
    for k in (0, 1):
        assert bits_equal(a.particles.read(k), b.particles.read(k)).all()
    a.dispose(); b.dispose()


# ---- 9: a row band -------------------------------------------------------------------------------------------------------------
def test_a_row_band_selects_its_rows_with_the_whole_textures_indices(states):
    shape, band = (100, 37), (25, 12)
    st = states[shape]
    rows = st[band[0]:band[0] + band[1]]
    p = context((shape[0], band[1]), rows, row0=band[0], global_height=shape[1])
    for kw in (CLAUSES["all"], dict(stride=7, phase=3), dict(box=BOX, stride=3, phase=0)):
        whole = reference(st, **kw)
        inside = (whole["y"] >= band[0]) & (whole["y"] < band[0] + band[1])
        want = reference(rows, row0=band[0], **kw)
        assert nontrivial(want) and (want["index"] == whole["index"][inside]).all() and (want["y"] == whole["y"][inside]).all()
        assert bits_equal(want["state"], whole["state"][inside]).all()
        assert want["index"].min() >= band[0] * shape[0] and want["particles"] == shape[0] * band[1]
        # (the stride runs over the WHOLE texture's index: 2 500 texels in front of this band, not a multiple of 7 or 3)
        assert (want["index"] % kw.get("stride", 1) == kw.get("phase", 0)).all()
        same(p.select(**kw), want)
    p.dispose()


# ---- 10: enqueue only ----------------------------------------------------------------------------------------------------------
def landed(p, addresses, count):
    records, info = addresses
    p.sync()
    counts = [int(v) for v in sharding.device_view(info, (4,), "<u8").cpu().numpy()]
    if not count:
        return counts, np.zeros((0, 32), np.uint8)
    return counts, sharding.device_view(records, (count, 32), "|u1").cpu().numpy()


def test_async_leaves_the_synchronous_calls_records_on_the_device(states):
    shape = (100, 37)
    st, kw = states[shape], CLAUSES["box"]
    full = reference(st, **kw)
    assert nontrivial(full) and full["matched"] > 40
    all_bytes = records_of(full)
    p = context(shape, st)
    for capacity in (16, full["matched"] + 100, 0, 1 << 40):      # a larger one after a smaller one: the records grow
        addresses = p.select_async(capacity, **kw)
        written = min(capacity, full["matched"])
        assert addresses[1] and bool(addresses[0]) == (capacity > 0)
        counts, records = landed(p, addresses, written)
        assert counts == [full["particles"], full["live"], full["matched"], written], capacity
        assert (records == all_bytes[:written]).all(), capacity
    same(p.select(**kw), full)                                    # the synchronous call after them: the same records
    lib = _capi.load()
    assert lib.th_select_async(p._ctx, C.byref(uniforms(**kw)), 0, 4, None, None) == _capi.TH_OK      # (both pointers may be null)
    p.sync()
    p.dispose()


# ---- 11: refusals --------------------------------------------------------------------------------------------------------------
# (every refusal of the header but one: a context of more than 2^28 texels is 4 GiB of state a buffer - not a quick test's)
def test_every_bad_argument_is_refused_by_name_and_the_next_call_is_unaffected(states):
    shape = (5, 3)
    st = states[shape]
    p = context(shape, st)
    lib, ctx = _capi.load(), p._ctx
    nan, inf = float("nan"), float("inf")
    good = uniforms(box=BOX, speed=SPEED)
    bad = [("null uniforms", None, 0), ("buffer -1", good, -1), ("buffer 2", good, 2),
           ("stride 0", uniforms(stride=0), 0), ("phase == stride", uniforms(stride=3, phase=3), 0), ("phase > stride", uniforms(stride=1, phase=2), 0),
           ("flag 8", uniforms(flags=8), 0), ("flag 1 << 31", uniforms(box=BOX, flags=(1 << 31) | 1), 0), ("reserved", uniforms(reserved=1), 0),
           ("box x0 nan", uniforms(box=(nan, 0, 1, 1)), 0), ("box y1 nan", uniforms(box=(0, 0, 1, nan)), 0),
           ("speed lo nan", uniforms(speed=(nan, 1.0)), 0), ("speed hi nan", uniforms(speed=(0.0, nan)), 0)]
    out, info = (_capi.Selected * 16)(), _capi.SelectInfo()
    records, device_info = C.c_void_p(), C.c_void_p()
    for what, u, buffer in bad:
        ref = None if u is None else C.byref(u)
        assert lib.th_select(ctx, ref, buffer, out, 16, C.byref(info)) == _capi.TH_ERR_INVALID, what
        assert b"th_select:" in lib.th_last_error(), (what, lib.th_last_error())
        assert lib.th_select_async(ctx, ref, buffer, 16, C.byref(records), C.byref(device_info)) == _capi.TH_ERR_INVALID, what
        assert b"th_select_async:" in lib.th_last_error(), (what, lib.th_last_error())
    assert lib.th_select(ctx, C.byref(good), 0, out, 16, None) == _capi.TH_ERR_INVALID and b"th_select:" in lib.th_last_error()
    assert lib.th_select(None, C.byref(good), 0, out, 16, C.byref(info)) == _capi.TH_ERR_INVALID and b"th_select:" in lib.th_last_error()
    assert lib.th_select_async(None, C.byref(good), 0, 16, None, None) == _capi.TH_ERR_INVALID and b"th_select_async:" in lib.th_last_error()
    # a NaN in a clause that is NOT asked is nobody's business, and infinities are bounds like any other
    idle = uniforms(stride=2, phase=1)
    idle.box[0], idle.speed2[1] = nan, nan
    call("th_select", ctx, C.byref(idle), 0, None, 0, C.byref(info))
    assert info.matched == reference(st, stride=2, phase=1)["matched"] > 0
    same(p.select(box=(-inf, -inf, inf, inf), speed=(0.0, inf)), reference(st, box=(-inf, -inf, inf, inf), speed=(0.0, inf)))
    # ... and the valid call after all of that is the one it would have been
    want = reference(st, box=BOX, speed=SPEED)
    assert nontrivial(want)
    same(p.select(box=BOX, speed=SPEED), want)
    p.dispose()


# ---- 12: the Python host -------------------------------------------------------------------------------------------------------
def test_the_host_fetches_exactly_matched_and_squares_the_speeds_in_float32(states):
    shape = (100, 37)
    st = np.array(states[shape])
    # A bound `hi` (a Python float, no float32) whose square the two arithmetics part: float32(hi) is z, and z * z in float32
    # is above the float64 square of hi rounded to float32.  A particle of speed exactly z then has q = z * z: on the closed
    # bound under the header's float32 square - it matches -, above the bound a host squaring in float64 would hand over.
    found = None
    for k in range(1, 4096):
        z = F(1.0 + 0.001 * k)                                    # (every mantissa bit in use)
        hi = float(z) * (1.0 - 2.0 ** -26)
        if F(hi) == z and F(hi * hi) < z * z:
            found = (z, hi)
            break
    assert found, "no bound whose float64 square rounds below its float32 square"
    z, hi = found
    st.reshape(-1, 4)[2000] = [0.0, 0.0, z, 0.0]
    kw = dict(speed=(0.25, hi))
    want = reference(st, **kw)
    assert nontrivial(want) and 2000 in want["index"] and not (z * z <= F(hi * hi))
    p = context(shape, st)
    got = same(p.select(**kw), want)                              # capacity=None: exactly `matched` records
    assert got["written"] == got["matched"] == len(p.select(**kw).index)
    assert len(p.select(capacity=3, **kw)) == 3 and "matched=%d" % want["matched"] in repr(p.select(capacity=3, **kw))
    p.dispose()
    t = tendrils((48, 48), (32, 24), np.array(states[(48, 48)]))
    kw = dict(box=BOX, stride=3, phase=2)
    want = reference(states[(48, 48)], **kw)
    assert nontrivial(want)
    same(t.select(**kw), want)                                    # Tendrils.select forwards (nothing has stepped: the uploaded state)
    t.dispose()
