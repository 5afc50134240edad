"""Follow on the GPU (include/tendrils_hip.h "follow"; tendrils_amd/csrc/th_follow.hip): the states of a chosen set of particles,
sample by sample, in a history kept on the device.  The reference is numpy indexing of the state in texel order - what was
uploaded, for packed rings the numpy codec of tests/helpers.py - and, for a ring that must stay in tile-sorted slots, the records
of select(inert=True) over everything (every texel, in texel order: a route that exists on the device already and is tested
against numpy in test_gpu_select.py); never the code under test.  A sample only copies, so everything is compared bit for bit.

Shapes: 5 x 3 (15 of 64 lanes, one mask word), 100 x 37 (3 700 texels = 57 mask words and 52 bits: a ragged last word and
workgroup), 1024 x 600 (614 400 texels = 9 600 count words: ten blocks of the 1 024-word scan; followed whole it is 2 400
workgroups of the gather, and its perm table more than the 2 048 workgroups of the locate's grid: the stride loop takes a second
turn); SORTED_SHAPES give tile-sorted slots.  Sets of 1, 63, 64, 65 and 257 members (a lane, a wave less one, a wave, a wave
and one, a workgroup and one) and of all texels; every set of two or more holds the first and the last texel."""
import ctypes as C

import numpy as np
import pytest

from tendrils_amd import _capi, sharding
from tendrils_amd._capi import call
from tendrils_amd.particles import Follow

from helpers import bits_equal, pack_state, unpack_state
from test_gpu_measure_program import SORTED_SHAPES, context, slot_order_read, sorted_buffers, step_until_sorted, tendrils
from test_gpu_select import BOX, spread_state

pytestmark = pytest.mark.gpu

F = np.float32
INERT = F(-1e6)
SHAPES = [(5, 3), (100, 37), (1024, 600)]
SEEDS = {(5, 3): 41, (100, 37): 137, (1024, 600): 1061, (48, 48): 83}
SIZES = (1, 63, 64, 65, 257, None)            # None: every texel
GUARD = np.uint32(0xA5A5A5A5)
INVALID = _capi.TH_ERR_INVALID


# ---- the states and the sets ---------------------------------------------------------------------------------------------------
def planted_state(w, h, seed):
    """spread_state (one texel in seven inert, positions about +-1.2, velocities about +-3) with the first texel inert, a NaN
    position, signed zeros and infinities behind it, and a live last texel"""
    st = spread_state(w, h, seed)
    flat = st.reshape(-1, 4)
    nan, inf = F(np.nan), F(np.inf)
    flat[0] = [INERT, INERT, 1.0, -0.0]
    flat[1] = [nan, 0.5, -0.0, 0.0]
    flat[2] = [0.0, -0.0, inf, -inf]
    flat[3] = [-0.0, 0.25, -0.0, 2.5]
    flat[-1] = [0.25, -0.5, -1.5, 0.0]
    return st


@pytest.fixture(scope="module")
def states():
    out = {}
    for (w, h), seed in SEEDS.items():
        st = planted_state(w, h, seed)
        st.setflags(write=False)
        out[(w, h)] = st
    return out


def moving(st):
    """a state to step: velocities the integrator keeps, about +-0.01, and the planted NaN and infinities taken out again (what
    a copy does with them is case 1's; here the particles have to move)"""
    st = np.array(st)
    st[..., :2] = np.where(np.isfinite(st[..., :2]), st[..., :2], F(0.5))
    st[..., 2:] = np.where(np.isfinite(st[..., 2:]), st[..., 2:] * F(1.0 / 300.0), F(0.0))
    return st


def a_set(count, n, seed):
    """`n` texels of `count`, strictly increasing: the planted ones, the last one and a seeded draw of the rest"""
    if n is None or n >= count:
        return np.arange(count, dtype=np.uint32)
    if n == 1:
        return np.array([count - 1], np.uint32)
    fixed = [0, 1, 2, 3, count - 1][:n - 1] + [count - 1]
    fixed = sorted(set(fixed))
    rest = np.setdiff1d(np.arange(count), fixed)
    drawn = np.random.default_rng(seed).choice(rest, n - len(fixed), replace=False)
    out = np.sort(np.concatenate([np.array(fixed, np.int64), drawn])).astype(np.uint32)
    assert len(out) == n and (np.diff(out.astype(np.int64)) > 0).all() and out[0] == 0 and out[-1] == count - 1
    return out


def live_of(rows):
    return ~((rows[:, 0] == INERT) & (rows[:, 1] == INERT))


def same_rows(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    wrong = ~bits_equal(got, want)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4])
    # bits_equal lets any NaN stand for any NaN; an f32 ring is copied: the same words (a packed ring decodes its NaN position)
    return got


def everyone(p, buffer=0):
    """the decoded state of every texel of a ring buffer, in texel order, the ring left where it lies: select's records"""
    sel = p.select(inert=True, buffer=buffer)
    count = p.shape[0] * p.shape[1]
    assert sel.matched == sel.written == count and (sel.index == np.arange(count) + p._row0 * p.shape[0]).all()
    return sel.state


def slot_order(p):
    info = _capi.SlotOrderInfo()
    call("th_slot_order", p._ctx, C.byref(info))
    return int(info.sorts), int(info.sorted_buffers)


def counters(f):
    i = f.info
    return i.samples, i.held, i.locates


def raw_read(p, n, first, count, room=2):
    """th_follow_read of `count` samples into a buffer with `room` rows of guard words behind them: (status, states, times, guard
    rows, guard times, info)"""
    states = np.full((count + room, n, 4), GUARD, np.uint32)
    times = np.full(count + room, -7.0, np.float64)
    info = _capi.FollowInfo()
    status = _capi.load().th_follow_read(p._ctx, first, count, states.ctypes.data_as(_capi._fp), times.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
    return status, states[:count].view(F), times[:count], states[count:], times[count:], info


# ---- 1: texel order, f32 and packed --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_ring_in_texel_order_gives_numpys_rows(states, shape, fmt):
    st = states[shape]
    count = shape[0] * shape[1]
    p = context(shape, st, packed=fmt == "f16")
    ref = (unpack_state(pack_state(st)) if fmt == "f16" else st).reshape(-1, 4)
    if fmt == "f16":
        assert bits_equal(p.read(0), ref.reshape(st.shape)).all() and not bits_equal(ref, st.reshape(-1, 4)).all()
    for k, n in enumerate(SIZES):
        index = a_set(count, n, 1000 + k)
        want = ref[index]
        if len(index) > 1:
            assert index[0] == 0 and index[-1] == count - 1
            assert live_of(want).any() and not live_of(want).all()          # an inert and a live particle, on the reference
        if len(index) > 4:
            assert np.isnan(want).any() and np.isinf(want).any() and (want.view(np.uint32) == 0x80000000).any()
        f = p.follow(index, depth=2)
        assert isinstance(f, Follow) and len(f) == len(index)
        f.sample(time=2.5)
        got, times = f.paths()
        assert got.shape == (len(index), 1, 4) and got.dtype == F and list(times) == [2.5]
        same_rows(got[:, 0], want)
        if fmt == "f32":
            assert (np.ascontiguousarray(got[:, 0]).view(np.uint32) == want.view(np.uint32)).all()      # a copy: the NaN's own bits
        info = f.info
        assert (info.particles, info.followed, info.depth, info.samples, info.held, info.locates) == (count, len(index), 2, 1, 1, 0)
    assert bits_equal(p.read(0), ref.reshape(st.shape)).all()    # (the ring is as it was)
    p.dispose()


# ---- 2: tile-sorted slots, f32 and packed --------------------------------------------------------------------------------------
def sorted_case(t, index, packed):
    """sample buffer 0 and buffer 1 of a ring in tile-sorted slots against select's records; the ring stays as it lies"""
    p = t.particles
    assert sorted_buffers(p) > 0
    before = sorted_buffers(p)
    is_sorted, perm_before, slots_before = slot_order_read(p, 0, packed)
    assert is_sorted and not (perm_before == np.arange(perm_before.size)).all()
    want = [everyone(p, 0)[index], everyone(p, 1)[index]]
    assert live_of(want[0]).any() and not bits_equal(want[0], want[1]).all()
    f = t.follow(index, depth=4)
    f.sample(buffer=0)
    f.sample(time=-1.0, buffer=1)
    f.sample()
    got, times = f.paths()
    assert got.shape == (len(index), 3, 4) and list(times) == [t.timer.time, -1.0, t.timer.time]
    again, perm_after, slots_after = slot_order_read(p, 0, packed)
    assert again and (perm_after == perm_before).all() and (slots_after == slots_before).all()
    assert sorted_buffers(p) == before
    same_rows(got[:, 0], want[0]); same_rows(got[:, 1], want[1]); same_rows(got[:, 2], want[0])
    assert f.info.locates >= 1
    # the slot table is the inverse of perm on the set: slot table[r] holds texel index[r]
    table = C.c_void_p()
    call("th_follow_query", p._ctx, None, None, C.byref(table))
    p.sync()
    slots = sharding.device_view(table.value, (len(index),), "<u4").cpu().numpy()
    assert (perm_before[slots] == index).all()                    # (the last sample read buffer 0)
    whole = p.read(0)                                             # (texel order: from here on the ring is no longer sorted)
    same_rows(got[:, 2], whole.reshape(-1, 4)[index])
    f.sample()                                                    # ... and now through the texel-order path
    same_rows(f.paths(last=1)[0][:, 0], whole.reshape(-1, 4)[index])
    return f


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_tile_sorted_slots_give_the_rows_of_texel_order_and_stay_sorted(states, shape, view, fmt):
    t = tendrils(shape, view, moving(states[shape]), fmt)
    step_until_sorted(t)
    box = t.select(box=BOX)
    assert 0 < box.matched < box.live < box.particles
    sorted_case(t, box.index, fmt == "f16")
    t.dispose()


def test_a_perm_table_longer_than_the_grid_is_walked_to_its_end(states):
    shape, view = (1024, 600), (640, 360)
    assert shape[0] * shape[1] > 2048 * 256
    t = tendrils(shape, view, moving(states[shape]))
    step_until_sorted(t)
    sorted_case(t, np.arange(0, shape[0] * shape[1], 5, dtype=np.uint32), False)
    t.dispose()


# ---- 3: the slot table follows the order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_the_slot_table_is_found_again_when_and_only_when_the_order_changes(states, fmt):
    """A loop of step(); sample() with a re-sort every second step and NO draw.  The invariant held: a step() over which
    th_slot_order's `sorts` and `sorted_buffers` did not change adds no locate to the sample of buffer 0 behind it.  That is
    right in such a loop: without draws every new order is laid out by the step that moves its output into it (begin_sort
    raises `sorts` in the same call), and a step that does not sort writes its output at its input's slots - the new buffer 0 is
    held in the (order, stamp) the old one was.  In a loop WITH draws it would not be: there the re-sort runs beside the draw
    (asort_start raises `sorts` behind one step) and the order is taken up by the NEXT step (asort_take), over which `sorts`
    stands still - the key the table is cached under is the sampled buffer's (order, stamp), not `sorts`."""
    shape, view = SORTED_SHAPES[0]
    t = tendrils(shape, view, moving(states[shape]), fmt)
    p = t.particles
    p.option("resort_steps", 2)
    p.option("rebucket_steps", 2)
    step_until_sorted(t)
    index = t.select(box=BOX).index
    assert 0 < len(index) < shape[0] * shape[1]
    f = t.follow(index, depth=16)
    f.sample()
    assert f.info.locates == 1
    sorts0, locates0 = slot_order(p)[0], 1
    perms, quiet_steps = set(), 0
    for frame in range(12):
        order_before, locates_before = slot_order(p), f.info.locates
        t.timer.tick()
        t.step()
        order_after = slot_order(p)
        f.sample()
        between = f.info.locates                                  # (th_follow_query launches nothing)
        f.sample()                                                # two samples with no call between them: the second finds its table
        locates = f.info.locates
        assert locates == between, (frame, between, locates)
        got = f.paths(last=2)[0]
        want = everyone(p, 0)[index]
        same_rows(got[:, 0], want); same_rows(got[:, 1], want)
        assert locates - locates_before in (0, 1), (frame, locates_before, locates)
        if order_after == order_before:
            quiet_steps += 1
            assert locates == locates_before, (frame, order_before, locates_before, locates)
        is_sorted, perm, _slots = slot_order_read(p, 0, fmt == "f16")
        if is_sorted:
            perms.add(perm.tobytes())
    print("follow: sorts %d -> %d, locates %d -> %d, %d perms seen, %d quiet steps" % (sorts0, slot_order(p)[0], locates0, f.info.locates, len(perms), quiet_steps))
    assert slot_order(p)[0] > sorts0 and f.info.locates > locates0
    assert len(perms) >= 2                                        # (the test's own observation: the order did change)
    assert quiet_steps > 0
    for buffer in (0, 1, 0):                                      # whatever it does to `locates`
        f.sample(buffer=buffer)
        same_rows(f.paths(last=1)[0][:, 0], everyone(p, buffer)[index])
    t.dispose()


# ---- 4: the history ------------------------------------------------------------------------------------------------------------
def test_the_history_keeps_the_last_depth_samples_across_the_wrap(states):
    shape, view = SORTED_SHAPES[0]
    t = tendrils(shape, view, moving(states[shape]))
    p = t.particles
    index = a_set(shape[0] * shape[1], 65, 7)
    n = len(index)
    f = p.follow(index, depth=3)
    want = []
    for k in range(7):
        t.timer.tick()
        t.step()
        f.sample(time=10.0 + k)
        want.append(everyone(p, 0)[index])
    assert not bits_equal(want[4], want[5]).all() and not bits_equal(want[5], want[6]).all()
    info = f.info
    assert (info.followed, info.depth, info.samples, info.held) == (n, 3, 7, 3)
    status, got, times, guard, guard_times, info = raw_read(p, n, 4, 3)
    assert status == _capi.TH_OK and (info.samples, info.held) == (7, 3)
    for k in range(3):
        same_rows(got[k], want[4 + k])                            # rows 1, 2, 0 of the history: across the wrap
    assert list(times) == [14.0, 15.0, 16.0]
    assert (guard == GUARD).all() and (guard_times == -7.0).all()
    status, got, times, guard, guard_times, _info = raw_read(p, n, 5, 1)       # a range inside what is held
    assert status == _capi.TH_OK and list(times) == [15.0] and (guard == GUARD).all()
    same_rows(got[0], want[5])
    lib = _capi.load()
    for first, count in ((3, 3), (5, 3), (7, 1), (0, 1)):
        status, got, times, guard, guard_times, _info = raw_read(p, n, first, count)
        assert status == INVALID and b"th_follow_read:" in lib.th_last_error(), (first, count)
        assert (got.view(np.uint32) == GUARD).all() and (times == -7.0).all()
    got, times = f.paths(last=2)
    assert got.shape == (n, 2, 4) and list(times) == [15.0, 16.0]
    same_rows(got[:, 0], want[5]); same_rows(got[:, 1], want[6])
    got, times = f.paths()
    assert got.shape == (n, 3, 4) and list(times) == [14.0, 15.0, 16.0]
    info = _capi.FollowInfo()                                     # count == 0 with null states: the info alone
    call("th_follow_read", p._ctx, 0, 0, None, None, C.byref(info))
    assert (info.samples, info.held, info.depth) == (7, 3, 3)
    t.dispose()


# ---- 5: replacing and ending ---------------------------------------------------------------------------------------------------
def test_a_new_set_replaces_the_old_one_and_n_0_ends_following(states):
    shape, view = SORTED_SHAPES[1]
    count = shape[0] * shape[1]
    t = tendrils(shape, view, moving(states[shape]))
    p = t.particles
    step_until_sorted(t)
    lib = _capi.load()
    ref = everyone(p, 0)
    first = p.follow(a_set(count, 64, 1), depth=2)
    first.sample(); first.sample(); first.sample()
    assert counters(first) == (3, 2, 1) and first.followed
    for n, seed in ((257, 2), (63, 3)):                           # a larger set, then a smaller one
        f = p.follow(a_set(count, n, seed), depth=5)
        assert f.followed and not first.followed
        assert counters(f) == (0, 0, 0) and f.info.followed == n and f.info.depth == 5
        status, _got, _times, _guard, _gt, _info = raw_read(p, n, 0, 1)
        assert status == INVALID and b"th_follow_read:" in lib.th_last_error()      # nothing is held yet
        f.sample(time=1.0)
        assert counters(f) == (1, 1, 1)
        got, times = f.paths()
        assert got.shape == (n, 1, 4) and list(times) == [1.0]
        same_rows(got[:, 0], ref[f.index])
        # the handle of a replaced set (64 members: the history's rows are 257, then 63 wide) raises before it reserves or
        # reads anything, and the set that is followed takes no sample and loses none through it
        for stale in (lambda: first.paths(), lambda: first.paths(last=1), lambda: first.read(0, 1), lambda: first.sample(), lambda: first.info):
            with pytest.raises(RuntimeError, match="no longer followed"):
                stale()
        first.stop()                                              # (nothing: it does not end the set that replaced it)
        assert counters(f) == (1, 1, 1) and f.info.followed == n
        same_rows(f.paths()[0][:, 0], ref[f.index])
    # th_follow_set called beside the handle: the context follows a set of another size, and the handle - whose buffers are
    # sized by its own - raises rather than hand th_follow_read too small a buffer; back on its own set it reads again
    other = a_set(count, 257, 9)
    call("th_follow_set", p._ctx, other.ctypes.data_as(C.POINTER(C.c_uint32)), len(other), 5)
    call("th_follow_sample", p._ctx, 0, 0.0)
    for stale in (lambda: f.paths(), lambda: f.read(0, 1), lambda: f.info):
        with pytest.raises(RuntimeError, match="the context follows 257"):
            stale()
    status, got, _times, guard, _gt, info = raw_read(p, 257, 0, 1)      # (the rows ARE 257 wide: the guard behind them stays)
    assert status == _capi.TH_OK and info.followed == 257 and (guard == GUARD).all()
    same_rows(got[0], ref[other])
    call("th_follow_set", p._ctx, f.index.ctypes.data_as(C.POINTER(C.c_uint32)), len(f), 5)
    f.sample(time=1.0)
    assert counters(f) == (1, 1, 1)
    # a refused set leaves the previous one followed
    unsorted = np.array(f.index)
    unsorted[10], unsorted[11] = unsorted[11], unsorted[10]
    assert lib.th_follow_set(p._ctx, unsorted.ctypes.data_as(C.POINTER(C.c_uint32)), len(unsorted), 5) == INVALID
    assert b"th_follow_set:" in lib.th_last_error() and b"position 11" in lib.th_last_error(), lib.th_last_error()
    assert counters(f) == (1, 1, 1) and f.info.followed == 63
    f.sample(time=2.0)
    got, times = f.paths()
    assert list(times) == [1.0, 2.0]
    same_rows(got[:, 1], ref[f.index])
    # n == 0 ends it
    f.stop()
    assert not f.followed
    info = _capi.FollowInfo()
    call("th_follow_query", p._ctx, C.byref(info), None, None)
    assert (info.particles, info.followed, info.depth, info.samples, info.held, info.locates) == (count, 0, 0, 0, 0, 0)
    for stale in (lambda: f.paths(), lambda: f.sample(), lambda: f.info):
        with pytest.raises(RuntimeError, match="no longer followed"):
            stale()
    assert lib.th_follow_sample(p._ctx, 0, 0.0) == INVALID and b"th_follow_sample:" in lib.th_last_error()
    status, _got, _times, guard, _gt, _info = raw_read(p, 63, 0, 1)
    assert status == INVALID and b"th_follow_read:" in lib.th_last_error()
    history, table = C.c_void_p(1), C.c_void_p(1)
    call("th_follow_query", p._ctx, None, C.byref(history), C.byref(table))
    assert history.value is None and table.value is None
    f.stop()                                                      # (ending twice is ending)
    again = p.follow(a_set(count, 65, 4), depth=1)                # ... and following starts over
    again.sample()
    same_rows(again.paths()[0][:, 0], ref[again.index])
    assert sorted_buffers(p) > 0
    t.dispose()


# ---- 6: read-only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_step_sample_draw_leaves_the_bits_of_step_draw(states, shape, view):
    st = moving(states[shape])
    a, b = tendrils(shape, view, st), tendrils(shape, view, st)
    f = a.follow(a_set(shape[0] * shape[1], 257, 11), depth=4)
    for frame in range(3):
        for t in (a, b):
            t.timer.tick()
            t.step()
        before = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]      # (the twin is read as well: both take the same calls but the samples)
        f.sample()
        f.sample(buffer=1)
        assert f.paths(last=2)[0].shape == (len(f), 2, 4)
        if frame == 1:
            f = a.follow(a_set(shape[0] * shape[1], 64, 12), depth=2)      # a new set between a step and its draw
            f.sample()
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
    assert f.info.locates > 0                                     # (the samples did go through the slot table)
    assert a.particles.stats(0.01) == b.particles.stats(0.01)          # (the respawned counter among them)
    assert bits_equal(a.flow.read(), b.flow.read()).all()
    assert (a.read_view() == b.read_view()).all() and a.read_view().any()
    for k in (0, 1):
        assert bits_equal(a.particles.read(k), b.particles.read(k)).all()
    a.dispose(); b.dispose()


# ---- 7: a row band -------------------------------------------------------------------------------------------------------------
def test_a_row_band_follows_its_rows_by_the_whole_textures_indices(states):
    shape, band = (100, 37), (25, 12)
    st = states[shape]
    rows = st[band[0]:band[0] + band[1]]
    base, count = band[0] * shape[0], band[1] * shape[0]
    p = context((shape[0], band[1]), rows, row0=band[0], global_height=shape[1])
    lib = _capi.load()
    index = (a_set(count, 65, 21).astype(np.int64) + base).astype(np.uint32)
    assert index[0] == base and index[-1] == base + count - 1
    f = p.follow(index, depth=2)
    f.sample()
    want = st.reshape(-1, 4)[index]                               # the whole texture's texels at the whole texture's indices
    assert live_of(want).any() and not live_of(want).all()
    same_rows(f.paths()[0][:, 0], want)
    assert f.info.particles == count
    # one index in the row above the band, one in the row below: refused, the position named
    above = np.concatenate([[base - 1], index]).astype(np.uint32)
    below = np.concatenate([index, [base + count]]).astype(np.uint32)
    for bad, position in ((above, 0), (below, len(below) - 1)):
        assert lib.th_follow_set(p._ctx, bad.ctypes.data_as(C.POINTER(C.c_uint32)), len(bad), 2) == INVALID
        message = lib.th_last_error()
        assert b"th_follow_set:" in message and b"position %d " % position in message and b"rows" in message, message
    local = a_set(count, 65, 21)                                  # the band's LOCAL texels are not what the call takes: 0 lies above the band
    assert lib.th_follow_set(p._ctx, local.ctypes.data_as(C.POINTER(C.c_uint32)), len(local), 2) == INVALID
    f.sample()                                                    # the set of before is still followed
    got = f.paths()[0]
    same_rows(got[:, 1], want)
    p.dispose()


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------
# (every refusal of the header but one: a context of more than 2^28 texels is 4 GiB of state a buffer - not a quick test's)
def test_every_bad_argument_is_refused_by_name_and_the_next_call_is_unaffected(states):
    shape = (100, 37)
    st = states[shape]
    count = shape[0] * shape[1]
    p = context(shape, st)
    lib, ctx = _capi.load(), p._ctx
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    good = a_set(count, 65, 5)
    gp = good.ctypes.data_as(u32p)
    info = _capi.FollowInfo()
    room = np.full((4, len(good), 4), GUARD, np.uint32)
    rp = room.ctypes.data_as(_capi._fp)

    def refused(status, entry, what):
        assert status == INVALID, what
        assert entry + b":" in lib.th_last_error(), (what, lib.th_last_error())

    # without a set
    refused(lib.th_follow_sample(ctx, 0, 0.0), b"th_follow_sample", "no set")
    refused(lib.th_follow_read(ctx, 0, 0, None, None, C.byref(info)), b"th_follow_read", "no set")
    # a null context
    refused(lib.th_follow_set(None, gp, len(good), 2), b"th_follow_set", "null context")
    refused(lib.th_follow_sample(None, 0, 0.0), b"th_follow_sample", "null context")
    refused(lib.th_follow_read(None, 0, 0, None, None, C.byref(info)), b"th_follow_read", "null context")
    refused(lib.th_follow_query(None, C.byref(info), None, None), b"th_follow_query", "null context")
    # the set
    big = np.arange(1025, dtype=np.uint32)
    equal, falling, outside = np.array(good), np.array(good), np.array(good)
    equal[7] = equal[6]
    falling[0], falling[1] = 5, 4
    outside[-1] = count
    bad_sets = [("null indices", None, 3, 2, None), ("n past the limit", gp, (1 << 20) + 1, 1, None), ("depth 0", gp, len(good), 0, None),
                ("depth past the limit", gp, len(good), (1 << 16) + 1, None), ("n * depth past the limit", big.ctypes.data_as(u32p), 1025, 1 << 14, None),
                ("an index equal to its predecessor", equal.ctypes.data_as(u32p), len(good), 2, b"position 7 "),
                ("a falling index", falling.ctypes.data_as(u32p), len(good), 2, b"position 1 "),
                ("an index past the texture", outside.ctypes.data_as(u32p), len(good), 2, b"position %d " % (len(good) - 1))]
    for what, pointer, n, depth, names in bad_sets:
        refused(lib.th_follow_set(ctx, pointer, n, depth), b"th_follow_set", what)
        assert names is None or names in lib.th_last_error(), (what, lib.th_last_error())
        call("th_follow_query", ctx, C.byref(info), None, None)
        assert info.followed == 0, what                           # nothing was reserved or changed
    # with a set: the sample and the read
    f = p.follow(good, depth=3)
    f.sample(time=1.0)
    for buffer in (-1, 2):
        refused(lib.th_follow_sample(ctx, buffer, 0.0), b"th_follow_sample", "buffer %d" % buffer)
    refused(lib.th_follow_read(ctx, 0, 1, rp, None, None), b"th_follow_read", "null info")
    refused(lib.th_follow_read(ctx, 0, 1, None, None, C.byref(info)), b"th_follow_read", "null states")
    for first, n in ((0, 2), (1, 1), (1 << 63, 1), (0, (1 << 64) - 1)):
        refused(lib.th_follow_read(ctx, first, n, rp, None, C.byref(info)), b"th_follow_read", "range [%d, +%d)" % (first, n))
    for what, pointer, n, depth, _names in bad_sets:              # ... and a refused set leaves this one followed
        refused(lib.th_follow_set(ctx, pointer, n, depth), b"th_follow_set", what)
    assert (room == GUARD).all()
    assert counters(f) == (1, 1, 0) and f.info.followed == len(good)
    # the valid calls after all of that are the ones they would have been
    f.sample(time=2.0)
    got, times = f.paths()
    assert list(times) == [1.0, 2.0]
    want = st.reshape(-1, 4)[good]
    same_rows(got[:, 0], want); same_rows(got[:, 1], want)
    with pytest.raises(ValueError):
        p.follow([], depth=2)
    with pytest.raises(_capi.TendrilsHipError):
        p.follow([3, 2, 1])
    assert f.info.followed == len(good)
    p.dispose()


# ---- 9: the device addresses ---------------------------------------------------------------------------------------------------
def test_query_hands_out_the_history_and_the_slot_table_and_launches_nothing(states):
    shape, view = SORTED_SHAPES[0]
    t = tendrils(shape, view, moving(states[shape]))
    p = t.particles
    step_until_sorted(t)
    index = t.select(box=BOX).index
    n, depth = len(index), 3
    assert 0 < n < shape[0] * shape[1]
    f = t.follow(index, depth=depth)
    info, history, table = _capi.FollowInfo(), C.c_void_p(), C.c_void_p()
    call("th_follow_query", p._ctx, C.byref(info), C.byref(history), C.byref(table))
    assert history.value and table.value is None                  # no table before the first sample of sorted slots
    assert (info.particles, info.followed, info.depth, info.samples, info.held, info.locates) == (shape[0] * shape[1], n, depth, 0, 0, 0)
    for k in range(5):
        t.timer.tick()
        t.step()
        f.sample(time=float(k))
    addresses = (C.c_void_p(), C.c_void_p())
    call("th_follow_query", p._ctx, C.byref(info), C.byref(addresses[0]), C.byref(addresses[1]))
    assert addresses[0].value == history.value and addresses[1].value       # valid until the next th_follow_set
    assert (info.samples, info.held) == (5, 3) and info.locates >= 1
    call("th_follow_query", p._ctx, None, None, None)             # (every pointer may be null)
    p.sync()
    rows = sharding.device_view(addresses[0].value, (depth, n, 4), "<f4").cpu().numpy()
    slots = sharding.device_view(addresses[1].value, (n,), "<u4").cpu().numpy()
    got, times = f.read(2, 3)
    assert list(times) == [2.0, 3.0, 4.0]
    for k in (2, 3, 4):
        same_rows(rows[k % depth], got[k - 2])                    # row k % depth holds sample k
        assert (rows[k % depth].view(np.uint32) == np.ascontiguousarray(got[k - 2]).view(np.uint32)).all()
    same_rows(got[2], everyone(p, 0)[index])
    is_sorted, perm, _slots = slot_order_read(p, 0)
    assert is_sorted and (perm[slots] == index).all()             # the table of the order the last sample read
    t.dispose()
