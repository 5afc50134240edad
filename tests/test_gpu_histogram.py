"""The histogram on the GPU (include/tendrils_hip.h "histogram"; tendrils_amd/csrc/th_histogram.hip): the particles of a ring
buffer that match select's clauses, counted per bin of one scalar of the state, and the exact order statistics radix select
builds from its key mode (Particles.quantiles).  The reference is numpy over the state in texel order - what was uploaded,
Particles.read(), or for packed rings the numpy codec of tests/helpers.py - evaluating the header's expressions in np.float32;
never the code under test (the key of a float is restated here, not imported).  Every accumulation of the library is an integer
addition, so all comparisons are exact, whatever order the ring is held in, and every call asserts the invariant
below + sum(counts) + above + nan == matched.

Shapes: 5 x 3 (15 of 64 lanes: one partial wave), 100 x 37 (3 700 slots: four blocks of 1 024, the last one ragged), and
1024 x 1025: a lane takes FOUR slots a turn, a workgroup 1 024, and the grid is capped at 1 024 workgroups, so a workgroup
takes a second turn of its loop from 1 048 577 slots on; 1024 x 1025 = 1 049 600 is the first whole row past that - workgroup 0
goes round twice, its second block a ragged one.  SORTED_SHAPES give tile-sorted slots.  Every clause set is non-trivial ON THE
NUMPY REFERENCE - 0 < matched < live < particles - unless the case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tendrils_amd import _capi, sharding
from tendrils_amd._capi import call
from tendrils_amd.particles import Histogram

from helpers import bits_equal, pack_state, unpack_state
from test_gpu_measure_program import SORTED_SHAPES, context, slot_order_read, sorted_buffers, step_until_sorted, tendrils
from test_gpu_select import BOX, CLAUSES, matching, spread_state

pytestmark = pytest.mark.gpu

F = np.float32
INERT = F(-1e6)
SHAPES = [(5, 3), (100, 37), (1024, 1025)]
SEEDS = {(5, 3): 36, (100, 37): 131, (1024, 1025): 2077, (48, 48): 79}
CHANNELS = ["x", "y", "vx", "vy", "speed2", "speed"]
BINS = [1, 7, 257, 1000, 4096]
CLAMPING = [(-1.0, 1.0, 4096), (-0.75, 0.875, 1000), (-1.2, 1.2, 257)]      # the last float below hi lands in bin `bins` before the min
# a range per channel that leaves particles of spread_state on both sides (positions to about +-1.2, velocities to about +-3)
RANGES = dict(x=(-1.0, 1.0), y=(-0.75, 0.875), vx=(-1.2, 1.2), vy=(-2.5, 2.0), speed2=(0.5, 9.0), speed=(0.25, 3.5))
INFO = ("particles", "live", "matched", "below", "above", "nan")
GUARD = 0xA5A5A5A5
PASSES = ((2048, 21), (2048, 10), (1024, 0))


# ---- the reference -------------------------------------------------------------------------------------------------------------
def key_of(v):
    """the header's key of float32 values: (u >> 31) ? ~u : (u | 0x80000000)"""
    u = np.ascontiguousarray(v, F).view(np.uint32)
    return np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float_of(key):
    key = np.asarray(key, np.uint32)
    return np.where((key >> np.uint32(31)) != 0, key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(F)


class Reference:
    """numpy over one state in texel order; the masks of a clause set and the channels' values are computed once"""

    def __init__(self, st, row0=0):
        self.st, self.row0 = np.asarray(st, F), row0
        s = self.st.reshape(-1, 4)
        with np.errstate(over="ignore", invalid="ignore"):
            q = (s[:, 2] * s[:, 2]) + (s[:, 3] * s[:, 3])
            assert q.dtype == F
            self.values = dict(x=s[:, 0], y=s[:, 1], vx=s[:, 2], vy=s[:, 3], speed2=q, speed=np.sqrt(q))
        assert self.values["speed"].dtype == F
        self.masks = {}

    def matched(self, clauses):
        name = repr(sorted(clauses.items()))
        if name not in self.masks:
            m, live, _index = matching(self.st, row0=self.row0, **clauses)
            self.masks[name] = (m, int(live.sum()))
        return self.masks[name]

    def counters(self, channel, clauses):
        m, live = self.matched(clauses)
        v = self.values[channel][m]
        nan = np.isnan(v)
        return v[~nan], dict(particles=self.st.shape[0] * self.st.shape[1], live=live, matched=int(m.sum()), nan=int(nan.sum()))

    def linear(self, channel, bins, lo, hi, **clauses):
        v, out = self.counters(channel, clauses)
        lo, hi = F(lo), F(hi)
        scale = F(bins) / (hi - lo)
        assert isinstance(scale, F)
        below, above = v < lo, v >= hi
        mid = v[~below & ~above]
        b = np.floor((mid - lo) * scale)
        assert b.dtype == F
        b = b.astype(np.int64)
        assert (b >= 0).all() and (b <= bins).all()
        out.update(below=int(below.sum()), above=int(above.sum()), counts=np.bincount(np.minimum(b, bins - 1), minlength=bins),
                   unclamped=int(b.max()) if b.size else -1)
        return out

    def key(self, channel, bins, shift, prefix, **clauses):
        v, out = self.counters(channel, clauses)
        key = key_of(v).astype(np.uint64)
        top = np.uint64(shift + bins.bit_length() - 1)
        head, want = key >> top, np.uint64(prefix) >> top
        out.update(below=int((head < want).sum()), above=int((head > want).sum()),
                   counts=np.bincount(((key[head == want] >> np.uint64(shift)) & np.uint64(bins - 1)).astype(np.int64), minlength=bins))
        return out

    def ordered(self, channel, **clauses):
        """the matched, non-NaN values in ascending key order"""
        v, _ = self.counters(channel, clauses)
        return float_of(np.sort(key_of(v)))


def nontrivial(want):
    return 0 < want["matched"] < want["live"] < want["particles"]


def same(got, want):
    """a Histogram (or (counts, th_histogram_info)) against the reference's dict, exactly - and the invariant"""
    counts, info = (got.counts, got) if isinstance(got, Histogram) else got
    have = {k: int(getattr(info, k)) for k in INFO}
    assert have == {k: want[k] for k in INFO}, (have, {k: want[k] for k in INFO})
    assert counts.dtype == np.uint32 and counts.shape == want["counts"].shape
    wrong = np.flatnonzero(counts != want["counts"])
    assert not wrong.size, (wrong[:4], counts[wrong[:4]], want["counts"][wrong[:4]])
    assert have["below"] + int(counts.sum(dtype=np.int64)) + have["above"] + have["nan"] == have["matched"]
    return want


def uniforms(channel=_capi.HIST_VX, mode=_capi.HIST_LINEAR, bins=16, lo=-1.0, hi=1.0, prefix=0, shift=0, reserved=0, **select):
    u = _capi.HistogramUniforms()
    u.select.stride, u.select.phase = select.get("stride", 1), select.get("phase", 0)
    u.select.flags, u.select.reserved = select.get("flags", 0), select.get("select_reserved", 0)
    if "box" in select:
        u.select.flags |= _capi.SELECT_BOX
        u.select.box[:] = select["box"]
    if "speed2" in select:
        u.select.flags |= _capi.SELECT_SPEED
        u.select.speed2[:] = select["speed2"]
    u.channel, u.mode, u.bins, u.lo, u.hi, u.key_prefix, u.key_shift, u.reserved = channel, mode, bins, lo, hi, prefix, shift, reserved
    return u


def raw_histogram(p, u, room=None, buffer=0):
    """th_histogram into `room` words (bins + 3 by default) filled with GUARD: (the words, th_histogram_info)"""
    out = np.full(u.bins + 3 if room is None else room, GUARD, np.uint32)
    info = _capi.HistogramInfo()
    call("th_histogram", p._ctx, C.byref(u), buffer, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info))
    return out, info


def key_pass(p, channel, bins, shift, prefix, **clauses):
    """one TH_HIST_KEY pass through the host's own route (Particles._key_pass): (counts, th_histogram_info)"""
    counts, info = p._key_pass(channel, bins, shift, prefix, clauses)
    return counts.astype(np.uint32), info


@pytest.fixture(scope="module")
def states():
    out = {}
    for (w, h), seed in SEEDS.items():
        st = spread_state(w, h, seed)
        st.setflags(write=False)
        out[(w, h)] = st
    return out


@pytest.fixture(scope="module")
def references(states):
    return {shape: Reference(st) for shape, st in states.items()}


# ---- 1, 2: every channel, both modes, every bin count, with and without clauses, at every shape --------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_channel_mode_and_bin_count_gives_numpys_counts(states, references, shape):
    st, ref = states[shape], references[shape]
    p = context(shape, st)
    for clauses in ({}, CLAUSES["all"]):
        assert not clauses or nontrivial(ref.counters("x", clauses)[1])
        for channel in CHANNELS:
            lo, hi = RANGES[channel]
            for bins in BINS:
                want = same(p.histogram(channel, bins, (lo, hi), **clauses), ref.linear(channel, bins, lo, hi, **clauses))
                if shape != (5, 3) and not clauses:
                    assert want["below"] > 0 and want["above"] > 0 and (want["counts"] > 0).sum() >= min(bins, 3), (channel, bins)
            # the three passes of a radix select towards the reference's median, and a pass whose bins reach bit 32 from lower down
            ordered = ref.ordered(channel, **clauses)
            median = int(key_of(ordered[len(ordered) // 2:len(ordered) // 2 + 1])[0])
            for bins, shift in PASSES + ((4096, 20), (1, 32), (1, 0)):
                want = same(key_pass(p, channel, bins, shift, median, **clauses), ref.key(channel, bins, shift, median, **clauses))
                assert want["counts"].sum() > 0
    same(p.histogram("x", 7, (-2e6, 2.0), inert=True), ref.linear("x", 7, -2e6, 2.0, inert=True))      # the inert ones: one bin of their own
    assert ref.linear("x", 7, -2e6, 2.0, inert=True)["matched"] == shape[0] * shape[1]
    assert bits_equal(p.read(0), st).all()                        # (the ring is as it was)
    p.dispose()


# ---- 3: values planted on every boundary, linear bins --------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,bins", CLAMPING)
def test_planted_boundary_values_fall_on_their_side_and_the_clamp_is_live(states, lo, hi, bins):
    shape = (100, 37)
    st = np.array(states[shape])
    flat = st.reshape(-1, 4)
    lo32, hi32 = F(lo), F(hi)
    under_hi = np.nextafter(hi32, F(-np.inf))
    planted = np.array([lo32, np.nextafter(lo32, F(-np.inf)), hi32, under_hi, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-40], F)
    at = 1000
    flat[at:at + len(planted), 2] = planted                       # s.z of live particles (1 in 7 of them inert: matched only under `inert`)
    flat[at:at + len(planted), 3] = F(0.0)
    flat[at:at + len(planted), :2] = F(0.25)
    ref = Reference(st)
    scale = F(bins) / (hi32 - lo32)
    assert int(np.floor((under_hi - lo32) * scale)) == bins      # the clamp decides where this one goes
    p = context(shape, st)
    want = same(p.histogram("vx", bins, (lo, hi)), ref.linear("vx", bins, lo, hi))
    assert want["unclamped"] == bins and want["nan"] == 1
    # each planted value alone (a box around nobody else would do; a stride picks exactly its texel)
    sides = []
    for k, v in enumerate(planted):
        clauses = dict(stride=3700, phase=at + k)
        one = same(p.histogram("vx", bins, (lo, hi), **clauses), ref.linear("vx", bins, lo, hi, **clauses))
        assert one["matched"] == 1
        sides.append("nan" if one["nan"] else "below" if one["below"] else "above" if one["above"] else int(np.flatnonzero(one["counts"])[0]))
    zero_bin = int(np.floor((F(0.0) - lo32) * scale))
    assert sides == [0, "below", "above", bins - 1, "above", "below", "nan", zero_bin, zero_bin, zero_bin, zero_bin], sides
    # the same values as a POSITION: live particles whatever they hold
    flat[at:at + len(planted), 0] = planted
    ref = Reference(st)
    p.upload_texels(st, 0)
    same(p.histogram("x", bins, (lo, hi)), ref.linear("x", bins, lo, hi))
    p.dispose()


# ---- 4: planted values, key bins -----------------------------------------------------------------------------------------------
def test_planted_values_in_key_mode_order_like_the_floats(states):
    shape = (100, 37)
    st = np.array(states[shape])
    flat = st.reshape(-1, 4)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001], np.uint32).view(F)
    planted = np.concatenate([np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf], F), nans])
    at = 2000
    flat[at:at + len(planted), 2] = planted
    flat[at:at + len(planted), :2] = F(0.25)
    ref = Reference(st)
    keys = key_of(planted[:8]).astype(np.int64)
    in_order = np.array([-np.inf, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 1e-40, np.inf], F)
    assert keys[0] + 1 == keys[1] == 0x80000000 and (planted[:8][np.argsort(keys)].view(np.uint32) == in_order.view(np.uint32)).all()
    p = context(shape, st)
    # key_shift + d == 32: no prefix takes part, every non-NaN value has a bin
    for bins, shift in ((2048, 21), (4096, 20), (1, 32), (2, 31)):
        want = same(key_pass(p, "vx", bins, shift, 0xdeadbeef), ref.key("vx", bins, shift, 0xdeadbeef))
        assert want["below"] == want["above"] == 0 and want["nan"] == 4 and want["counts"].sum() == want["matched"] - 4
    # the prefix of +0.0: the negative values (-0.0 among them) below, +0.0 and the positive denormals inside, the rest above
    zero = 0x80000000
    for bins, shift in ((2048, 10), (1024, 0), (1, 0), (8, 3)):
        want = same(key_pass(p, "vx", bins, shift, zero), ref.key("vx", bins, shift, zero))
        assert want["below"] > 0 and want["above"] > 0 and want["counts"].sum() > 0 and want["nan"] == 4, (bins, shift)
    # each planted value alone, last pass under its own prefix: its own bin - or, a NaN, none
    for k, v in enumerate(planted):
        clauses = dict(stride=3700, phase=at + k)
        prefix = int(key_of(v.reshape(1))[0])
        one = same(key_pass(p, "vx", 1024, 0, prefix, **clauses), ref.key("vx", 1024, 0, prefix, **clauses))
        assert one["matched"] == 1 and one["nan"] == (1 if k >= 8 else 0) and one["below"] == one["above"] == 0
        assert k >= 8 or one["counts"][prefix & 1023] == 1
    # the planted particles alone (nobody else sits on exactly this position): their eight values come out in the floats' order,
    # -0.0 below +0.0, the four NaNs taking no part
    alone = dict(box=(0.25, 0.25, float(np.nextafter(F(0.25), F(1))), float(np.nextafter(F(0.25), F(1)))))
    assert ref.counters("vx", alone)[1]["matched"] == 12 and ref.counters("vx", alone)[1]["nan"] == 4
    got = p.quantiles("vx", [k / 8.0 for k in range(8)], **alone)
    assert (got.view(np.uint32) == in_order.view(np.uint32)).all(), got
    p.dispose()


# ---- 5: skew -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(100, 37), (1024, 1025)], ids=lambda s: "%dx%d" % s)
def test_every_particle_in_one_bin_and_two_alternating_values(states, shape):
    st = np.array(states[shape])
    st[..., 2], st[..., 3] = F(0.6), F(0.8)                       # one speed: every live particle in one bin
    ref = Reference(st)
    p = context(shape, st)
    for channel, (lo, hi) in (("speed", (0.0, 2.0)), ("speed2", (0.0, 2.0)), ("vx", (-1.0, 1.0))):
        for bins in (1024, 4096, 7):
            want = same(p.histogram(channel, bins, (lo, hi)), ref.linear(channel, bins, lo, hi))
            assert want["counts"].max() == want["matched"] == want["live"] > 0 and (want["counts"] > 0).sum() == 1
    want = same(key_pass(p, "speed", 2048, 21, 0), ref.key("speed", 2048, 21, 0))
    assert want["counts"].max() == want["live"]
    assert bits_equal(p.quantiles("speed", [0.0, 0.5, 1.0]), ref.ordered("speed")[[0, 0, 0]]).all()
    flat = st.reshape(-1, 4)
    flat[1::2, 2], flat[1::2, 3] = F(-0.3), F(0.4)                # two values, alternating lane by lane
    ref = Reference(st)
    p.upload_texels(st, 0)
    for channel, (lo, hi) in (("speed", (0.0, 2.0)), ("vx", (-1.0, 1.0))):
        want = same(p.histogram(channel, 1024, (lo, hi)), ref.linear(channel, 1024, lo, hi))
        assert (want["counts"] > 0).sum() == 2 and want["counts"].sum() == want["live"]
    p.dispose()


# ---- 6: tile-sorted slots, f32 and packed; a packed ring in texel order ---------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_tile_sorted_slots_give_the_counts_of_texel_order_and_stay_sorted(states, shape, view, fmt):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)                    # (velocities the integrator keeps: about +-0.01)
    t = tendrils(shape, view, st, fmt)
    p = t.particles
    step_until_sorted(t)
    assert sorted_buffers(p) > 0
    is_sorted, perm_before, slots_before = slot_order_read(p, 0, fmt == "f16")
    assert is_sorted and not (perm_before == np.arange(perm_before.size)).all()
    texels = np.zeros_like(slots_before)
    texels[perm_before] = slots_before
    back = (unpack_state(texels) if fmt == "f16" else texels.view(F)).reshape(shape[1], shape[0], 4)
    ref = Reference(back)
    top = float(ref.ordered("speed")[-1])
    ranges = dict(x=(-1.0, 1.0), y=(-0.75, 0.875), vx=(-0.5 * top, 0.5 * top), vy=(-0.5 * top, 0.25 * top), speed2=(0.0, 0.5 * top * top), speed=(0.0, top))
    picks = [{}, dict(stride=3, phase=1), dict(box=BOX, stride=2, phase=1), dict(box=BOX), dict(stride=5, phase=3, inert=True)]
    got = [(kw, ch, p.histogram(ch, 257, ranges[ch], **kw), key_pass(p, ch, 2048, 21, 0, **kw), p.quantiles(ch, [0.0, 0.5, 0.95, 1.0], **kw))
           for kw in picks for ch in CHANNELS]
    forwarded = (t.histogram("speed", 64, ranges["speed"], box=BOX), t.quantiles("speed", 0.5, box=BOX))      # Tendrils.*: buffers[0]
    again, perm_after, slots_after = slot_order_read(p, 0, fmt == "f16")
    assert again and (perm_after == perm_before).all() and (slots_after == slots_before).all()
    assert sorted_buffers(p) > 0
    for kw, ch, hist, keyed, quants in got:
        want = same(hist, ref.linear(ch, 257, *ranges[ch], **kw))
        assert want["counts"].sum() > 0 and (nontrivial(want) or not kw or kw.get("inert")), (kw, ch)
        same(keyed, ref.key(ch, 2048, 21, 0, **kw))
        assert bits_equal(quants, quantiles_of(ref.ordered(ch, **kw), [0.0, 0.5, 0.95, 1.0])).all(), (kw, ch)
    same(forwarded[0], ref.linear("speed", 64, *ranges["speed"], box=BOX))
    assert bits_equal(forwarded[1], quantiles_of(ref.ordered("speed", box=BOX), [0.5])[0])
    other = p.histogram("x", 257, ranges["x"], stride=3, phase=1, buffer=1)       # the other buffer, in whatever order it is held
    assert bits_equal(p.read(0), back).all()                      # (texel order: from here on the ring is no longer sorted)
    same(other, Reference(p.read(1)).linear("x", 257, *ranges["x"], stride=3, phase=1))
    same(p.histogram("speed", 257, ranges["speed"], stride=3, phase=1), ref.linear("speed", 257, *ranges["speed"], stride=3, phase=1))
    t.dispose()


def quantiles_of(ordered, qs):
    n = len(ordered)
    return ordered[[min(int(np.floor(q * n)), n - 1) for q in qs]]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_packed_ring_in_texel_order(states, shape):
    st = states[shape]
    p = context(shape, st, packed=True)
    decoded = unpack_state(pack_state(st))                        # what the 8-byte texels hold, by the numpy mirror of the codec
    assert not bits_equal(decoded, st).all()
    ref = Reference(decoded)
    for clauses in ({}, CLAUSES["all"]):
        assert not clauses or nontrivial(ref.counters("x", clauses)[1])
        for channel in CHANNELS:
            same(p.histogram(channel, 1000, RANGES[channel], **clauses), ref.linear(channel, 1000, *RANGES[channel], **clauses))
            same(key_pass(p, channel, 2048, 21, 0, **clauses), ref.key(channel, 2048, 21, 0, **clauses))
    assert bits_equal(p.quantiles("speed", [0.25, 0.5], **CLAUSES["all"]), quantiles_of(ref.ordered("speed", **CLAUSES["all"]), [0.25, 0.5])).all()
    p.dispose()


# ---- 7: read-only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_step_histogram_quantiles_draw_leaves_the_bits_of_step_draw(states, shape, view):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)
    a, b = tendrils(shape, view, st), tendrils(shape, view, st)
    for frame in range(3):
        for t in (a, b):
            t.timer.tick()
            t.step()
        before = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]      # (the twin is read as well: both take the same calls but these)
        assert a.histogram("speed", 1024, (0.0, 0.02)).matched > 0
        assert a.quantiles("speed", [0.5, 0.95], box=BOX) is not None
        a.particles.histogram("x", 7, (-1.0, 1.0), stride=3, phase=2, buffer=1)
        a.particles.histogram_async("vy", 4096, (-0.01, 0.01), box=BOX, inert=True)
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


# ---- 8: a row band -------------------------------------------------------------------------------------------------------------
def test_a_row_band_counts_its_rows_and_strides_over_the_whole_textures_indices(states):
    shape, band = (100, 37), (25, 12)
    st = states[shape]
    rows = st[band[0]:band[0] + band[1]]
    p = context((shape[0], band[1]), rows, row0=band[0], global_height=shape[1])
    ref, local = Reference(rows, row0=band[0]), Reference(rows)
    for clauses in (dict(stride=7, phase=3), dict(box=BOX, speed=(1.0, 3.5), stride=3, phase=1), dict(box=BOX, stride=3, phase=0)):
        want = ref.linear("vx", 257, -1.2, 1.2, **clauses)
        assert nontrivial(want)
        # (2 500 texels lie in front of this band, no multiple of 7 or 3: the band's own indices would choose other particles)
        assert not (want["counts"] == local.linear("vx", 257, -1.2, 1.2, **clauses)["counts"]).all()
        same(p.histogram("vx", 257, (-1.2, 1.2), **clauses), want)
        assert bits_equal(p.quantiles("vx", [0.25, 0.5], **clauses), quantiles_of(ref.ordered("vx", **clauses), [0.25, 0.5])).all()
    p.dispose()


# ---- 9: quantiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3), (100, 37), (1024, 1025)], ids=lambda s: "%dx%d" % s)
def test_quantiles_are_the_elements_of_the_sorted_reference_bit_for_bit(states, shape):
    st = np.array(states[shape])
    flat = st.reshape(-1, 4)
    planted = 2 if shape == (5, 3) else 5
    flat[:planted, 2] = F(np.nan)                                 # matched NaNs (vx, and so both speeds): excluded from n
    flat[:planted, :2] = F(0.25)
    ref = Reference(st)
    p = context(shape, st)
    qs = [0.0, 0.25, 0.5, 0.95, 1.0]
    for clauses in ({}, dict(box=(-1.0, -1.0, 1.0, 1.0), stride=2, phase=1)):
        assert not clauses or nontrivial(ref.counters("x", clauses)[1])
        for channel in CHANNELS:
            ordered = ref.ordered(channel, **clauses)
            _values, counters = ref.counters(channel, clauses)
            assert len(ordered) == counters["matched"] - counters["nan"] > 0
            assert (counters["nan"] > 0) == (channel in ("vx", "speed2", "speed"))
            got = p.quantiles(channel, qs, **clauses)
            assert got.dtype == F and got.shape == (5,)
            want = quantiles_of(ordered, qs)
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (channel, got, want)
            assert want[0] == ordered.min() and want[-1] == ordered.max()
    assert ref.counters("vx", {})[1]["nan"] == planted
    one = p.quantiles("speed", 0.5)
    assert isinstance(one, F) and one.view(np.uint32) == quantiles_of(ref.ordered("speed"), [0.5])[0].view(np.uint32)
    assert p.quantiles("speed", [0.5], box=(0.25, -2.0, 0.25, 2.0)) is None          # x0 == x1: nobody matches
    only_nans = dict(stride=len(flat), phase=0)                   # texel 0 alone: a NaN
    assert ref.counters("vx", only_nans)[1] == dict(particles=len(flat), live=ref.counters("vx", {})[1]["live"], matched=1, nan=1)
    assert p.quantiles("vx", 0.5, **only_nans) is None
    with pytest.raises(ValueError):
        p.quantiles("speed", 1.5)
    p.dispose()


# ---- 10: plumbing --------------------------------------------------------------------------------------------------------------
def test_async_leaves_the_synchronous_calls_bytes_on_the_device_and_null_counts_fill_the_info(states, references):
    shape = (100, 37)
    st, ref = states[shape], references[shape]
    p = context(shape, st)
    for channel, bins in (("speed", 1000), ("x", 4096), ("vy", 1)):
        lo, hi = RANGES[channel]
        want = ref.linear(channel, bins, lo, hi, **CLAUSES["box"])
        assert nontrivial(want)
        counts_at, info_at = p.histogram_async(channel, bins, (lo, hi), **CLAUSES["box"])
        assert counts_at and info_at
        p.sync()
        info = _capi.HistogramInfo.from_buffer_copy(sharding.device_view(info_at, (6,), "<u8").cpu().numpy().tobytes())
        counts = sharding.device_view(counts_at, (bins,), "<u4").cpu().numpy().astype(np.uint32)
        same((counts, info), want)
        same(p.histogram(channel, bins, (lo, hi), **CLAUSES["box"]), want)        # the synchronous call after it: the same
    lib = _capi.load()
    u = uniforms(channel=_capi.HIST_SPEED, bins=1000, lo=0.25, hi=3.5, box=BOX)
    assert lib.th_histogram_async(p._ctx, C.byref(u), 0, None, None) == _capi.TH_OK      # (both pointers may be null)
    p.sync()
    info = _capi.HistogramInfo()
    call("th_histogram", p._ctx, C.byref(u), 0, None, C.byref(info))                    # counts == NULL: the info alone
    want = ref.linear("speed", 1000, 0.25, 3.5, box=BOX)
    assert {k: int(getattr(info, k)) for k in INFO} == {k: want[k] for k in INFO}
    out, info = raw_histogram(p, u)
    same((out[:1000], info), want)
    assert (out[1000:] == GUARD).all()                            # past `bins` words: untouched
    p.dispose()


# ---- 11: refusals --------------------------------------------------------------------------------------------------------------
# (every refusal of the header but one: a context of more than 2^28 texels is 4 GiB of state a buffer - not a quick test's)
def test_every_bad_argument_is_refused_by_name_and_the_next_call_is_unaffected(states, references):
    shape = (5, 3)
    st, ref = states[shape], references[shape]
    p = context(shape, st)
    lib, ctx = _capi.load(), p._ctx
    nan, inf, big = float("nan"), float("inf"), 3.0e38
    K = _capi.HIST_KEY
    good = uniforms(bins=16, lo=-1.2, hi=1.2, box=BOX)
    bad = [("null uniforms", None, 0), ("buffer -1", good, -1), ("buffer 2", good, 2),
           # what th_select refuses about the embedded block
           ("stride 0", uniforms(stride=0), 0), ("phase == stride", uniforms(stride=3, phase=3), 0), ("select flag 8", uniforms(flags=8), 0),
           ("select reserved", uniforms(select_reserved=1), 0), ("box nan", uniforms(box=(nan, 0, 1, 1)), 0), ("speed2 nan", uniforms(speed2=(0.0, nan)), 0),
           ("channel -1", uniforms(channel=-1), 0), ("channel 6", uniforms(channel=6), 0), ("mode -1", uniforms(mode=-1), 0), ("mode 2", uniforms(mode=2), 0),
           ("bins 0", uniforms(bins=0), 0), ("bins 4097", uniforms(bins=4097), 0), ("bins 1 << 31", uniforms(bins=1 << 31), 0),
           ("key bins 0", uniforms(mode=K, bins=0), 0), ("key bins 8192", uniforms(mode=K, bins=8192), 0),
           ("lo nan", uniforms(lo=nan), 0), ("hi nan", uniforms(hi=nan), 0), ("lo -inf", uniforms(lo=-inf), 0), ("hi inf", uniforms(hi=inf), 0),
           ("lo == hi", uniforms(lo=0.5, hi=0.5), 0), ("lo > hi", uniforms(lo=1.0, hi=-1.0), 0),
           ("hi - lo infinite", uniforms(lo=-big, hi=big), 0), ("scale infinite", uniforms(bins=4096, lo=0.0, hi=1e-40), 0),
           ("key bins 7", uniforms(mode=K, bins=7), 0), ("key bins 1000", uniforms(mode=K, bins=1000), 0),
           ("key top 33", uniforms(mode=K, bins=2048, shift=22), 0), ("key shift 33", uniforms(mode=K, bins=1, shift=33), 0),
           ("key shift wraps", uniforms(mode=K, bins=2, shift=0xffffffff), 0),
           ("reserved", uniforms(reserved=1), 0), ("key reserved", uniforms(mode=K, reserved=7), 0)]
    out, info = np.full(4100, GUARD, np.uint32), _capi.HistogramInfo()
    counts_at, info_at = C.c_void_p(), C.c_void_p()
    for what, u, buffer in bad:
        arg = None if u is None else C.byref(u)
        assert lib.th_histogram(ctx, arg, buffer, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info)) == _capi.TH_ERR_INVALID, what
        assert b"th_histogram:" in lib.th_last_error(), (what, lib.th_last_error())
        assert lib.th_histogram_async(ctx, arg, buffer, C.byref(counts_at), C.byref(info_at)) == _capi.TH_ERR_INVALID, what
        assert b"th_histogram_async:" in lib.th_last_error(), (what, lib.th_last_error())
        assert (out == GUARD).all(), what
    counts = out.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.th_histogram(ctx, C.byref(good), 0, counts, None) == _capi.TH_ERR_INVALID and b"th_histogram:" in lib.th_last_error()
    assert lib.th_histogram(None, C.byref(good), 0, counts, C.byref(info)) == _capi.TH_ERR_INVALID and b"th_histogram:" in lib.th_last_error()
    assert lib.th_histogram_async(None, C.byref(good), 0, None, None) == _capi.TH_ERR_INVALID and b"th_histogram_async:" in lib.th_last_error()
    assert (out == GUARD).all()
    # what the OTHER mode reads is nobody's business: a NaN range under TH_HIST_KEY, a wild shift under TH_HIST_LINEAR
    idle = uniforms(mode=K, bins=2048, shift=21, lo=nan, hi=nan)
    got, info = raw_histogram(p, idle)
    same((got[:2048], info), ref.key("vx", 2048, 21, 0))
    idle = uniforms(bins=7, lo=-1.2, hi=1.2, shift=77, prefix=5)
    got, info = raw_histogram(p, idle)
    same((got[:7], info), ref.linear("vx", 7, -1.2, 1.2))
    assert (got[7:] == GUARD).all()
    # ... and the valid call after all of that is the one it would have been
    got, info = raw_histogram(p, good)
    want = same((got[:16], info), ref.linear("vx", 16, -1.2, 1.2, box=BOX))
    assert nontrivial(want) and (got[16:] == GUARD).all()
    p.dispose()
