"""The packed-state codec without a GPU: the numpy mirror of helpers.py - the reference of every packed GPU test - held against
the exact reference of packed_codec_cases.py on every value and word of its sets, bit for bit; the exact reference itself held
against the definition (a nearest binary16, ties to the even mantissa; a nearest quantum); monotone, idempotent, clear of the
sentinel; and the two position formulas of th_packed.inc side by side - pack-then-unpack against the fused carry's closed form -
which agree everywhere in value and part in the bits exactly where the closed form gives -0.0.

The sets are built once for the module and never written."""
import numpy as np
import pytest

import packed_codec_cases as cases
from helpers import bits_equal, pack_state, unpack_state

F = np.float32


@pytest.fixture(scope="module")
def sets():
    out = dict(velocity=cases.velocity_values(), position=cases.position_values(), words=cases.raw_words(),
               full=cases.full_texels(), special=cases.special_texels())
    for v in out.values():
        v.setflags(write=False)
    return out


def as_texels(pos=None, vel=None):
    """a value set as [n, 4] texels: in x and (opposite order) y, or in z and (opposite order) w"""
    v = pos if pos is not None else vel
    st = np.zeros((len(v), 4), F)
    st[:, 0 if pos is not None else 2], st[:, 1 if pos is not None else 3] = v, v[::-1]
    return st


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def test_the_sets_hold_every_boundary(sets):
    assert len(cases.velocity_values(distinct=False)) >= 507920 and len(cases.position_values(distinct=False)) >= 196627
    vel, pos = sets["velocity"], sets["position"]

    def holds(v, x):
        x = np.atleast_1d(np.asarray(x, F))
        return np.isin(x.view(np.uint32), v.view(np.uint32)).all()
    h = np.arange(0x7c00)
    every_half = h.astype(np.uint16).view(np.float16).astype(F)       # (the decode side: numpy's own binary16)
    assert holds(vel, every_half) and holds(vel, -every_half)
    mid = (every_half[:-1].astype(np.float64) + every_half[1:]) / 2
    for v in (mid, np.nextafter(mid.astype(F), F(np.inf)), np.nextafter(mid.astype(F), F(-np.inf))):
        assert holds(vel, v) and holds(vel, -v.astype(F))
    assert holds(vel, [65504, 65520, np.nextafter(F(65520), F(0)), np.nextafter(F(65520), F(np.inf)), 1e30, np.inf, -np.inf,
                       2.0 ** -25, np.nextafter(F(2.0 ** -25), F(1)), 2.0 ** -24, 2.0 ** -149, -2.0 ** -149, 0.0, -0.0])
    assert np.isnan(vel).any()
    k = np.arange(-32769, 32769)
    tie = ((k + 0.5) / 16384).astype(F)
    assert holds(pos, tie) and holds(pos, np.nextafter(tie, F(np.inf))) and holds(pos, np.nextafter(tie, F(-np.inf)))
    assert holds(pos, [0.0, -0.0, 1e-6, -1e-6, -1e-30, 2.5, -2.5, np.inf, -np.inf, 1e30, -1e30, -1e6,
                       np.nextafter(F(-1e6), F(0)), np.nextafter(F(-1e6), F(-np.inf))])
    assert len(np.unique(vel.view(np.uint32))) == len(vel) and len(np.unique(pos.view(np.uint32))) == len(pos)
    # every pairing that meets a sentinel
    pairs = cases.PAIRINGS
    inert = (pairs == F(-1e6)).all(-1)
    assert inert.sum() == 1 and ((pairs == F(-1e6)).any(-1) & ~inert & ~np.isnan(pairs).any(-1)).sum() >= 2
    assert np.isnan(pairs[:, 0]).any() and np.isnan(pairs[:, 1]).any() and ((pairs[:, 0] == F(-1e6)) & np.isnan(pairs[:, 1])).any()
    # the full state holds every value in each of its four components
    full = sets["full"]
    for c, v in ((0, pos), (1, pos), (2, vel), (3, vel)):
        assert holds(np.ascontiguousarray(full[:, c]), v), c


def test_the_words_hold_every_pattern_in_every_half(sets):
    w = sets["words"].astype(np.int64)
    for half in (w[:, 0] & 0xffff, w[:, 0] >> 16, w[:, 1] & 0xffff, w[:, 1] >> 16):
        assert len(np.unique(half)) == 0x10000
    xs, ys = w[:, 0] & 0xffff, w[:, 0] >> 16
    assert len(np.unique(ys[xs == 0x8000])) == 0x10000                    # the NaN sentinel beside anything; inert among them
    assert ((xs != 0x8000) & (ys == 0x8000)).any()                        # a word pack_state never writes


def test_the_layout_is_the_smallest_odd_one(sets):
    for n in (len(sets["full"]), len(sets["words"]), 1500):
        w, h = cases.shape_for(n)
        assert w % 64 != 0 and (w * h) % 256 != 0 and w * h >= n and (h - 2) * w < n and w * h <= 1000 * 256
    st = cases.lay_out(sets["special"], (50, 30))
    assert st.shape == (30, 50, 4) and bits_equal(st.reshape(-1, 4)[:len(sets["special"])], sets["special"]).all()
    assert (st.reshape(-1, 4)[len(sets["special"]):] == np.array([-1e6, -1e6, 0, 0], F)).all()
    words = cases.lay_out_words(sets["words"])
    assert (words.reshape(-1, 2)[len(sets["words"]):] == (0x80008000, 0)).all()


# ---- the exact reference against the definition ------------------------------------------------------------------------------------------
def test_the_reference_half_is_a_nearest_half_with_ties_to_even(sets):
    v = sets["velocity"]
    got = cases.encode_half(v).astype(np.int64)
    nan = np.isnan(v)
    assert cases.half_is_nan(got[nan]).all() and not cases.half_is_nan(got[~nan]).any()
    assert ((got[nan] >> 15) == (v[nan].view(np.uint32) >> 31)).all()
    v, got = v[~nan], got[~nan]
    assert ((got >> 15) == (v.view(np.uint32) >> 31)).all()                # the sign, of a zero too
    mag, a = got & 0x7fff, np.abs(v).astype(np.float64)
    # the finite halves in order, and 2^16 where the next one would be: rounding treats the range as unbounded, then 2^16 is infinity
    table = np.append(np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64), 65536.0)
    lo = np.clip(np.searchsorted(table, a, side="right") - 1, 0, 0x7c00 - 1)
    below, above = a - table[lo], table[lo + 1] - a
    want = np.where(below < above, lo, np.where(above < below, lo + 1, lo + (lo & 1)))      # a tie: the even one of the two
    want = np.where(a >= 65536.0, 0x7c00, want)
    assert (mag == want).all(), int((mag != want).sum())
    assert ((mag == 0x7c00) == (a >= 65520.0)).all()                       # the overflow threshold
    assert (mag[a <= 2.0 ** -25] == 0).all() and (mag[(a > 2.0 ** -25) & (a <= 2.0 ** -24)] == 1).all()
    # decode is numpy's own binary16 on every pattern, and encode its inverse
    h = np.arange(0x10000, dtype=np.uint16)
    assert bits_equal(cases.decode_half(h), h.view(np.float16).astype(F)).all()
    keep = ~cases.half_is_nan(h)
    assert (cases.encode_half(cases.decode_half(h[keep])) == h[keep]).all()


def test_the_reference_position_is_the_nearest_quantum_with_ties_to_even(sets):
    x = sets["position"]
    q = cases.encode_position(x)
    assert (np.abs(q) <= 32767).all()
    scaled = np.clip(x.astype(np.float64) * 16384, -32767, 32767)          # exact in float64
    floor = np.floor(scaled)
    frac = scaled - floor
    want = np.where(frac < 0.5, floor, np.where(frac > 0.5, floor + 1, floor + (floor.astype(np.int64) & 1)))
    assert (q == want).all(), int((q != want).sum())
    assert (frac == 0.5).sum() >= 65534 and set(np.unique(q)) == set(range(-32767, 32768))


# ---- the mirror against the exact reference ----------------------------------------------------------------------------------------------
def test_the_mirror_encodes_every_value_as_the_exact_reference(sets):
    with np.errstate(all="ignore"):
        for name, st in (("velocity", as_texels(vel=sets["velocity"])), ("position", as_texels(pos=sets["position"])),
                         ("full", sets["full"])):
            got, want = pack_state(st), cases.encode(st)
            same = cases.words_equal(got, want)
            assert same.all(), (name, int((~same).sum()), st[~same][:4])


def test_the_mirror_decodes_every_word_as_the_exact_reference(sets):
    words = sets["words"]
    got, want = unpack_state(words), cases.decode(words)
    same = bits_equal(got, want).all(-1)
    assert same.all(), (int((~same).sum()), words[~same][:4])
    xs, ys = (words[:, 0] & 0xffff).astype(np.int64), (words[:, 0] >> 16).astype(np.int64)
    nan, inert = (xs == 0x8000) & (ys != 0x8000), (xs == 0x8000) & (ys == 0x8000)
    assert np.isnan(want[nan, :2]).all() and (want[inert, :2] == F(-1e6)).all() and inert.sum() >= 1
    odd = (xs != 0x8000) & (ys == 0x8000)
    assert (want[odd, 1] == F(-2.0)).all() and not np.isnan(want[odd, 0]).any()
    # and what the mirror encodes, it decodes as the reference does
    with np.errstate(all="ignore"):
        assert bits_equal(unpack_state(pack_state(sets["full"])), cases.quantised(sets["full"])).all()


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_encode_is_monotone_over_the_sorted_finite_values(sets):
    pos = np.sort(sets["position"][np.isfinite(sets["position"])])
    assert (np.diff(cases.encode_position(pos)) >= 0).all()
    vel = np.sort(sets["velocity"][np.isfinite(sets["velocity"])])
    dec = cases.decode_half(cases.encode_half(vel)).astype(np.float64)
    assert (dec[1:] >= dec[:-1]).all()                                     # (as values: -inf .. inf, -0 = +0)
    # the words of whole texels too, through the state encoder
    st = as_texels(pos=pos)
    xs = (cases.encode(st)[:, 0] & 0xffff).astype(np.uint16).view(np.int16)
    assert (np.diff(xs.astype(np.int64)) >= 0).all()


def test_decode_of_encode_is_idempotent(sets):
    q = cases.quantised(sets["full"])
    again = cases.quantised(q)
    assert bits_equal(again, q).all()
    assert (cases.encode(q) == cases.encode(sets["full"])).all()           # (the NaN halves too: one quiet NaN per sign)
    assert (~bits_equal(q, sets["full"])).any()


def test_every_encoded_position_is_clear_of_the_sentinel(sets):
    st = sets["full"]
    w0 = cases.encode(st)[:, 0].astype(np.int64)
    xs = (w0 & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)
    ys = (w0 >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    inert = (st[:, 0] == F(-1e6)) & (st[:, 1] == F(-1e6))
    nan = np.isnan(st[:, :2]).any(-1) & ~inert
    assert inert.any() and nan.any()
    assert (xs[inert] == -32768).all() and (ys[inert] == -32768).all()
    assert (xs[nan] == -32768).all() and (ys[nan] == 0).all()
    live = ~inert & ~nan
    assert (np.abs(xs[live]) <= 32767).all() and (np.abs(ys[live]) <= 32767).all()
    assert (xs[live] == 32767).any() and (xs[live] == -32767).any()


def test_probe_results_are_fixed_points_of_the_codec(sets):
    st = cases.quantised(sets["full"])
    for c in range(4):
        p = cases.probe(st, c)
        assert bits_equal(cases.quantised(p), p).all(), c
        # and they tell every bit: the component's bits come back out of the probe
        b = (np.rint(p[:, 0].astype(np.float64) * 16384).astype(np.int64) | (np.rint(p[:, 1].astype(np.float64) * 16384).astype(np.int64) << 15)
             | (p[:, 2].astype(np.int64) << 30))
        v = np.ascontiguousarray(st[:, c])
        assert (b == np.where(np.isnan(v), cases.NAN_CODE, v.view(np.uint32).astype(np.int64))).all(), c


# ---- the two formulas of th_packed.inc ---------------------------------------------------------------------------------------------------
def test_the_closed_form_and_pack_then_unpack_part_only_at_negative_zero(sets):
    """quantize_state's position was rint(clamp(x * 16384)) * 2^-14; the stored path is unpack_state(pack_state(x)), through a
    short.  In value the two agree everywhere.  In the bits they part exactly where the closed form gives -0.0 - the negative
    inputs of magnitude up to half a quantum, where the short is 0 and decodes to +0.0: in the position set -0.0, -1e-30, -1e-6,
    the tie -2^-15 and its neighbour towards zero.  The device's quantize_state must follow the stored path - +0.0 - since
    that is what the next step reads when it runs unfused (tests/test_gpu_packed_codec.py holds it to that)."""
    x = sets["position"]
    x = x[~np.isnan(x)]
    with np.errstate(all="ignore"):
        closed = (np.rint(np.clip(x * F(16384), F(-32767), F(32767))) * F(2.0 ** -14)).astype(F)
    stored = (cases.encode_position(x) / 16384.0).astype(F)
    assert (closed == stored).all()
    apart = ~bits_equal(closed, stored)
    assert (closed[apart].view(np.uint32) == 0x80000000).all() and (stored[apart].view(np.uint32) == 0).all()
    assert (apart == (closed.view(np.uint32) == 0x80000000)).all()
    assert (apart == cases.negative_zero_positions(x)).all()
    named = np.array([-0.0, -1e-30, -1e-6, -2.0 ** -15, np.nextafter(F(-2.0 ** -15), F(0))], F)
    assert sorted(x[apart].view(np.uint32).tolist()) == sorted(named.view(np.uint32).tolist())
    # the repair - scaling back as fma(q, 2^-14, +0.0): the product is exact in float64, the sum takes -0.0 to +0.0, one rounding
    # to fp32 - closes the gap and changes nothing else; so does adding +0.0 before the product
    with np.errstate(all="ignore"):
        q = np.rint(np.clip(x * F(16384), F(-32767), F(32767)))
    assert bits_equal((q.astype(np.float64) * 2.0 ** -14 + 0.0).astype(F), stored).all()
    assert bits_equal(((q + F(0.0)) * F(2.0 ** -14)).astype(F), stored).all()
