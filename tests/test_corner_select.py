"""The facts the stage-y corner selects, the folded falloff clamp and the folded z mask of the noise's table path rest on
(th_logic.hpp: snoise_corners_tab, snoise_finish), in numpy with every operation rounded to fp32 as the
device rounds it:

  1. for all eight values of the three order compares, picking q1 / q2 from the two pairs B[a0], B[a0 + 4] and B[a1],
     B[a1 + 4] after the reads names the table word that reading at sel + e named; i1.z implies !i1.y and !i2.z implies i2.y;
  2. on the real tables (permA / permB and winA / winB), for every a0, a1 the chain can produce and all eight mask values,
     q0 .. q3 are the old chain's, and the pair reads stay inside the tables: the largest index read is a + 4, the one the
     old chain already read as a1 + 4;
  3. med3(x, 0, 1) == max(x, 0) bit for bit on x = fl(0.6 - d), d a sum of squares;
  4. the low 16 bits of bits(r + 2^21) are 4 * r for every r the window's z index takes."""
import itertools

import numpy as np

from test_hash_window import BIAS_A, BIAS_B, K_LUT_MIN, ORIGINS, WIN_A, WIN_B, bias_bits, permute_int, tables

f32 = np.float32
u32 = np.uint32
PERM_A, PERM_B = 292, 584                       # th_logic.hpp: kPermA, kPermB
MASKS = list(itertools.product((False, True), repeat=3))


def order_masks(l1, l2, l3):
    """the order block of snoise_corners_tab: (my1, mz1, my2, mz2) = (i1.y, i1.z, i2.y, i2.z)"""
    return l1 & ~l2, l2 & ~l3, l1 | ~l2, l2 | ~l3


def test_the_masks_pick_the_word_that_sel_plus_e_named():
    for l1, l2, l3 in MASKS:
        my1, mz1, my2, mz2 = (bool(m) for m in order_masks(np.bool_(l1), np.bool_(l2), np.bool_(l3)))
        assert not (mz1 and my1), (l1, l2, l3)
        assert mz2 or my2, (l1, l2, l3)
        # a word's name: (which first-stage sum, byte step)
        old1 = ("a1" if mz1 else "a0", 4 if my1 else 0)
        old2 = ("a1" if mz2 else "a0", 4 if my2 else 0)
        u0, u1, w0, w1 = ("a0", 0), ("a0", 4), ("a1", 0), ("a1", 4)
        new1 = w0 if mz1 else (u1 if my1 else u0)
        new2 = (w1 if my2 else w0) if mz2 else u1
        assert new1 == old1 and new2 == old2, (l1, l2, l3)
    # i1 has at most one component set, i2 at least two
    for l1, l2, l3 in MASKS:
        l = [np.bool_(v) for v in (l1, l2, l3)]
        i1 = [l[2] & ~l[0], l[0] & ~l[1], l[1] & ~l[2]]
        i2 = [l[2] | ~l[0], l[0] | ~l[1], l[1] | ~l[2]]
        assert sum(map(bool, i1)) <= 1 and sum(map(bool, i2)) >= 2


def plain_tables():
    """hash_tables_kernel: every entry of both tables from permute_int itself"""
    pa = (4 * permute_int(np.arange(PERM_A)).astype(np.int64) - BIAS_A).astype(u32)
    pb = (16 * (permute_int(np.arange(PERM_B)).astype(np.int64) - K_LUT_MIN) - BIAS_B).astype(u32)
    return pa, pb


def old_chain(B, a0, a1, masks):
    my1, mz1, my2, mz2 = masks
    sel1, sel2 = (a1 if mz1 else a0), (a1 if mz2 else a0)
    e1y, e2y = u32(4 if my1 else 0), u32(4 if my2 else 0)
    idx = [a0 // 4, (sel1 + e1y) // 4, (sel2 + e2y) // 4, (a1 + u32(4)) // 4]
    return [B[i] for i in idx], max(int(i.max()) for i in idx), int((a1 // 4 + 1).max())


def new_chain(B, a0, a1, masks):
    my1, mz1, my2, mz2 = masks
    i0, i1 = a0 // 4, a1 // 4
    read = [i0, i0 + 1, i1, i1 + 1]
    assert min(int(i.min()) for i in read) >= 0 and max(int(i.max()) for i in read) < len(B), "a pair read leaves the table"
    u0, u1, w0, w1 = (B[i] for i in read)
    q1 = w0 if mz1 else (u1 if my1 else u0)
    q2 = (w1 if my2 else w0) if mz2 else u1
    return [u0, q1, q2, w1], max(int(i.max()) for i in read)


def check_tables(A, B, a_args, y_args):
    """every first-stage argument z (entries z and z + 1 of A) against every second coordinate"""
    z, ry = (g.ravel() for g in np.meshgrid(a_args, y_args, indexing="ij"))
    yb = bias_bits(ry, 2.0 ** 21)
    a0, a1 = A[z] + yb, A[z + 1] + yb                       # uint32: the sums wrap as the device's do
    assert (a0 % 4 == 0).all() and (a1 % 4 == 0).all() and int(a1.max()) + 4 < 4 * len(B)
    for l in MASKS:
        masks = tuple(bool(m) for m in order_masks(*(np.bool_(v) for v in l)))
        old, old_top, q3_top = old_chain(B, a0, a1, masks)
        new, new_top = new_chain(B, a0, a1, masks)
        for k, (o, n) in enumerate(zip(old, new)):
            assert np.array_equal(o, n), "q%d, compares %s" % (k, l)
        assert new_top == q3_top == old_top, "the largest index read is the old chain's a1 + 4"


def test_plain_tables_every_argument_and_mask():
    A, B = plain_tables()
    # mod289_int returns an integer in [0, 289] (tests/test_gpu_hash_chain.py asserts 289 occurs)
    check_tables(A, B, np.arange(0, 290), np.arange(0, 290))
    assert 290 + 1 < PERM_A and 288 + 289 + 1 < PERM_B


def test_window_tables_every_argument_and_mask():
    A, B, _ = tables()
    assert len(A) == WIN_A and len(B) == WIN_B
    # i - c in [0, 577] on every axis (tests/test_hash_window.py), + 1 for the far z corner
    check_tables(A, B, np.arange(0, 578), np.arange(0, 578))
    assert 577 + 1 < WIN_A and 288 + 577 + 1 < WIN_B


def med3(x, lo, hi):
    """the median of three, without assuming where x lies"""
    return np.sort(np.stack([x, np.full_like(x, lo), np.full_like(x, hi)]), axis=0)[1]


def test_falloff_med3_is_max_bit_for_bit():
    c = f32(0.6)
    near = (c.view(u32) + np.arange(-64, 65, dtype=np.int64)).astype(u32).view(f32)      # every d within 64 ulp of 0.6
    d = np.concatenate([np.linspace(0.0, 4.0, (1 << 22) + 1, dtype=np.float64).astype(f32), near,
                        np.array([0.0, np.inf], f32)])
    assert (d >= 0).all() and near.min() < c < near.max() and len(np.unique(near)) == 129
    x = c - d                                               # fp32: one rounding, as v_sub_f32
    assert x.dtype == f32 and x.max() == c and c < f32(1.0)
    assert not (np.signbit(x) & (x == 0)).any()             # 0.6 - 0.6 is +0: no negative zero to tell the two forms apart
    a, b = med3(x, f32(0), f32(1)), np.maximum(x, f32(0))
    assert np.array_equal(a.view(u32), b.view(u32))
    assert b[-1] == 0 and b[-2] == c                        # d = +inf, d = 0
    assert (b[d > c] == 0).all() and (b[d < c] > 0).all()


def test_bias_low_word_is_the_offset():
    r = np.arange(0, 580)
    assert np.array_equal(bias_bits(r, 2.0 ** 21) & u32(0xffff), (4 * r).astype(u32))
    assert 4 * 579 < 1 << 16
    # with the window's origin in the constant, as the kernel adds it: bits(iz + (2^21 - cz))
    for cz in ORIGINS:
        assert float(f32(2.0 ** 21 - cz)) == 2.0 ** 21 - cz
        low = bias_bits(cz + r, 2.0 ** 21 - cz) & u32(0xffff)
        assert np.array_equal(low, (4 * r).astype(u32)), cz
        assert np.array_equal(low, bias_bits(cz + r, 2.0 ** 21 - cz) & u32(0xffc))       # what the mask gave
