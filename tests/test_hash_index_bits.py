"""The bit identities the fused integrator's hash index chain rests on (th_logic.hpp: snoise_corners_tab).

mod289_int() returns an exact integer r in [0, 289].  Added to 2^21 (one ulp = 1/4) or 2^19 (one ulp = 1/16) as a float,
r sits in the mantissa already shifted to a byte offset: no float -> int conversion and no shift.  The constant high bits
are taken off by the LDS tables' own entries (hash_tables_kernel), in 32-bit wrap-around arithmetic."""
import numpy as np

BIAS_A, BITS_A = np.float32(2097152.0), np.uint32(0x4A000000)      # 2^21: r << 2, offsets into permA (4-byte entries)
BIAS_B, BITS_B = np.float32(524288.0), np.uint32(0x49000000)       # 2^19: r << 4, offsets into the gradient table (16-byte)
K_LUT_MIN = -2                                                     # th_math.hpp: kLutMin

R = np.arange(0, 290, dtype=np.uint32)                             # every value mod289_int can return (289 included)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def permute_int(x):
    """th_math.hpp: permute_int on exact small integers"""
    x = np.asarray(x, np.int64)
    return ((34 * x + 1) * x) % 289


def test_bias_identities_for_every_mod289_result():
    rf = R.astype(np.float32)
    assert np.array_equal(bits(rf + BIAS_A), BITS_A + (R << np.uint32(2)))
    assert np.array_equal(bits(rf + BIAS_B), BITS_B + (R << np.uint32(4)))
    assert np.array_equal(bits(rf + BIAS_A) & np.uint32(0xffc), R << np.uint32(2))
    assert int((R << np.uint32(4)).max()) == 4624 < 2 ** 23                      # stays inside the mantissa


def test_negative_zero_is_offset_zero():
    z = np.float32(-0.0)
    assert bits(z + BIAS_A) == BITS_A and bits(z + BIAS_B) == BITS_B
    assert bits(z + BIAS_A) & np.uint32(0xffc) == 0


def test_wraparound_sums_of_the_y_stage():
    """permA[k] = 4 * permute_int(k) - 0x4A000000 (mod 2^32); + bits(r + 2^21) = 4 * (p + r): the byte offset into permB."""
    p = permute_int(np.arange(0, 291))                                           # stage z reads permA[iz], permA[iz + 1]
    assert p.min() >= 0 and p.max() <= 288
    ent = (np.uint32(4) * p.astype(np.uint32) - BITS_A).astype(np.uint32)        # uint32 arithmetic wraps
    yb = bits(R.astype(np.float32) + BIAS_A)
    got = (ent[:, None] + yb[None, :]).astype(np.uint32)
    want = (4 * (p[:, None] + R.astype(np.int64)[None, :])).astype(np.uint32)
    assert np.array_equal(got, want)
    for e in (0, 4):                                                             # the y step of a corner: one entry more
        assert np.array_equal((got + np.uint32(e)).astype(np.uint32), want + np.uint32(e))
    assert int(want.max()) + 4 < 4 * 584                                         # inside permB (kPermB entries)


def test_wraparound_sums_of_the_x_stage():
    """permB[k] = 16 * (permute_int(k) - kLutMin) - 0x49000000; + bits(r + 2^19) = 16 * (p + r - kLutMin): the byte
    offset of the gradient entry."""
    p = permute_int(np.arange(0, 581))                                           # stage y arguments: p + r + {0, 1} <= 579
    ent = (np.uint32(16) * (p - K_LUT_MIN).astype(np.uint32) - BITS_B).astype(np.uint32)
    xb = bits(R.astype(np.float32) + BIAS_B)
    got = (ent[:, None] + xb[None, :]).astype(np.uint32)
    want = (16 * (p[:, None] + R.astype(np.int64)[None, :] - K_LUT_MIN)).astype(np.uint32)
    assert np.array_equal(got, want)
    for e in (0, 16):
        assert np.array_equal((got + np.uint32(e)).astype(np.uint32), want + np.uint32(e))
    assert int(want.max()) + 16 < 16 * 584                                       # inside the gradient table (kLutSize entries)
