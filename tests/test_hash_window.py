"""The three facts the windowed lattice hash of the fused integrator rests on (th_logic.hpp "over a window"),
in numpy with every operation rounded to fp32 as the device rounds it:

  1. mod289_int(i) is the true i mod 289 for every integer |i| <= 8958 and not beyond - the bound the host refuses a window at;
  2. permute_int(k) == permute_int(k mod 289) on [-2, 581], the arguments of the unwindowed tables, with values in [0, 288];
  3. the index chain over the periodically extended tables, fed with raw coordinates and bias constants that carry the
     window's origin, ends at the hash value of the reference chain - on every edge of a full-width window, in every corner
     combination, and on random cells - and never leaves the tables."""
import os
import re

import numpy as np

f32 = np.float32
KINV289 = f32(1.0) / f32(289.0)
K_LUT_MIN = -2
WIN_A, WIN_B, WIN_G = 580, 868, 868
BIAS_A, BIAS_B = 0x4A000000, 0x49000000
MAX_CELL = 8958
SPAN = 286


def mod289_int(x):
    """th_math.hpp: fma(-289, floor(x * (1/289)), x): the product rounded to fp32, the fma exact on these integers"""
    x = np.asarray(x, np.float64)
    q = np.floor(x.astype(f32) * KINV289)
    return x - 289.0 * q.astype(np.float64)


def permute_int(x):
    """th_math.hpp: t = fma(x, 34, 1) * x (an exact integer below 2^24 here), then fma(-289, floor(t * (1/289)), t)"""
    x = np.asarray(x, np.float64)
    t = (x * 34.0 + 1.0) * x
    assert np.abs(t).max() < 2.0 ** 24
    q = np.floor(t.astype(f32) * KINV289)
    return t - 289.0 * q.astype(np.float64)


def test_inv289_rounds_up():
    assert float(KINV289) > 1.0 / 289.0 and abs(float(KINV289) - 0.0034602077) < 1e-9


def test_mod289_int_is_the_true_residue_up_to_8958_and_not_at_8959():
    i = np.arange(-MAX_CELL, MAX_CELL + 1)
    assert np.array_equal(mod289_int(i), i % 289)
    beyond = np.array([-(MAX_CELL + 1), MAX_CELL + 1])
    assert (mod289_int(beyond) != beyond % 289).any()


def test_the_hosts_constants_are_these():
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "tendrils_amd", "csrc", "th_kernels.hpp")).read()
    assert int(re.search(r"kWinMaxCell\s*=\s*(\d+)", text).group(1)) <= MAX_CELL
    assert int(re.search(r"kWinSpan\s*=\s*(\d+)", text).group(1)) <= SPAN
    logic = open(os.path.join(here, "..", "tendrils_amd", "csrc", "th_logic.hpp")).read()
    sizes = re.search(r"kWinA\s*=\s*(\d+),\s*kWinB\s*=\s*(\d+),\s*kWinG\s*=\s*(\d+)", logic).groups()
    assert tuple(map(int, sizes)) == (WIN_A, WIN_B, WIN_G)


def test_permute_int_is_periodic_on_the_tables_arguments():
    k = np.arange(K_LUT_MIN, 582)
    p = permute_int(k)
    assert np.array_equal(p, permute_int(k % 289))
    assert p.min() >= 0 and p.max() <= 288
    assert np.array_equal(p, ((34 * k + 1) * k) % 289)


def tables():
    P = permute_int(np.arange(289)).astype(np.int64)
    win_a = (4 * P[np.arange(WIN_A) % 289] - BIAS_A).astype(np.uint32)          # wraps mod 2^32, as the device's uint32 does
    win_b = (16 * (P[np.arange(WIN_B) % 289] - K_LUT_MIN) - BIAS_B).astype(np.uint32)
    win_g = np.arange(WIN_G) % 289                                              # the argument whose gradient entry winG[k] holds
    return win_a, win_b, win_g


def bias_bits(i, k):
    """bits of fp32(i + k): the v_add_f32 of the chain"""
    return (np.asarray(i, f32) + f32(k)).view(np.uint32)


def windowed(ix, iy, iz, cxy, cz, ex, ey, ez):
    """snoise_corners_tab<.., WIN>: the hash argument whose gradient entry a corner reads, and the largest index into each table"""
    win_a, win_b, win_g = tables()
    kz, ky, kx = 2.0 ** 21 - cz, 2.0 ** 21 - cxy, 2.0 ** 19 - cxy
    for k in (kz, ky, kx):
        assert float(f32(k)) == k
    zb = bias_bits(iz, kz) & np.uint32(0xffc)
    yb, xb = bias_bits(iy, ky), bias_bits(ix, kx)
    u = zb // 4 + ez
    a = win_a[u] + yb + np.uint32(4) * ey.astype(np.uint32)
    assert (a % 4 == 0).all()
    j = a // 4
    q = win_b[j] + xb + np.uint32(16) * ex.astype(np.uint32)
    assert (q % 16 == 0).all()
    k = q.astype(np.int64) // 16 + K_LUT_MIN
    return win_g[k], (int(u.max()), int(j.max()), int(k.max())), (int(u.min()), int(j.min()), int(k.min()))


def reference(ix, iy, iz, ex, ey, ez):
    """the last permute of permute(permute(permute(mod289(iz) + ez) + mod289(iy) + ey) + mod289(ix) + ex)"""
    arg = permute_int(permute_int(mod289_int(iz) + ez) + mod289_int(iy) + ey) + mod289_int(ix) + ex
    assert arg.min() >= K_LUT_MIN and arg.max() <= 581
    return arg


ORIGINS = (-8670, -289, 0, 289, 1445, 8092)          # c + 577 + 1 stays within 8958 in magnitude


def compare(u_x, u_y, u_z, cxy, cz):
    corners = np.array(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")).reshape(3, -1)
    for ex, ey, ez in corners.T:
        e = [np.full(u_x.shape, v, np.int64) for v in (ex, ey, ez)]
        ix, iy, iz = cxy + u_x, cxy + u_y, cz + u_z
        assert max(np.abs(ix).max(), np.abs(iy).max(), np.abs(iz).max()) + 1 <= MAX_CELL
        k, hi, lo = windowed(ix, iy, iz, cxy, cz, *e)
        assert min(lo) >= 0 and hi[0] < WIN_A and hi[1] < WIN_B and hi[2] < WIN_G
        ref = reference(ix, iy, iz, *e)
        assert np.array_equal(permute_int(k), permute_int(ref)), "corner (%d, %d, %d), origins %d, %d" % (ex, ey, ez, cxy, cz)
        assert np.array_equal(k, ref % 289)


def test_windowed_chain_on_every_edge_of_a_full_width_window():
    edge = np.array([0, 1, 287, 288, 289, 576, 577])
    u_x, u_y, u_z = (g.ravel() for g in np.meshgrid(edge, edge, edge, indexing="ij"))
    for cxy, cz in list(zip(ORIGINS, ORIGINS[::-1])) + [(0, 0), (289, 289), (-8670, -8670), (8092, 8092)]:
        compare(u_x, u_y, u_z, cxy, cz)


def test_windowed_chain_on_random_cells():
    rng = np.random.default_rng(289)
    for cxy, cz in ((-8670, 8092), (289, 1445), (0, -289)):
        u_x, u_y, u_z = rng.integers(0, 578, (3, 1 << 17))
        compare(u_x, u_y, u_z, cxy, cz)


def test_a_window_of_the_widest_range_stays_inside_the_tables():
    """the host: c = 289 * floor(lo / 289) and hi - lo <= 286, so i - c <= 288 + 286, + 1 for the far corner"""
    top = 288 + SPAN + 1
    assert top <= 577 and top + 1 <= WIN_A - 1
    assert 288 + top <= WIN_B - 1 and 288 + top <= WIN_G - 1
