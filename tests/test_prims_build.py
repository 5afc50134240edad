"""CPU side of the primitives' tests: the harness (tests/native/) cross-compiles, exports its thp_ entry points and nothing
else, and holds the launchers of the SHIPPED object (lib/obj/th_sort.o); no product library carries a thp_ symbol.  And the
numpy references of tests/prims.py on hand-made inputs whose answers are written out here, so that a wrong reference
cannot agree with a wrong kernel by construction."""
import os
import re
import subprocess

import numpy as np
import pytest

import prims

ROOT = prims.ROOT
LIBS = [os.path.join(ROOT, "tendrils_amd", "lib", "libtendrils_hip.so"),
        os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")]


def nm(path, *flags):
    return subprocess.run(["nm", "-C"] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def harness():
    import __graft_entry__ as g
    if not all(os.path.exists(p) for p in LIBS + [prims.SORT_OBJECT]):
        g.build()
    return prims.build()


def test_harness_exports_exactly_its_entry_points(harness):
    dynamic = re.findall(r"^[0-9a-f]+ (\w) (.+)$", nm(harness, "-D", "--defined-only"), flags=re.M)
    assert sorted(name for _, name in dynamic) == prims.ENTRY_POINTS and {kind for kind, _ in dynamic} == {"T"}


def test_harness_holds_the_shipped_sort_object(harness):
    """the launchers are defined inside the harness library (linked from lib/obj/th_sort.o: tests/native/Makefile names no
    other source of them), and the harness source holds no kernel of the sort or the scan"""
    defined = nm(harness, "--defined-only")
    for launcher in ("th::launch_exclusive_scan_u32(", "th::launch_texel_set_rank(", "th::launch_radix_sort_u32(", "th::launch_radix_sort_u64(",
                     "th::exclusive_scan_sum_words(", "th::radix_sort_temp_bytes("):
        assert re.search(r"^[0-9a-f]+ [Tt] %s" % re.escape(launcher), defined, flags=re.M), launcher
    in_object = nm(prims.SORT_OBJECT, "--defined-only")
    assert re.search(r"^[0-9a-f]+ T th::launch_exclusive_scan_u32\(", in_object, flags=re.M)
    makefile = open(os.path.join(prims.NATIVE, "Makefile")).read()
    assert "lib/obj/th_sort.o" in makefile and "th_sort.hip" not in re.sub(r"#.*", "", makefile)
    source = open(os.path.join(prims.NATIVE, "prims_harness.hip")).read()
    assert "sort_scan_" not in source and "radix_scatter" not in source and "radix_hist" not in source and "texel_set_c" not in source


def test_no_product_library_exports_a_harness_symbol(harness):
    for lib in LIBS:
        assert "thp_" not in nm(lib, "-D"), lib


# ---- the references, on inputs small enough to do by hand -----------------------------------------------------------------
def test_scan_reference_by_hand():
    assert prims.scan_reference([3, 0, 1, 4]).tolist() == [0, 3, 3, 4]
    assert prims.scan_reference([7]).tolist() == [0]
    # the running sum passes 2^32: 0xfffffffe + 3 = 2^32 + 1 -> 1
    assert prims.scan_reference([0xfffffffe, 3, 5, 0xffffffff, 1]).tolist() == [0, 0xfffffffe, 1, 6, 5]
    out = prims.scan_reference([0xfffffffe, 3])
    assert out.dtype == np.uint32


def test_texel_set_reference_by_hand():
    # texels 0, 3 and 63 | none | texel 128 + 36 = 164 alone: 3, 0, 1 members, so 0, 3, 3 before the words
    before, members = prims.texel_set_reference(np.array([(1 << 63) | 0b1001, 0, 1 << 36], np.uint64))
    assert before.tolist() == [0, 3, 3] and before.dtype == np.uint32 and members == 4
    before, members = prims.texel_set_reference(np.array([0xffffffffffffffff, 0xfffffffff], np.uint64))      # 100 texels, all members
    assert before.tolist() == [0, 64] and members == 100
    before, members = prims.texel_set_reference(np.zeros(1, np.uint64))
    assert before.tolist() == [0] and members == 0


def test_block_scan_reference_by_hand():
    v = np.array([[1, 2, 3, 4], [0, 0, 0, 9]], np.uint32)
    before, total = prims.block_scan_reference(v)
    assert before.tolist() == [[0, 1, 3, 6], [0, 0, 0, 0]] and total.tolist() == [10, 9]
    big = np.array([[2 ** 33, 2 ** 32 + 1, 5]], np.uint64)         # a truncation to 32 bits would give 0, 1, 5
    before, total = prims.block_scan_reference(big)
    assert before.tolist() == [[0, 2 ** 33, 3 * 2 ** 32 + 1]] and total.tolist() == [3 * 2 ** 32 + 6]
    wrap = np.array([[0xffffffff, 2, 1]], np.uint32)
    before, total = prims.block_scan_reference(wrap)
    assert before.tolist() == [[0, 0xffffffff, 1]] and total.tolist() == [2]


def test_sort_reference_ten_elements_with_ties():
    # digits = bits [4, 8): the low nibble is outside the range and must neither order nor change
    keys = np.array([0x3a, 0x11, 0x3f, 0x20, 0x15, 0x30, 0x2c, 0x10, 0x31, 0x2b], np.uint32)
    #     digit        3     1     3     2     1     3     2     1     3     2
    k, v = prims.sort_reference(keys, None, 4, 8)
    assert v.tolist() == [1, 4, 7, 3, 6, 9, 0, 2, 5, 8]
    assert k.tolist() == [0x11, 0x15, 0x10, 0x20, 0x2c, 0x2b, 0x3a, 0x3f, 0x30, 0x31]
    vals = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108, 109], np.uint32)
    k2, v2 = prims.sort_reference(keys, vals, 4, 8)
    assert k2.tolist() == k.tolist() and v2.tolist() == [101, 104, 107, 103, 106, 109, 100, 102, 105, 108]
    # u64, one bit high up: bit 33
    keys64 = np.array([1 << 33, 5, (1 << 33) | 7, 9, 1 << 40], np.uint64)
    k3, v3 = prims.sort_reference(keys64, None, 33, 34)
    assert v3.tolist() == [1, 3, 4, 0, 2] and k3.tolist() == [5, 9, 1 << 40, 1 << 33, (1 << 33) | 7]
    # the whole 64 bits (a mask of 2^64 - 1)
    k4, v4 = prims.sort_reference(np.array([1 << 63, 3, (1 << 63) | 1, 3], np.uint64), None, 0, 64)
    assert v4.tolist() == [1, 3, 0, 2]


def test_sort_passes_of_the_ranges_the_product_uses():
    assert [prims.sort_passes(*r) for r in [(0, 1), (0, 7), (0, 8), (0, 11), (0, 21), (0, 32), (32, 53), (56, 59), (32, 56), (0, 64),
                                            (5, 6)]] == [1, 1, 1, 2, 3, 4, 3, 1, 3, 8, 1]


def test_stats_reference_twelve_texels_one_of_each_class():
    f32 = np.float32
    limit = f32(0.01)
    cap = f32(limit * f32(1.0 - 2.0 ** -20))
    assert cap == f32(0.00999999) and f32(0.0099999) < cap < np.nextafter(cap, f32(1)) < limit      # (2^-20 is some ten float32 steps)
    nan, inf = f32(np.nan), f32(np.inf)
    st = np.array([
        [-1e6, -1e6, 0, 0],                        # 0  inert
        [-1e6, -1e6, nan, 0],                      # 1  inert, NaN velocity: nan, not live
        [nan, 0.5, 0.001, 0],                      # 2  NaN x: live (a NaN differs from -1e6), nan, not finite
        [0.5, 0.5, 0, nan],                        # 3  NaN w: live, nan
        [0.5, 0.5, inf, 0],                        # 4  infinite velocity: live, not nan, not finite: neither capped nor summed
        [0.5, 0.5, 2e19, 2e19],                    # 5  z*z overflows float32: the same
        [0.1, 0.2, cap, 0],                        # 6  exactly at the cap: capped
        [0.1, 0.2, 0, np.nextafter(cap, f32(0))],  # 7  one ulp below: not capped
        [0.1, 0.2, np.nextafter(cap, f32(1)), 0],  # 8  one ulp above: capped
        [0.1, 0.2, 1e-42, 0],                      # 9  denormal velocity: its square is 0, speed 0
        [0.1, 0.2, 0, 0],                          # 10 at rest
        [-1e6, 0.3, 0.003, 0.004],                 # 11 x alone inert: live
    ], f32)
    got = prims.stats_reference(st, limit)
    speeds = [float(cap), float(np.nextafter(cap, f32(0))), float(np.nextafter(cap, f32(1))), 0.0, 0.0,
              float(np.sqrt(f32(0.003) * f32(0.003) + f32(0.004) * f32(0.004)))]
    assert got["particles"] == 12 and got["live"] == 10 and got["nan"] == 3 and got["capped"] == 2
    assert got["max_speed"] == float(np.nextafter(cap, f32(1)))
    assert abs(got["sum_speed"] - sum(speeds)) <= 1e-15
    # another limit moves `capped` only: 0.005 <= the speed of texel 11 and of 6, 7, 8
    other = prims.stats_reference(st, 0.005)
    assert other["capped"] == 4 and {k: v for k, v in other.items() if k != "capped"} == {k: v for k, v in got.items() if k != "capped"}
    # no finite particle at all
    none = prims.stats_reference(st[:6], limit)
    assert none["max_speed"] == 0.0 and none["sum_speed"] == 0.0 and none["capped"] == 0 and none["live"] == 4 and none["nan"] == 3


def test_crafted_states_of_the_gpu_tests_hold_what_they_say():
    """tests/test_gpu_statistics.py's generator states its counts from how it was built; the reference must find the same"""
    from test_gpu_statistics import LIMIT, crafted_state
    for n in (10, 50, 333):
        st, known = crafted_state(n, LIMIT, 5)
        want = prims.stats_reference(st, LIMIT)
        assert {k: want[k] for k in known} == known
        assert prims.stats_reference(st, LIMIT / 4)["capped"] > want["capped"]


def test_assert_counters_names_the_wrong_counter():
    want = dict(particles=4, live=3, nan=1, capped=1, sum_speed=1.0, max_speed=0.5)
    prims.assert_counters(dict(want, sum_speed=1.0 + 2.0 ** -52), want, "case")        # 2 ulp of 1: inside 4 * 2^-53
    with pytest.raises(AssertionError, match="capped = 2, reference 1"):
        prims.assert_counters(dict(want, capped=2), want, "case")
    with pytest.raises(AssertionError, match="sum_speed"):
        prims.assert_counters(dict(want, sum_speed=1.0 + 2.0 ** -50), want, "case")
