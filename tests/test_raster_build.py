"""CPU side of the line rasteriser's tests: the harness (tests/native/raster_harness.hip) cross-compiles for gfx950, exports
its thr_ entry points and nothing else, and holds no span routine of its own; no product library carries a thr_ symbol.  And
the references of tests/raster.py on polygons worked through by hand here, so that a wrong reference cannot agree with a
wrong kernel by construction."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster

ROOT = raster.ROOT
LIBS = [os.path.join(ROOT, "tendrils_amd", "lib", "libtendrils_hip.so"),
        os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")]
ROUTINES = ["dep_raster_poly", "dep_raster_small_hexagon", "dep_raster_small_hexagon2", "dep_hexagon_row_span", "dep_hexagon_is_small",
            "tri_span", "dep_param", "dep_setup", "dep_ceil_div"]


def nm(path, *flags):
    return subprocess.run(["nm", "-C"] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def harness():
    import __graft_entry__ as g
    if not all(os.path.exists(p) for p in LIBS):
        g.build()
    return raster.build()


def test_harness_cross_compiles_for_gfx950(harness):
    blob = open(harness, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"spans_kernel" in blob and b"param_kernel" in blob


def test_harness_exports_exactly_its_entry_points(harness):
    dynamic = re.findall(r"^[0-9a-f]+ (\w) (.+)$", nm(harness, "-D", "--defined-only"), flags=re.M)
    assert sorted(name for _, name in dynamic) == raster.ENTRY_POINTS and {kind for kind, _ in dynamic} == {"T"}


def test_harness_holds_no_span_routine_of_its_own():
    """every routine is named only as a call into namespace th (th::name), the header they live in is included, and none of
    the ways they divide appears in the harness's code"""
    source = open(os.path.join(raster.NATIVE, "raster_harness.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert '#include "th_raster.hpp"' in code
    for name in ROUTINES:
        for m in re.finditer(r"\b%s\b" % name, code):
            assert code[max(0, m.start() - 4):m.start()] == "th::", (name, code[max(0, m.start() - 40):m.end() + 20])
    for name in ("dep_raster_poly<6>", "dep_raster_poly<0>", "dep_raster_small_hexagon(", "dep_raster_small_hexagon2(", "dep_hexagon_row_span(",
                 "tri_span(", "dep_param(", "dep_hexagon_is_small(", "dep_setup<"):
        assert "th::" + name in code, name
    for word in ("rcpf", "__mul24", "floorf", "__builtin_floor", "% ", "/ (16", "/ den"):
        assert word not in code, word
    makefile = re.sub(r"#.*", "", open(os.path.join(raster.NATIVE, "Makefile")).read())
    assert "libth_raster.so" in makefile and "raster_exports.map" in makefile and "-ffp-contract=off" in makefile
    assert re.search(r"^all:.*\$\(RASTER\)", makefile, flags=re.M)


def test_no_product_library_exports_a_harness_symbol(harness):
    for lib in LIBS:
        assert "thr_" not in nm(lib, "-D"), lib


# ---- the rule, on polygons small enough to do by hand -----------------------------------------------------------------------
def test_width_one_hexagon_of_a_horizontal_line():
    """Texel centres (2, 3) -> (5, 3): endpoints (32, 48), (80, 48), half-diamond 8, dx > dy and dx > -dy: L0 T0 T1 R1 B1 B0.
    edge 0 (24,48) -> (32,56) up:    rows ceil(48/16) = 3 <= y < ceil(56/16) = 4; y = 3: (8 * 0 + 24 * 8) / (16 * 8) = 192/128 -> left 2
    edge 1 (32,56) -> (80,56):       horizontal, no row
    edge 2 (80,56) -> (88,48) down:  from (88,48): rows 3 <= y < 4; y = 3: (-8 * 0 + 88 * 8) / 128 = 704/128 = 5.5 -> right 6
    edge 3 (88,48) -> (80,40) down:  from (80,40): rows ceil(40/16) = 3 <= y < ceil(48/16) = 3: none
    edge 4 (80,40) -> (32,40):       horizontal
    edge 5 (32,40) -> (24,48) up:    rows 3 <= y < 3: none
    Row 3 covers 2 <= x < 6."""
    X, Y = [24, 32, 80, 88, 80, 32], [48, 56, 56, 48, 40, 40]
    nv, HX, HY = raster.hexagons([32], [48], [80], [48], 8)
    assert HX[0, :6].tolist() == X and HY[0, :6].tolist() == Y and nv.tolist() == [6]
    rows = raster.spans_reference(64, 64, X, Y)
    assert rows == {3: (2, 6)}
    assert raster.covered(rows) == {(2, 3), (3, 3), (4, 3), (5, 3)}
    # the same line drawn backwards: dx < dy, dx < -dy ... the other order, the same texels
    nv, HX, HY = raster.hexagons([80], [48], [32], [48], 8)
    assert HX[0, :6].tolist() == [24, 32, 80, 88, 80, 32] and HY[0, :6].tolist() == [48, 56, 56, 48, 40, 40]


def test_steep_hexagon():
    """Texel centres (2, 1) -> (4, 7): endpoints (32, 16), (64, 112), dx = 32 <= dy = 96, dx > -dy: L0 L1 T1 R1 R0 B0 =
    (24,16) (56,112) (64,120) (72,112) (40,16) (32,8).
    edge 0 (24,16) -> (56,112) up:   rows 1 <= y < 7, (32 (16 y - 16) + 24 * 96) / 1536 = (512 y + 1792) / 1536:
                                     y = 1..6: 1.5, 1.83, 2.17, 2.5, 2.83, 3.17 -> left 2, 2, 3, 3, 3, 4
    edge 1 (56,112) -> (64,120) up:  row 7: (0 + 56 * 8) / 128 = 3.5 -> left 4
    edge 2 (64,120) -> (72,112) down: from (72,112): row 7: (0 + 72 * 8) / 128 = 4.5 -> right 5
    edge 3 (72,112) -> (40,16) down: from (40,16): rows 1 <= y < 7, (512 y + 3328) / 1536:
                                     y = 1..6: 2.5, 2.83, 3.17, 3.5, 3.83, 4.17 -> right 3, 3, 4, 4, 4, 5
    edge 4 (40,16) -> (32,8) down:   from (32,8): rows ceil(8/16) = 1 <= y < ceil(16/16) = 1: none
    edge 5 (32,8) -> (24,16) up:     rows 1 <= y < 1: none
    One texel per row: x = 2, 2, 3, 3, 3, 4, 4 on rows 1..7 (the line x = 2 + (y - 1) / 3, rounded)."""
    nv, X, Y = raster.hexagons([32], [16], [64], [112], 8)
    assert X[0, :6].tolist() == [24, 56, 64, 72, 40, 32] and Y[0, :6].tolist() == [16, 112, 120, 112, 16, 8]
    rows = raster.spans_reference(16, 16, X[0, :6], Y[0, :6])
    assert rows == {1: (2, 3), 2: (2, 3), 3: (3, 4), 4: (3, 4), 5: (3, 4), 6: (4, 5), 7: (4, 5)}
    # a target of 5 rows and 3 columns: rows 5.. are not walked, x is clamped to 3 (row 3's span [3, 4) becomes [3, 3): empty)
    assert raster.spans_reference(3, 5, X[0, :6], Y[0, :6]) == {1: (2, 3), 2: (2, 3), 3: (3, 3), 4: (3, 3)}


def test_rows_are_half_open_at_a_vertex_on_a_texel_centre():
    """a rectangle (0,Ya) (0,Yb) (64,Yb) (64,Ya): the left edge goes up, the right edge down, x from 0 to ceil(64/16) = 4.
    Ya = 16, Yb = 48: rows ceil(16/16) = 1 <= y < ceil(48/16) = 3 - the row whose centre the lower vertices lie ON is covered,
    the row whose centre the upper vertices lie on is not.  One sixteenth up (17, 49): rows 2, 3.  One down (15, 47): 1, 2."""
    def rect(ya, yb):
        return raster.spans_reference(8, 8, [0, 0, 64, 64], [ya, yb, yb, ya])
    assert rect(16, 48) == {1: (0, 4), 2: (0, 4)}
    assert rect(17, 49) == {2: (0, 4), 3: (0, 4)}
    assert rect(15, 47) == {1: (0, 4), 2: (0, 4)}
    assert rect(0, 16) == {0: (0, 4)} and rect(-16, 0) == {} and rect(-15, 1) == {0: (0, 4)}
    assert rect(112, 200) == {7: (0, 4)}                         # (rows 7 .. 12 of a target of 8)


def test_a_crossing_exactly_on_an_integer_and_a_sixteenth_to_either_side():
    """edge (X, 0) -> (X + 32, 32) going up, against a right edge far away at x = 10; row 1: (32 * 16 + X * 32) / 512.
    X = 32: 1536 / 512 = 3 exactly: ceil adds nothing, left 3.  X = 31: 1504 / 512 = 2.94 -> 3.  X = 33: 1568 / 512 = 3.06 -> 4.
    Row 0: X * 32 / 512 = X / 16: 2 exactly, 1.94 -> 2, 2.06 -> 3.
    The same edge going down (the polygon listed the other way round) is the right end: texel 3 is covered only from 3.06 on."""
    def left(X):
        return raster.spans_reference(16, 16, [X, X + 32, 160, 160], [0, 32, 32, 0])
    assert left(32) == {0: (2, 10), 1: (3, 10)}
    assert left(31) == {0: (2, 10), 1: (3, 10)}
    assert left(33) == {0: (3, 10), 1: (4, 10)}
    def right(X):
        return raster.spans_reference(16, 16, [-160, -160, X + 32, X], [0, 32, 32, 0])
    assert right(32) == {0: (0, 2), 1: (0, 3)}
    assert right(31) == {0: (0, 2), 1: (0, 3)}
    assert right(33) == {0: (0, 3), 1: (0, 4)}
    assert raster.ceil_div(-1, 16) == 0 and raster.ceil_div(-16, 16) == -1 and raster.ceil_div(-17, 16) == -1 and raster.ceil_div(17, 16) == 2


def test_a_later_edge_overwrites_an_earlier_one():
    """a bow tie (0,0) (64,32) (64,0) (0,32): edges 0 and 2 both go up and both cross rows 0 and 1; edge 2 is listed later, so its
    x is the row's left: row 0: 64, row 1: ceil((-64 * 16 + 64 * 32) / 512) = 2.  Edge 1 goes down at x = 4, edge 3 at x = 0 (later)."""
    assert raster.spans_reference(16, 16, [0, 64, 64, 0], [0, 32, 0, 32]) == {0: (4, 0), 1: (2, 0)}


def test_batch_reference_equals_the_python_integers():
    """the int64 form of the rule against the Python integers: random polygons of 3..10 vertices, small coordinates and
    coordinates up to 2^25, targets that clamp and targets that do not"""
    rng = np.random.default_rng(11)
    for scale, fw, fh, cap in ((200, 16, 16, 32), (3000, 100, 300, 400), (1 << 25, 1 << 22, 64, 64), (1 << 25, 4096, 300, 300)):
        polys = []
        for _ in range(40):
            n = int(rng.integers(3, 11))
            polys.append((rng.integers(-scale // 4, scale, n).tolist(), rng.integers(-scale // 4, scale, n).tolist()))
        nv, X, Y = raster.pack(polys)
        r0, left, right = raster.spans_reference_batch(fw, fh, nv, X, Y, cap)
        w0, w1, ymin, ymax = raster.window(fh, nv, Y)
        assert (w0 == r0).all()
        seen = 0
        for t, (x, y) in enumerate(polys):
            assert ymin[t] == min(y) and ymax[t] == max(y)
            want = raster.spans_reference(fw, fh, x, y)
            got = {int(r0[t]) + r: (int(left[t, r]), int(right[t, r])) for r in range(cap) if (left[t, r], right[t, r]) != (fw, 0)}
            assert got == {r: s for r, s in want.items() if s != (fw, 0)}, (scale, t)
            seen += len(want)
        assert seen > 100


def test_small_predicate_by_hand():
    nv = np.full(4, 6)
    X = np.array([[0, 4095, 5, 6, 7, 8], [0, 4096, 5, 6, 7, 8], [1 << 19, (1 << 19) - 9, (1 << 19) - 5, (1 << 19) - 5, (1 << 19) - 5, (1 << 19) - 5],
                  [-(1 << 19) + 1, -(1 << 19) + 9, -(1 << 19) + 9, -(1 << 19) + 9, -(1 << 19) + 9, -(1 << 19) + 9]])
    Y = np.array([[0, 1023, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1024, 2, 3, 4, 5]])
    assert raster.is_small_reference(nv, X, Y).tolist() == [True, False, False, False]
    Y[3, 1] = 1023
    assert raster.is_small_reference(nv, X, Y).tolist() == [True, False, False, True]


def test_param_reference_by_hand():
    f32 = np.float32
    # ten texels along x: fragment (5, 0) lies half way; (3, 7) projects to 0.3 whatever its y; one texel before the start: -0.1
    assert raster.param_reference(0, 0, 160, 0, 5, 0) == f32(0.5)
    assert raster.param_reference(0, 0, 160, 0, 3, 7) == f32(7680.0) / f32(25600.0) == f32(0.3)
    assert raster.param_reference(0, 0, 160, 0, -1, 0) == f32(-0.1)
    assert raster.param_reference(8, 8, 8, 8, 3, 3) is None
    # integers past 2^24 are rounded to even BEFORE the division: ex = 4097, the fragment 4111 sixteenths along.
    # num = 4111 * 4097 = 16842767 -> 16842768 (between ...766 and ...768, the halves 8421383 and 8421384: the even one)
    # den = 4097^2 = 16785409 -> 16785408 (halves 8392704 and 8392705)
    got = raster.param_reference(1, 0, 4098, 0, 257, 0)
    assert 4111 * 4097 == 16842767 and 4097 * 4097 == 16785409
    assert got == f32(16842768.0) / f32(16785408.0) and got.dtype == np.float32
    ok, bits = raster.param_reference_batch([1, 0, 8], [0, 0, 8], [4098, 160, 8], [0, 0, 8], [257, 3, 3], [0, 7, 3])
    assert ok.tolist() == [True, True, False] and bits[:2].tolist() == [int(got.view(np.uint32)), int(f32(0.3).view(np.uint32))]
    assert raster.short32_reference([0, 0, 5, 5], [0, 0, 0, 0], [16383, 16384, 5, -16379], [0, 0, -16384, 16383]).tolist() == [True, False, False, False]
    rng = np.random.default_rng(3)
    a = rng.integers(-40000, 40000, (6, 500))
    ok, bits = raster.param_reference_batch(a[0], a[1], a[2], a[3], a[4] // 16, a[5] // 16)
    for k in range(500):
        want = raster.param_reference(a[0, k], a[1, k], a[2, k], a[3, k], a[4, k] // 16, a[5, k] // 16)
        assert ok[k] and bits[k] == want.view(np.uint32)
