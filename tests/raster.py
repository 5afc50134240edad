"""The test-only harness around the line rasteriser's integer routines (tests/native/raster_harness.hip: the header functions
of th_raster.hpp, instantiated as the product's kernels instantiate them) as numpy-in / numpy-out functions, and the exact
references the GPU tests compare with (tests/test_gpu_raster.py); the references are pinned on cases worked through by hand
in tests/test_raster_build.py.

The rule (th_raster.hpp, oracle/tendrils_oracle.c): a polygon snapped to sixteenths of a texel, texel centres at multiples of
16.  An edge (X1, Y1) -> (X2, Y2), Y1 < Y2, crosses the rows ceil(Y1/16) <= y < ceil(Y2/16) at
x = clamp(ceil((DX (16 y - Y1) + X1 DY) / (16 DY)), 0, fw); an edge that goes up in y as the vertices are listed sets the row's
`left`, one that goes down its `right`, a later edge over an earlier one; the row covers left <= x < right."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIB_PATH = os.environ.get("TH_RASTER_LIB") or os.path.join(NATIVE, "_build", "libth_raster.so")   # TH_RASTER_LIB: diagnostic builds
ENTRY_POINTS = ["thr_last_error", "thr_param", "thr_spans"]
VARIANTS = {"poly6": 0, "poly0": 1, "small_hexagon": 2, "small_hexagon2": 3, "row_span": 4, "tri_span": 5}
SMALL_VARIANTS = ("small_hexagon", "small_hexagon2", "row_span")
STRIDE = 12             # vertices a polygon's row of X / Y holds (raster_harness.hip: kMaxVertices)
PARAM_VIEW = 4096       # (raster_harness.hip: kParamView)

_i32p, _u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_PROTOTYPES = {
    "thr_last_error": (C.c_char_p, []),
    "thr_spans": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "thr_param": (C.c_int, [C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _u32p]),
}
_lib = None


class RasterError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("raster harness code %d: %s" % (code, message))
        self.code = code


def build():
    """make the harness (and the product first, when it is missing: the loader takes the product library before this one)"""
    if not os.path.exists(os.path.join(ROOT, "tendrils_amd", "lib", "libtendrils_hip.so")):
        import __graft_entry__ as g
        g.build()
    subprocess.check_call(["make", "-C", NATIVE, "all"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    """The product library first (tendrils_amd._capi.load: the process keeps ONE ROCm runtime), then the harness."""
    global _lib
    if _lib is None:
        from tendrils_amd import _capi
        _capi.load()
        if not os.path.exists(LIB_PATH):
            build()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _call(name, *args):
    lib = load()
    code = getattr(lib, name)(*args)
    if code != 0:
        raise RasterError(code, lib.thr_last_error().decode(errors="replace"))


def _i32(a):
    a = np.asarray(a)
    assert np.all(np.abs(a.astype(np.int64)) < 2 ** 31)
    return np.ascontiguousarray(a, np.int32)


# ---- the routines, host arrays in and out ---------------------------------------------------------------------------------
def pack(polygons):
    """[(X list, Y list), ...] -> nv [count], X [count, STRIDE], Y [count, STRIDE] (the unused places 0)"""
    nv = np.array([len(x) for x, _ in polygons], np.int32)
    X, Y = np.zeros((len(polygons), STRIDE), np.int64), np.zeros((len(polygons), STRIDE), np.int64)
    for t, (x, y) in enumerate(polygons):
        assert len(x) == len(y) <= STRIDE
        X[t, :len(x)] = x
        Y[t, :len(y)] = y
    return nv, X, Y


def spans(variant, fw, fh, nv, X, Y, cap):
    """One lane per polygon through `variant` on an fw x fh target.  -> head [count, 8], rows [count, cap, 4]:
    head = (verdict of dep_hexagon_is_small or -1, ymin, ymax, first row of the window, texels, strays, rows out of order, rows
    asked for); rows[t, r] = (texels, least x, greatest x, texels not after their predecessor) of row head[t, 3] + r."""
    nv, X, Y = _i32(nv), _i32(X), _i32(Y)
    count = nv.size
    assert X.shape == Y.shape == (count, STRIDE)
    head, rows = np.empty((count, 8), np.int32), np.empty((count, cap, 4), np.int32)
    _call("thr_spans", VARIANTS[variant], fw, fh, count, cap, nv.ctypes.data_as(_i32p), X.ctypes.data_as(_i32p), Y.ctypes.data_as(_i32p),
          head.ctypes.data_as(_i32p), rows.ctypes.data_as(_i32p))
    return head, rows


def param(sx0, sy0, sx1, sy1, x, y):
    """dep_param of fragment (x, y) of the line with these snapped endpoints, set up by dep_setup.  -> [count, 9] uint32:
    (short32, verdict, bits of t, verdict and bits of t with short32 forced false, the endpoints as dep_setup snapped them)"""
    arrays = [_i32(a) for a in (sx0, sy0, sx1, sy1, x, y)]
    count = arrays[0].size
    assert all(a.shape == (count,) for a in arrays)
    out = np.empty((count, 9), np.uint32)
    _call("thr_param", count, *[a.ctypes.data_as(_i32p) for a in arrays], out.ctypes.data_as(_u32p))
    return out


# ---- references ---------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    """ceil(a / b) of Python integers, b > 0 (floor division rounds down for either sign)"""
    assert b > 0
    return -((-a) // b)


def spans_reference(fw, fh, X, Y):
    """The rule for ONE polygon in Python integers.  -> {row: (left, right)} of every row an edge crosses (left >= right: no texel)"""
    X, Y = [int(v) for v in X], [int(v) for v in Y]
    rows, n = {}, len(X)
    for k in range(n):
        xa, ya, xb, yb = X[k], Y[k], X[(k + 1) % n], Y[(k + 1) % n]
        if ya == yb:
            continue
        up = yb > ya
        x1, y1, x2, y2 = (xa, ya, xb, yb) if up else (xb, yb, xa, ya)
        dx, dy = x2 - x1, y2 - y1
        for y in range(max(ceil_div(y1, 16), 0), min(ceil_div(y2, 16), fh)):
            x = min(max(ceil_div(dx * (16 * y - y1) + x1 * dy, 16 * dy), 0), fw)
            left, right = rows.get(y, (fw, 0))
            rows[y] = (x, right) if up else (left, x)
    return rows


def covered(rows):
    """{row: (left, right)} -> the set of covered texels (x, y)"""
    return {(x, y) for y, (left, right) in rows.items() for x in range(left, right)}


def window(fh, nv, Y):
    """per polygon: the first row of its range inside the target and the row behind its last (the harness's window starts there)"""
    Y = np.asarray(Y, np.int64)
    live = np.arange(Y.shape[1])[None, :] < np.asarray(nv)[:, None]
    ymin = np.where(live, Y, np.iinfo(np.int64).max).min(axis=1)
    ymax = np.where(live, Y, np.iinfo(np.int64).min).max(axis=1)
    r0, r1 = np.clip((ymin + 15) >> 4, 0, None), np.clip((ymax + 15) >> 4, None, fh)
    return r0, np.maximum(r1, r0), ymin, ymax


def spans_reference_batch(fw, fh, nv, X, Y, cap, census=None):
    """spans_reference for many polygons at once in int64 (every product is bounded below 2^62 first, from the inputs: the
    arithmetic is then exact; tests/test_raster_build.py holds it against the Python integers).
    -> r0 [count], left [count, cap], right [count, cap] for rows r0 + 0..cap-1 (fw, 0 where no edge crosses)
    census: a dict that receives, per polygon, whether any crossing had remainder 0 ("exact"), 1 ("one") or den - 1 ("last")"""
    nv, X, Y = np.asarray(nv, np.int64), np.asarray(X, np.int64), np.asarray(Y, np.int64)
    count = nv.size
    r0, r1, _, _ = window(fh, nv, Y)
    assert int((r1 - r0).max()) <= cap
    span_x, span_y = int(np.abs(X).max()) * 2 + 1, int(np.abs(Y).max()) * 2 + 16 * cap + 16
    assert span_x * span_y * 2 < 2 ** 62
    y = r0[:, None] + np.arange(cap, dtype=np.int64)[None, :]
    inside = y < r1[:, None]
    left, right = np.full((count, cap), fw, np.int64), np.zeros((count, cap), np.int64)
    for k in range(int(nv.max())):
        kn = np.where(k + 1 == nv, 0, k + 1)
        kn = np.where(k < nv, kn, 0)
        xa, ya, xb, yb = X[:, k], Y[:, k], X[np.arange(count), kn], Y[np.arange(count), kn]
        up = yb > ya
        x1, y1, x2, y2 = np.where(up, xa, xb), np.where(up, ya, yb), np.where(up, xb, xa), np.where(up, yb, ya)
        dx, dy = x2 - x1, y2 - y1
        live = (k < nv) & (dy > 0)
        crosses = inside & live[:, None] & (y >= ((y1 + 15) >> 4)[:, None]) & (y < ((y2 + 15) >> 4)[:, None])
        den = np.where(live, 16 * dy, 1)[:, None]
        num = dx[:, None] * (16 * y - y1[:, None]) + (x1 * dy)[:, None]
        x = np.clip(-((-num) // den), 0, fw)
        if census is not None:
            rem = num - (num // den) * den
            for name, hit in (("exact", rem == 0), ("one", (rem == 1) & (den > 16)), ("last", (rem == den - 1) & (den > 16))):
                census[name] = census.get(name, np.zeros(count, bool)) | (crosses & hit).any(axis=1)
        left = np.where(crosses & up[:, None], x, left)
        right = np.where(crosses & ~up[:, None], x, right)
    return r0, left, right


def assert_spans(head, rows, reference, what, select=None):
    """What the harness tallied is exactly the reference's spans: per row the run left..right-1, every texel once and in rising
    order, no row twice, no texel outside the window or the target.  select: the polygons to hold to it (default all)."""
    r0, left, right = reference
    pick = np.ones(head.shape[0], bool) if select is None else np.asarray(select, bool)
    want = np.clip(right - left, 0, None)

    def first(bad):
        t = int(np.flatnonzero(bad)[0])
        return "%s: polygon %d: head %s, rows %s, reference left %s right %s from row %d" % (
            what, t, head[t].tolist(), rows[t][:12].tolist(), left[t][:12].tolist(), right[t][:12].tolist(), int(r0[t]))

    bad = pick & (head[:, 3] != r0)
    assert not bad.any(), "window: " + first(bad)
    bad = pick & ((head[:, 5] != 0) | (head[:, 6] != 0))
    assert not bad.any(), "strays or rows out of order: " + first(bad)
    bad = pick & (rows[:, :, 0] != want).any(axis=1)
    assert not bad.any(), "texels of a row: " + first(bad)
    some = want > 0
    bad = pick & (some & ((rows[:, :, 1] != left) | (rows[:, :, 2] != right - 1))).any(axis=1)
    assert not bad.any(), "ends of a row: " + first(bad)
    bad = pick & (rows[:, :, 3] != 0).any(axis=1)
    assert not bad.any(), "a texel twice or out of order: " + first(bad)
    bad = pick & (head[:, 4] != want.sum(axis=1))
    assert not bad.any(), "texels in all: " + first(bad)


def is_small_reference(nv, X, Y):
    """the stated predicate of dep_hexagon_is_small: every x inside (-2^19, 2^19), less than 4096 wide, less than 1024 tall"""
    X, Y = np.asarray(X, np.int64)[:, :6], np.asarray(Y, np.int64)[:, :6]
    assert (np.asarray(nv) == 6).all()
    return ((X.min(axis=1) > -(1 << 19)) & (X.max(axis=1) < (1 << 19)) & (X.max(axis=1) - X.min(axis=1) < 4096)
            & (Y.max(axis=1) - Y.min(axis=1) < 1024))


def param_reference(sx0, sy0, sx1, sy1, x, y):
    """ONE fragment in Python integers: None when the endpoints are one point, else float32(num) / float32(den) - each integer
    rounded to nearest even (through float(), exact below 2^53), the division in float32"""
    ex, ey = int(sx1) - int(sx0), int(sy1) - int(sy0)
    den = ex * ex + ey * ey
    if den == 0:
        return None
    num = (16 * int(x) - int(sx0)) * ex + (16 * int(y) - int(sy0)) * ey
    assert abs(num) < 2 ** 53 and den < 2 ** 53
    return np.float32(float(num)) / np.float32(float(den))


def param_reference_batch(sx0, sy0, sx1, sy1, x, y):
    """-> (den != 0, bits of t as uint32) in int64 / float64 (|num|, den < 2^53 asserted: exact), then as param_reference"""
    sx0, sy0, sx1, sy1, x, y = [np.asarray(a, np.int64) for a in (sx0, sy0, sx1, sy1, x, y)]
    ex, ey = sx1 - sx0, sy1 - sy0
    assert max(int(np.abs(ex).max()), int(np.abs(ey).max())) < 2 ** 25 and int(np.abs(16 * x - sx0).max()) < 2 ** 26 and int(np.abs(16 * y - sy0).max()) < 2 ** 26
    den = ex * ex + ey * ey
    num = (16 * x - sx0) * ex + (16 * y - sy0) * ey
    fnum, fden = num.astype(np.float64).astype(np.float32), np.where(den == 0, 1, den).astype(np.float64).astype(np.float32)
    t = fnum / fden
    assert t.dtype == np.float32
    return den != 0, t.view(np.uint32)


def short32_reference(sx0, sy0, sx1, sy1):
    """the stated gate of dep_param's 32-bit branch: |ex| and |ey| below 2^14"""
    ex, ey = np.asarray(sx1, np.int64) - np.asarray(sx0, np.int64), np.asarray(sy1, np.int64) - np.asarray(sy0, np.int64)
    return (np.abs(ex) < (1 << 14)) & (np.abs(ey) < (1 << 14))


# ---- hexagons as the front end leaves them -------------------------------------------------------------------------------------
def hexagons(ax, ay, bx, by, h, jitter=None):
    """The six vertices of lines a -> b (snapped endpoints, sixteenths; arrays) with a half-diamond of h sixteenths, in the
    order of dep_hexagon's four cases (chosen by the signs of dx - dy and dx + dy), plus `jitter` [count, 2, 6] on every
    coordinate.  -> nv, X, Y for spans()"""
    ax, ay, bx, by = [np.asarray(a, np.int64) for a in (ax, ay, bx, by)]
    count = ax.size
    h = np.broadcast_to(np.asarray(h, np.int64), (count,))
    dx, dy = bx - ax, by - ay
    X, Y = np.zeros((count, STRIDE), np.int64), np.zeros((count, STRIDE), np.int64)
    px, py = (ax, bx), (ay, by)
    # L: (x - h, y)  T: (x, y + h)  R: (x + h, y)  B: (x, y - h), of endpoint 0 (a) or 1 (b)
    orders = {(True, True): "L0 T0 T1 R1 B1 B0", (True, False): "L1 L0 T0 R0 R1 B1",
              (False, True): "L0 L1 T1 R1 R0 B0", (False, False): "L1 T1 T0 R0 B0 B1"}
    for (c1, c2), order in orders.items():
        m = ((dx > dy) == c1) & ((dx > -dy) == c2)
        for k, name in enumerate(order.split()):
            e = int(name[1])
            ox = {"L": -1, "R": 1}.get(name[0], 0)
            oy = {"T": 1, "B": -1}.get(name[0], 0)
            X[m, k] = (px[e] + ox * h)[m]
            Y[m, k] = (py[e] + oy * h)[m]
    if jitter is not None:
        X[:, :6] += jitter[:, 0]
        Y[:, :6] += jitter[:, 1]
    return np.full(count, 6, np.int32), X, Y
