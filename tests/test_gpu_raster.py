"""The line rasteriser's span routines and dep_param (th_raster.hpp) on the GPU, through the harness of tests/native/, against
the rule in exact integers (tests/raster.py; pinned by hand in tests/test_raster_build.py).  Everything is compared for equality:
per polygon and row the exact run of texels, every texel once.

The polygons are hexagons as the front end leaves them - two snapped endpoints, a half-diamond of 8 x width sixteenths, the six
vertices in dep_hexagon's order, every coordinate jittered by -1, 0 or +1 (rint of a - h and of a can differ by one) - in
families named for the branch or limit they visit; every case first asserts FROM ITS INPUTS that it holds at least 100
polygons on each side of what it is named for."""
import functools

import numpy as np
import pytest

import raster

pytestmark = pytest.mark.gpu

GENERAL = ("poly6", "poly0", "tri_span")
ALL = GENERAL + raster.SMALL_VARIANTS
MIN_SIDE = 100
CHUNK_ROWS = 1 << 21        # rows of all polygons of one launch (32 MiB of tallies)


def jitter(rng, count):
    return rng.integers(-1, 2, (count, 2, 6))


def edge_is_small(nv, X, Y):
    """per polygon and edge (DY > 0): inside the stated domain of dep_raster_poly's 32-bit branch - DY < 1024, |DX| < 4096,
    |X1| < 2^19 (X1: the lower end) - and whether the edge exists at all"""
    nv, X, Y = np.asarray(nv), np.asarray(X, np.int64), np.asarray(Y, np.int64)
    k = np.arange(raster.STRIDE)[None, :]
    kn = np.where(k + 1 == nv[:, None], 0, np.minimum(k + 1, raster.STRIDE - 1))
    xb, yb = np.take_along_axis(X, kn, 1), np.take_along_axis(Y, kn, 1)
    up = yb > Y
    x1 = np.where(up, X, xb)
    dx, dy = np.abs(xb - X), np.abs(yb - Y)
    edge = (k < nv[:, None]) & (dy > 0)
    return edge & (dy < 1024) & (dx < 4096) & (np.abs(x1) < (1 << 19)), edge


class Case:
    """polygons on one target, cut into launches of polygons of like height, each with its reference (computed once)"""
    def __init__(self, fw, fh, nv, X, Y, census=False):
        self.fw, self.fh, self.nv, self.X, self.Y = fw, fh, np.asarray(nv), np.asarray(X, np.int64), np.asarray(Y, np.int64)
        r0, r1, _, _ = raster.window(fh, self.nv, self.Y)
        self.rows = r1 - r0
        order = np.argsort(self.rows, kind="stable")
        self.census = {} if census else None
        self.chunks, at = [], 0
        while at < order.size:
            # (the polygons are sorted by height: the chunk ends where its tallest polygon times its count passes CHUNK_ROWS)
            n = 1
            while at + n < order.size and (n + 1) * (int(self.rows[order[at + n]]) + 1) <= CHUNK_ROWS and n < 32768:
                n += 1
            idx = order[at:at + n]
            cap = int(self.rows[idx].max()) + 1
            part = {} if census else None
            ref = raster.spans_reference_batch(fw, fh, self.nv[idx], self.X[idx], self.Y[idx], cap, part)
            ref = (ref[0], ref[1].astype(np.int32), ref[2].astype(np.int32))
            if census:
                for name, hit in part.items():
                    self.census.setdefault(name, np.zeros(order.size, bool))[idx] = hit
            self.chunks.append((idx, cap, ref))
            at += n
        self.small = raster.is_small_reference(self.nv, self.X, self.Y) if (self.nv == 6).all() else None

    def run(self, variant, what):
        for idx, cap, ref in self.chunks:
            nv, X, Y = self.nv[idx], self.X[idx], self.Y[idx]
            if variant == "tri_span":
                keep = nv <= 7                                           # (a TrianglePoly holds seven vertices)
                if not keep.any():
                    continue
                idx, nv, X, Y, ref = idx[keep], nv[keep], X[keep], Y[keep], tuple(r[keep] for r in ref)
            elif variant != "poly0":
                assert (nv == 6).all()
            head, rows = raster.spans(variant, self.fw, self.fh, nv, X, Y, cap)
            select = None
            if variant in raster.SMALL_VARIANTS:
                select = self.small[idx]
                assert (head[:, 0] == select).all(), "%s: dep_hexagon_is_small differs from its stated predicate at polygon %d" % (
                    what, int(idx[np.flatnonzero(head[:, 0] != select)[0]]))
                assert (head[~select, 4] == 0).all()
                assert (head[:, 1] == Y[:, :6].min(axis=1)).all() and (head[:, 2] == Y[:, :6].max(axis=1)).all()
            else:
                assert (head[:, 0] == -1).all()
            raster.assert_spans(head, rows, ref, "%s / %s" % (what, variant), select)


def both_sides(flag, what):
    flag = np.asarray(flag, bool)
    assert flag.sum() >= MIN_SIDE and (~flag).sum() >= MIN_SIDE, "%s: %d on one side, %d on the other" % (what, flag.sum(), (~flag).sum())


def line_hexagons(rng, ax, ay, bx, by, h, jit=True):
    count = np.asarray(ax).size
    return raster.hexagons(ax, ay, bx, by, h, jitter(rng, count) if jit else None)


# ---- 1: the limits of dep_hexagon_is_small -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def small_limits(limit, fw):
    rng = np.random.default_rng({"width": 1, "height": 2, "xmax": 3, "xmin": 4}[limit] * 1000 + fw)
    count = 6000
    h = rng.choice([8, 16, 28], count)
    flip = rng.random(count) < 0.5
    fh = 256
    if limit == "width":          # xmax - xmin = |dx| + 2 h (+ jitter) around 4095
        dx = (4095 - 2 * h + rng.integers(-2, 3, count)) * rng.choice([-1, 1], count)
        dy = rng.integers(-900, 901, count)
        ax = rng.integers(5000, 16 * 32768 - 10000, count)
    elif limit == "height":       # ymax - ymin = |dy| + 2 h around 1023
        dy = (1023 - 2 * h + rng.integers(-2, 3, count)) * rng.choice([-1, 1], count)
        dx = rng.integers(-3000, 3001, count)
        ax = rng.integers(5000, 16 * 32768 - 10000, count)
    else:                         # the rightmost vertex around 2^19 (16 fw of a 32768-texel view), or the leftmost around -2^19
        dx = rng.integers(0, 3000, count)
        dy = rng.integers(-900, 901, count)
        edge = (1 << 19) - 1 + rng.integers(-2, 3, count)
        ax = edge - h - dx if limit == "xmax" else -(edge - h) + 0 * dx
    ay = rng.integers(1100, 16 * fh - 1100, count)
    bx, by = ax + dx, ay + dy
    ax, bx = np.where(flip, bx, ax), np.where(flip, ax, bx)
    ay, by = np.where(flip, by, ay), np.where(flip, ay, by)
    nv, X, Y = line_hexagons(rng, ax, ay, bx, by, h)
    return Case(fw, fh, nv, X, Y)


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("fw", [32768, 40000])
@pytest.mark.parametrize("limit", ["width", "height", "xmax", "xmin"])
def test_limits_of_the_small_hexagon(limit, fw, variant):
    """xmax - xmin in {4094, 4095, 4096}, ymax - ymin in {1022, 1023, 1024}, xmax in {2^19 - 2, 2^19 - 1, 2^19} (and xmin
    mirrored), on a view of 32768 texels and on a wider one that does not clamp the quotient at 2^19"""
    case = small_limits(limit, fw)
    X, Y = case.X[:, :6], case.Y[:, :6]
    measure = {"width": X.max(axis=1) - X.min(axis=1), "height": Y.max(axis=1) - Y.min(axis=1), "xmax": X.max(axis=1), "xmin": -X.min(axis=1)}[limit]
    values = {"width": (4094, 4095, 4096), "height": (1022, 1023, 1024)}.get(limit, ((1 << 19) - 2, (1 << 19) - 1, 1 << 19))
    for v in values:
        assert (measure == v).sum() >= MIN_SIDE, (limit, v, int((measure == v).sum()))
    both_sides(case.small, "small / not small")
    assert ((measure >= values[2]) == ~case.small).all()               # (nothing else decides the verdict here)
    case.run(variant, "limit %s, fw %d" % (limit, fw))


# ---- 2: every denominator --------------------------------------------------------------------------------------------------
DX_SET = [0, 1, 15, 16, 17, 255, 4077, 4095]           # (4077 = 4095 - 2 h - 2: the widest a SMALL hexagon of width 1 gets)
X1_SET = [0, 17, 1 << 15, (1 << 19) - 4097]


@functools.lru_cache(maxsize=1)
def every_denominator():
    rng = np.random.default_rng(20)
    dy, dx, x1 = np.meshgrid(np.arange(1, 1024), np.array(sorted({s * d for d in DX_SET for s in (1, -1)})), np.array(X1_SET), indexing="ij")
    dy, dx, x1 = dy.ravel(), dx.ravel(), x1.ravel()
    count = dy.size
    h = 8
    ax, ay = x1 + h, rng.integers(100, 400, count)
    bx, by = ax + dx, ay + dy
    flip = rng.random(count) < 0.5
    ax, bx = np.where(flip, bx, ax), np.where(flip, ax, bx)
    ay, by = np.where(flip, by, ay), np.where(flip, ay, by)
    nv, X, Y = line_hexagons(rng, ax, ay, bx, by, h, jit=False)
    return Case(40000, 96, nv, X, Y), dy, dx, x1


@pytest.mark.parametrize("variant", ALL)
def test_every_denominator(variant):
    """DY = 1 .. 1023 (v_rcp_f32's error depends on the denominator) x DX in +-{0, 1, 15, 16, 17, 255, 4077, 4095} x
    X1 in {0, 17, 2^15, 2^19 - 4097}: the hexagon's two long edges have exactly that DX and DY (no jitter here) and start at X1
    and X1 + 2 h; fw = 40000 clamps none of it."""
    case, dy, dx, x1 = every_denominator()
    X, Y = case.X[:, :6], case.Y[:, :6]
    ex, ey = np.roll(X, -1, axis=1) - X, np.roll(Y, -1, axis=1) - Y
    has = ((np.abs(ey) == dy[:, None]) & (np.abs(ex) == np.abs(dx)[:, None])).sum(axis=1)
    assert (has >= 2).all() and sorted(set(dy.tolist())) == list(range(1, 1024))
    assert sorted(set(np.abs(dx).tolist())) == sorted(DX_SET) and sorted(set(x1.tolist())) == sorted(X1_SET)
    for d in DX_SET:
        for s in X1_SET:
            assert len(set(dy[(np.abs(dx) == d) & (x1 == s)].tolist())) == 1023
    both_sides(case.small, "small / not small")
    small_edges, edges = edge_is_small(case.nv, case.X, case.Y)
    assert (small_edges == edges)[x1 < (1 << 18)].all()                 # every edge takes dep_raster_poly's 32-bit branch (but beside 2^19)
    case.run(variant, "every denominator")


# ---- 3: exact hits -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def exact_hits():
    rng = np.random.default_rng(30)
    count = 30000
    grid = np.arange(count) < count // 2         # half of them: endpoints on texel centres, width 2 (h = 16): every vertex a multiple of 16
    h = np.where(grid, 16, rng.choice([8, 16, 28], count))
    ax, ay = rng.integers(-40, 2000, count), rng.integers(-40, 2000, count)
    dx, dy = rng.integers(-640, 641, count), rng.integers(-640, 641, count)
    ax, ay, dx, dy = [np.where(grid, v // 16 * 16, v) for v in (ax, ay, dx, dy)]
    jit = jitter(rng, count) * ~grid[:, None, None]
    nv, X, Y = raster.hexagons(ax, ay, ax + dx, ay + dy, h, jit)
    return Case(120, 120, nv, X, Y, census=True), grid


@pytest.mark.parametrize("variant", ALL)
def test_exact_hits(variant):
    """vertices on texel centres (X and Y multiples of 16: rows half-open at both ends of every edge), and crossings that leave
    remainder 0 (ceil adds nothing), 1 and den - 1"""
    case, grid = exact_hits()
    on_grid = ((case.X[:, :6] % 16 == 0) & (case.Y[:, :6] % 16 == 0)).all(axis=1)
    assert (on_grid[grid]).all() and on_grid.sum() >= MIN_SIDE and (~on_grid).sum() >= MIN_SIDE
    for name in ("exact", "one", "last"):
        both_sides(case.census[name], "crossings with remainder " + name)
        assert (case.census[name] & case.small).sum() >= MIN_SIDE
    case.run(variant, "exact hits")


# ---- 4: beyond the cheap branch --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def beyond(fw):
    rng = np.random.default_rng(40 + fw)
    combos = [(dx * sx, dy * sy, x1) for dx in (4096, 1 << 14, 1 << 20, 1 << 25) for sx in (1, -1) for dy in (1024, 1 << 15, 1 << 25) for sy in (1, -1)
              for x1 in (1000, 1 << 19, 1 << 24)] * 3
    dx, dy, x1 = [np.array(v) for v in zip(*combos)]
    count = dx.size
    h = rng.choice([8, 16, 28], count)
    ax, ay = x1 + h, rng.integers(-200, 4000, count)
    ay = np.where(dy < 0, 16 * 4096 - ay, ay)                # (a line that goes down starts at the top of the target)
    nv, X, Y = line_hexagons(rng, ax, ay, ax + dx, ay + dy, h)
    return Case(fw, 4096, nv, X, Y), dx, dy, x1


@pytest.mark.parametrize("variant", GENERAL)
@pytest.mark.parametrize("fw", [32768, 1 << 22])
def test_beyond_the_cheap_branch(fw, variant):
    """|DX| in {4096, 2^14, 2^20, 2^25}, DY in {1024, 2^15, 2^25}, X1 in {2^19, 2^24}, up to 4096 rows: the 64-bit division of
    dep_raster_poly and tri_span, on a view that clamps and on one wide enough (2^22 texels) to hold most quotients"""
    case, dx, dy, x1 = beyond(fw)
    assert case.nv.size == 4 * 2 * 3 * 2 * 3 * 3 and case.rows.max() >= 4000
    small_edges, edges = edge_is_small(case.nv, case.X, case.Y)
    long_edges = edges & ~small_edges
    # (a jitter of -1 takes an edge of exactly 4096 or 1024 back inside: those are the limit's other side)
    assert long_edges.any(axis=1).sum() >= MIN_SIDE and (long_edges.sum(axis=1) >= 2).sum() >= MIN_SIDE and small_edges.sum() >= MIN_SIDE
    for v in (4096, 1 << 14, 1 << 20, 1 << 25):
        assert (np.abs(dx) == v).sum() >= 30
    for v in (1024, 1 << 15, 1 << 25):
        assert (np.abs(dy) == v).sum() >= 30
    for v in (1000, 1 << 19, 1 << 24):
        assert (x1 == v).sum() >= 30
    assert fw == 32768 or fw > (1 << 24) // 16 + (1 << 20) // 16         # (the wide view clamps no quotient of a line 2^20 long from 2^24)
    case.run(variant, "beyond the cheap branch, fw %d" % fw)


# ---- 5: clipped shapes -----------------------------------------------------------------------------------------------------
def clip_to_view(x, y, fw, fh):
    """Sutherland-Hodgman in integers against X >= -8, X <= 16 fw - 8, Y <= 16 fh - 8, Y >= -8 (the view's edges in sixteenths),
    an intersection rounded to the nearest sixteenth; like the product's clipper it emits a vertex ON a plane and then, when the
    next one is outside, the intersection - the same point again"""
    pts = list(zip(x, y))
    for axis, bound, sign in ((0, -8, 1), (0, 16 * fw - 8, -1), (1, 16 * fh - 8, -1), (1, -8, 1)):
        out = []
        for k, p in enumerate(pts):
            q = pts[(k + 1) % len(pts)]
            di, dj = sign * (p[axis] - bound), sign * (q[axis] - bound)
            cut = None
            if (di >= 0 and dj < 0) or (di < 0 and dj > 0):
                other = 1 - axis
                num, den = (q[other] - p[other]) * di, di - dj
                if den < 0:
                    num, den = -num, -den
                v = p[other] + (2 * num + den) // (2 * den)
                cut = (bound, v) if axis == 0 else (v, bound)
            if di >= 0:
                out.append(p)
                if dj < 0:
                    out.append(cut)
            elif dj > 0:
                out.append(cut)
        pts = out
        if len(pts) < 3:
            return None
    return pts


@functools.lru_cache(maxsize=1)
def clipped():
    rng = np.random.default_rng(50)
    fw, fh, count = 96, 64, 12000
    h = rng.choice([8, 28, 128, 512], count)
    # endpoints near the view's edges and corners (and some on them: vertices ON a plane)
    ax = rng.choice([-8, 16 * fw - 8], count) + rng.integers(-300, 301, count) * (rng.random(count) < 0.8)
    ay = rng.choice([-8, 16 * fh - 8, 500], count) + rng.integers(-300, 301, count) * (rng.random(count) < 0.8)
    swap = rng.random(count) < 0.5
    ax, ay = np.where(swap, rng.integers(-200, 16 * fw + 200, count), ax), np.where(swap, ay, rng.integers(-200, 16 * fh + 200, count))
    dx, dy = rng.integers(-900, 901, count), rng.integers(-900, 901, count)
    _, X, Y = line_hexagons(rng, ax, ay, ax + dx, ay + dy, h)
    polys = []
    for t in range(count):
        pts = clip_to_view(X[t, :6].tolist(), Y[t, :6].tolist(), fw, fh)
        if pts is None or len(pts) > raster.STRIDE:
            continue
        if len(pts) < 10 and rng.random() < 0.3:                          # a vertex twice in a row
            k = int(rng.integers(len(pts)))
            pts.insert(k, pts[k])
        polys.append(([p[0] for p in pts], [p[1] for p in pts]))
    nv, X, Y = raster.pack(polys)
    return Case(fw, fh, nv, X, Y), fw, fh


@pytest.mark.parametrize("variant", ["poly0", "tri_span"])
def test_clipped_shapes(variant):
    """hexagons of widths 1 .. 64 cut by the view: 3 to 10 vertices (tri_span: the 3 to 7 a TrianglePoly holds), horizontal
    edges on the top and bottom rows, vertical edges at X = -8 and X = 16 fw - 8, a vertex twice in a row"""
    case, fw, fh = clipped()
    nv, X, Y = case.nv, case.X, case.Y
    k = np.arange(raster.STRIDE)[None, :]
    kn = np.where(k + 1 == nv[:, None], 0, np.minimum(k + 1, raster.STRIDE - 1))
    xb, yb, live = np.take_along_axis(X, kn, 1), np.take_along_axis(Y, kn, 1), k < nv[:, None]
    for n in range(3, 11):
        assert (nv == n).sum() >= (MIN_SIDE if n <= 9 else 10), (n, int((nv == n).sum()))
    assert nv.max() <= 10
    flat, upright, distinct = live & (Y == yb), live & (X == xb), (X != xb) | (Y != yb)
    for what, hit in (("bottom", flat & distinct & (Y == -8)), ("top", flat & distinct & (Y == 16 * fh - 8)),
                      ("left", upright & distinct & (X == -8)), ("right", upright & distinct & (X == 16 * fw - 8)),
                      ("twice", live & ~distinct)):
        assert hit.any(axis=1).sum() >= MIN_SIDE, (what, int(hit.any(axis=1).sum()))
    case.run(variant, "clipped shapes")


# ---- 6: random jittered hexagons -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def random_hexagons(width):
    rng = np.random.default_rng(int(width * 10))
    count, fw, fh = 20000, 1024, 1024
    length = rng.uniform(0, 300 * 16, count) * (rng.random(count) > 0.02)          # (some of length 0: the diamond alone)
    angle = rng.uniform(0, 2 * np.pi, count)
    ax, ay = rng.integers(-20 * 16, (fw + 20) * 16, count), rng.integers(-20 * 16, (fh + 20) * 16, count)
    bx, by = ax + np.rint(length * np.cos(angle)).astype(np.int64), ay + np.rint(length * np.sin(angle)).astype(np.int64)
    nv, X, Y = line_hexagons(rng, ax, ay, bx, by, int(8 * width))
    return Case(fw, fh, nv, X, Y), bx - ax, by - ay


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("width", [1, 2, 3.5, 64])
def test_random_jittered_hexagons(width, variant):
    """20 000 lines per width, 0 to 300 texels long in any direction, on and around a 1024 x 1024 target: the hexagons the two
    pipelines rasterise with DIFFERENT routines"""
    case, dx, dy = random_hexagons(width)
    if width < 64:                                                       # (a hexagon of width 64 is 1024 sixteenths tall: never small)
        both_sides(case.small, "small / not small")
    else:
        assert case.small.sum() < MIN_SIDE
    small_edges, edges = edge_is_small(case.nv, case.X, case.Y)
    assert (edges & ~small_edges).any(axis=1).sum() >= MIN_SIDE and small_edges.any(axis=1).sum() >= MIN_SIDE
    for quadrant in ((dx > 0) & (dy > 0), (dx > 0) & (dy < 0), (dx < 0) & (dy > 0), (dx < 0) & (dy < 0)):
        assert quadrant.sum() >= MIN_SIDE
    case.run(variant, "random hexagons of width %s" % width)


# ---- dep_param -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def param_lines():
    rng = np.random.default_rng(70)
    ext = sorted({s * v for v in (0, 1, (1 << 14) - 1, 1 << 14, (1 << 14) + 1) for s in (1, -1)})
    ex, ey = [v.ravel() for v in np.meshgrid(np.array(ext), np.array(ext), indexing="ij")]
    reps = 40
    ex, ey = np.tile(ex, reps), np.tile(ey, reps)
    lines = ex.size
    sx0, sy0 = rng.integers(-(1 << 16), 1 << 17, lines), rng.integers(-(1 << 16), 1 << 17, lines)
    # fragments: along = -33 texels, the start, the middle, the end, +33 texels; across = -33, 0, +33 texels; and three anywhere between
    length = np.maximum(np.hypot(ex, ey), 1.0)
    ux, uy = ex / length, ey / length
    along = [-33 * 16 + 0 * length, 0 * length, length / 2, length, length + 33 * 16]
    frags = [(a, c) for a in along for c in (-33 * 16, 0, 33 * 16)]
    frags += [(rng.uniform(-33 * 16, 1, lines) + rng.random(lines) * (length + 33 * 16), rng.uniform(-33 * 16, 33 * 16, lines)) for _ in range(3)]
    cols = []
    for a, c in frags:
        fx, fy = sx0 + a * ux - c * uy, sy0 + a * uy + c * ux
        cols.append((sx0, sy0, sx0 + ex, sy0 + ey, np.floor(fx / 16 + 0.5).astype(np.int64), np.floor(fy / 16 + 0.5).astype(np.int64)))
    return [np.concatenate(v) for v in zip(*cols)]


def test_dep_param_both_branches_give_the_reference_float():
    """|ex|, |ey| in {0, 1, 2^14 - 1, 2^14, 2^14 + 1} in both signs; fragments at the ends, in the middle and up to 33 texels
    beyond each end and to each side.  short32 is what dep_setup set: it must be the stated gate; where it is true the 32-bit and the
    64-bit branch must give the same bits; both must be float32(num) / float32(den) of the exact integers; one point: false."""
    sx0, sy0, sx1, sy1, x, y = param_lines()
    want_short = raster.short32_reference(sx0, sy0, sx1, sy1)
    both_sides(want_short, "short32")
    point = (sx0 == sx1) & (sy0 == sy1)
    assert point.sum() >= MIN_SIDE
    # the bound the 32-bit branch is stated for: a fragment within 33 texels (and a rounding) of its line's box
    ex, ey = sx1 - sx0, sy1 - sy0
    assert (np.abs(16 * x - sx0)[want_short] < (1 << 14) + 48 * 16).all() and (np.abs(16 * y - sy0)[want_short] < (1 << 14) + 48 * 16).all()
    for v in (0, 1, (1 << 14) - 1, 1 << 14, (1 << 14) + 1):
        for e in (ex, ey):
            assert (e == v).sum() >= MIN_SIDE and (e == -v).sum() >= MIN_SIDE
    out = raster.param(sx0, sy0, sx1, sy1, x, y)
    ok, bits = raster.param_reference_batch(sx0, sy0, sx1, sy1, x, y)
    assert (ok == ~point).all()
    drawn = out[:, 5].view(np.int32) != 0x7fffffff                       # (dep_setup draws nothing between two equal positions)
    for k, s in enumerate((sx0, sy0, sx1, sy1)):
        assert (out[drawn, 5 + k].view(np.int32) == s[drawn]).all(), "dep_setup snapped endpoint word %d elsewhere" % k
    assert drawn[~point].all() and drawn[point].sum() >= MIN_SIDE        # (the nudged pairs: drawn, and snapped to one point)
    assert (out[drawn, 0] == want_short[drawn]).all(), "short32 is not |ex|, |ey| < 2^14"
    assert (out[~drawn, 0] == 0).all()
    assert (out[:, 1] == ok).all() and (out[:, 3] == ok).all(), "dep_param's verdict"
    bad = ok & (out[:, 2] != out[:, 4])
    assert not bad.any(), "the 32-bit and the 64-bit branch differ at line %d" % int(np.flatnonzero(bad)[0])
    bad = ok & (out[:, 2] != bits)
    assert not bad.any(), "t differs from the reference at line %d: %08x, reference %08x" % (
        int(np.flatnonzero(bad)[0]), int(out[np.flatnonzero(bad)[0], 2]), int(bits[np.flatnonzero(bad)[0]]))
    # a sample against the Python integers themselves
    for k in np.random.default_rng(1).integers(0, x.size, 300):
        want = raster.param_reference(sx0[k], sy0[k], sx1[k], sy1[k], x[k], y[k])
        assert (want is None) == (not ok[k]) and (want is None or want.view(np.uint32) == out[k, 2])
