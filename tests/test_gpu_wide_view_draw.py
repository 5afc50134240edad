"""draw() on views wide and tall enough to leave the rasteriser's 32-bit branches, against the CPU restatement (which divides in
exact 64-bit integers: oracle/tendrils_oracle.c ceil_div), through both pipelines: fragments, the flow field bit for bit, the
view's bytes.  `prev` and `cur` are drawn independently, so every line crosses the view: edges with |DX| >= 4096 or DY >= 1024
sixteenths (dep_raster_poly's 64-bit division on the slow list, bins_span_lines' fp64 estimate in the bins) and lines of 2^14
sixteenths and more (dep_param's 64-bit branch).  Which branch a line takes is derived here from its snapped extents, and every
case asserts that it holds at least 200 drawing lines of each class it is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import bits_equal

pytestmark = pytest.mark.gpu

MIN_LINES = 200
f32 = np.float32


def drawing_rows(n):
    """the rows of an n x n state whose line joins the row's own texel of `previous` and of `current` (th_stream.inc: the two
    vertices of the other rows read one texel of one buffer - no line), in the lookup's fp32 arithmetic"""
    draws = np.zeros(n, bool)
    for m in range(n):
        buf = []
        for j in (2 * m, 2 * m + 1):
            near = f32(j / (2 * n - 1)) * f32(n)
            fl = np.floor(near)
            assert int(np.clip(np.floor((fl / f32(n)) * f32(n)), 0, n - 1)) == m          # (no shape here drifts off its own row)
            buf.append(bool(near - fl > f32(0.25)))
        draws[m] = buf[0] != buf[1]
    return draws


def snap(clip, texels):
    """dep_snap of a clip-space coordinate on a target `texels` wide, operation by operation in fp32"""
    scale = f32(8.0) * f32(texels)
    return np.rint(np.asarray(clip, f32) * scale + (scale - f32(8.0))).astype(np.int64)


def lines_of(cur, prev, view, vs, width=1.0):
    """per particle of the drawing rows: the snapped extents |ex|, |ey| of its line and the rows its hexagon covers"""
    fw, fh = view
    draws = drawing_rows(cur.shape[0])
    a, b = prev[draws].reshape(-1, 4), cur[draws].reshape(-1, 4)
    ax, ay, bx, by = a[:, 0] * f32(vs[0]), a[:, 1] * f32(vs[1]), b[:, 0] * f32(vs[0]), b[:, 1] * f32(vs[1])
    ex, ey = np.abs(snap(bx, fw) - snap(ax, fw)), np.abs(snap(by, fh) - snap(ay, fh))
    hy = f32(0.5 * width) / (f32(0.5) * f32(fh))
    ymin, ymax = np.minimum(snap(ay - hy, fh), snap(by - hy, fh)), np.maximum(snap(ay + hy, fh), snap(by + hy, fh))
    rows = np.clip((ymax + 15) >> 4, None, fh) - np.clip((ymin + 15) >> 4, 0, None)
    return ex, ey, rows


def crossing_state(n, view, seed, m):
    fw, fh = view
    rng = np.random.default_rng(seed)
    vs = (1.0, fw / fh)
    prev, cur = np.zeros((n, n, 4), np.float32), np.zeros((n, n, 4), np.float32)
    for a in (prev, cur):
        a[..., 0] = rng.uniform(-m, m, (n, n)) / vs[0]
        a[..., 1] = rng.uniform(-m, m, (n, n)) / vs[1]
        a[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    return cur, prev, vs


RENDER_KEYS = ("speedLimit", "flowDecay", "speedAlpha", "colorMapAlpha", "baseColor", "flowColor")
TIME = 1500.0


@functools.lru_cache(maxsize=2)
def reference(oracle, key, n, view, seed, m, flow_w, view_w, dealt):
    """inputs and the restatement's results of one case (computed once, shared by the pipelines, left unchanged)"""
    if dealt:
        cur, prev, vs = dealt_state(n, view, seed)
    else:
        cur, prev, vs = crossing_state(n, view, seed, m)
    base = np.zeros((view[1], view[0], 4), np.float32)
    want_flow, frags = oracle.flow_deposit(cur, prev, base, TIME, view_size=vs, line_width=flow_w)
    return cur, prev, vs, want_flow, frags


def dealt_state(n, view, seed):
    """lines 2 texels across and 10.5 .. 13.5 texels up or down: hexagons of 11 to 14 rows around kMaxRowsDealt = 12"""
    fw, fh = view
    rng = np.random.default_rng(seed)
    vs = (1.0, fw / fh)
    prev = np.zeros((n, n, 4), np.float32)
    prev[..., 0] = rng.uniform(-0.7, 0.7, (n, n)) / vs[0]
    prev[..., 1] = rng.uniform(-0.5, 0.5, (n, n)) / vs[1]
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., 0] += (rng.choice([-2.0, 2.0], (n, n)) * 2.0 / fw / vs[0]).astype(np.float32)
    cur[..., 1] += (rng.choice([-1.0, 1.0], (n, n)) * rng.uniform(10.5, 13.5, (n, n)) * 2.0 / fh / vs[1]).astype(np.float32)
    cur[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    return cur, prev, vs


def pipeline_of(t):
    from tendrils_amd import _capi
    info = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(info))
    return int(info.pipeline)


def draw_and_compare(oracle, pipeline, n, view, cur, prev, vs, want_flow, frags, flow_w=1, view_w=1, widths=(1, 1)):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    opts["lineWidthRange"] = widths
    t = ta.Tendrils(View(*view), opts)
    t.resize()
    t.viewSize[:] = vs                       # (the tall views: positions are laid out for (1, fw / fh), as the restatement is told)
    t.setup(n)
    t.particles.draw_pipeline(pipeline)
    t.state.update(flowWidth=flow_w, lineWidth=view_w, autoClearView=False, autoFade=False)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.flow.set_pixels(np.zeros((view[1], view[0], 4), np.float32))
    t.timer.time = TIME
    t.renderView = True
    t.clearView()
    t.draw()
    assert pipeline_of(t) == {"stream": 0, "bins": 1}[pipeline]
    u = {k: v for k, v in t.state.items() if k in RENDER_KEYS}
    want_view, _ = oracle.view_render(cur, prev, np.zeros((view[1], view[0], 4), np.uint8), TIME, view_size=vs, line_width=view_w, **u)
    got_frags, got_flow, got_view = t.fragments, t.flow.read(), t.read_view()
    t.dispose()
    assert got_frags == frags
    same = bits_equal(got_flow, want_flow)
    assert same.all(), "%d texels of the flow field differ, the first at (x, y) = %s" % (
        (~same.all(axis=2)).sum(), tuple(int(v) for v in np.argwhere(~same.all(axis=2))[0][::-1]))
    assert (got_view == want_view).all() and want_view.any()


# n, view, seed, and the classes of lines the case is there for
CROSSING = {
    "2048x32": (48, (2048, 32), 1, ("x4096", "either2^14")),
    "32x2048": (48, (32, 2048), 2, ("y1024", "either2^14")),
    "640x360": (48, (640, 360), 3, ("x4096", "y1024")),
    "4096x16": (32, (4096, 16), 4, ("x4096", "either2^14")),
}


def classes(ex, ey):
    return {"x4096": ex >= 4096, "y1024": ey >= 1024, "either2^14": (ex >= (1 << 14)) | (ey >= (1 << 14))}


@pytest.mark.parametrize("pipeline", ["stream", "bins"])
@pytest.mark.parametrize("m", [0.97, 1.2])
@pytest.mark.parametrize("case", sorted(CROSSING))
def test_lines_across_wide_and_tall_views_equal_the_restatement(oracle, case, m, pipeline):
    """m = 0.97: the hexagons lie inside the view and are not small - dep_raster_poly<6> from the slow list, the span list in the
    bins; m = 1.2: they are clipped - dep_raster_poly<0> with long edges."""
    n, view, seed, wanted = CROSSING[case]
    cur, prev, vs, want_flow, frags = reference(oracle, case, n, view, seed, m, 1.0, 1.0, False)
    ex, ey, _ = lines_of(cur, prev, view, vs)
    have = classes(ex, ey)
    for name in wanted:
        assert have[name].sum() >= MIN_LINES, (name, int(have[name].sum()))
    assert frags > 100_000
    draw_and_compare(oracle, pipeline, n, view, cur, prev, vs, want_flow, frags)


@pytest.mark.parametrize("pipeline", ["stream", "bins"])
@pytest.mark.parametrize("flow_w", [5, 64])
def test_wide_lines_around_two_to_the_fourteen(oracle, flow_w, pipeline):
    """dep_param's bound - a fragment within 33 texels of its line - on lines just under and over 2^14 sixteenths: 2048 x 32,
    flowWidth 5 and 64, lineWidth 3"""
    n, view, seed = 48, (2048, 32), 5
    cur, prev, vs, want_flow, frags = reference(oracle, "wide", n, view, seed, 0.97, float(flow_w), 3.0, False)
    ex, ey, _ = lines_of(cur, prev, view, vs, flow_w)
    long = (ex >= (1 << 14)) | (ey >= (1 << 14))
    assert long.sum() >= MIN_LINES and (~long).sum() >= MIN_LINES
    near = (ex >= (1 << 14) - 2048) & (ex < (1 << 14) + 2048)               # within 128 texels of the limit, on either side
    assert (near & long).sum() >= 20 and (near & ~long).sum() >= 20
    draw_and_compare(oracle, pipeline, n, view, cur, prev, vs, want_flow, frags, flow_w=flow_w, view_w=3, widths=(1, 64))


@pytest.mark.parametrize("pipeline", ["stream", "bins"])
def test_hexagons_of_eleven_to_fourteen_rows(oracle, pipeline):
    """kMaxRowsDealt = 12 (th_bins.hip bins_fused_kernel): small hexagons of up to 12 rows have their rows dealt to the wave's
    lanes (dep_hexagon_row_span), taller ones walk their own (dep_raster_small_hexagon2) - the same texels either way"""
    n, view, seed = 32, (64, 64), 6
    cur, prev, vs, want_flow, frags = reference(oracle, "dealt", n, view, seed, 0.0, 1.0, 1.0, True)
    ex, ey, rows = lines_of(cur, prev, view, vs)
    assert (ex < 4096 - 16).all() and (ey < 1024 - 16).all()                # (small hexagons, all of them)
    for r in (11, 12, 13, 14):
        assert (rows == r).sum() >= 10, (r, int((rows == r).sum()))
    assert (rows <= 12).sum() >= 100 and (rows > 12).sum() >= 100         # (dealt / walked)
    draw_and_compare(oracle, pipeline, n, view, cur, prev, vs, want_flow, frags)
