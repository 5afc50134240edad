"""The binned draw()'s ordering routines (th_bins.hip) at the fragment counts where one hands over to the next, with every
position of every run visible in the result.

The crowded tests that came before this module draw velocities that make four fragments in ten opaque: only the last place
or two of a run shows in the flow field (tests/test_planted_runs.py states that as a number).  Here the runs are PLANTED
(tests/planted_runs.py): a plan says how many fragments each texel receives - exactly the limits kBinCap = 4096 (the large
bins), kRankMaxRun = kOwnRun = kWaveRun = 256, kGiantRun = 1024, kCrowdCap = kGiantWindow = 2048, one less and one more - and a
layout is drawn once per WINDOW of 64 run positions, with velocities under which exchanging any two neighbours inside the
window changes the texel's bits (pinned on the CPU restatement: tests/test_planted_runs.py).  One context per layout draws
all velocity sets one after the other - the page store is used again over the same keys - and every draw is compared with
the restatement bit for bit; th_draw_query's crowded_fragments pins which side of kBinCap every bin fell on.

    A        ordinary bins of 1, 255, 256, 257, 4095, 4096 places, every run <= 256: bins_blend_kernel's counting rank, its
             rounds of 256 places; the 4096 bin sits at kBinCap and at kRankMaxRun at once
    B        {256, 5, 5}: ranked by counting | {5, 257, 5}: bin_crowded, one batch through bin_bitonic, the 257-run by
             bin_blend_long and the 5-runs by bin_blend_own in the same batch
    C_2048   8 x 256 | 257, 1791: bin_crowded's first batch is exactly kCrowdCap and ranked by counting, the second bitonic
    C_2047   7 x 256 + 255 | 257 | 1792: the same one off
    C_pad    bin_bitonic's padding: batches of 2048 (none), 2047, 1025 (to 2048), and a bin {2000 | 60, 5 | 2000} (a batch of
             65 fragments between two full ones: its longest run is 60 - ranked by counting, as any batch that short must be)
    D        blend_texel_windows inside an ordinary bin: {3, 2049, 3} (batches on both sides of the windowed texel), {4096},
             {2048, 2048} (each texel a batch alone)
    E1       a large bin of 17 x 241 = 4097: crowd_sort_kernel / crowd_walk_kernel alone
    E2       a large bin {1, 255, 256 | 257, 1023, 1024 | 1025, 2048 | 2049}: crowd_sort, long_sort_kernel, giants of one and
             of two windows (giant_part / giant_sort), run_walk_kernel
    E3       large bins {4097} and {4096, 1}
    E4       an ordinary bin of 4096 beside a large one of 4097 in the same draw
    F_B, F_E2   B and E2 on a 50 x 20 target (partial bins in both directions)
    G        the giants' fallback: a run with more than kGiantWindow stream indices in one of giant_part_kernel's buckets
             (2048 x 2048 state) goes to crowd_blend_kernel, whose windows narrow
Every layout is drawn with its particles taken at random from the whole state ("spread": every list of a bin is used) and as
consecutive slots ("rows": a workgroup reserves its places in a bin at a stroke, on and across the 256-place pages)."""
import ctypes as C

import numpy as np
import pytest

import planted_runs as pr
from helpers import bits_equal

pytestmark = pytest.mark.gpu

RENDER = dict(speedLimit=pr.SPEED_LIMIT, flowDecay=0.005, speedAlpha=0.000001, colorMapAlpha=0.0,
              baseColor=[1, 0.6, 0.2, 0.07], flowColor=[0.3, 1, 0.8, 0.3])


def make(n, view, pipeline):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    t = ta.Tendrils(View(*view))
    t.resize()
    t.setup(n)
    assert tuple(t.viewSize) == pr.view_size(view)
    for k, v in RENDER.items():
        t.state[k] = v
    t.particles.draw_pipeline(pipeline)
    t.timer.time = pr.TIME
    t.renderView = False
    return t


def query(t):
    from tendrils_amd import _capi
    info = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(info))
    return int(info.pipeline), int(info.fragments), int(info.crowded_fragments)


_flow = {}


def inputs(oracle, lay, key, k):
    """velocity set k of a layout: both buffers and the restatement's flow field (computed once per session)"""
    cur, prev = pr.velocities(lay, k)
    if (key, k) not in _flow:
        want, frags = pr.deposit(oracle, cur, prev, lay.base(), lay.view)
        assert frags == lay.fragments
        _flow[key, k] = want
    return cur, prev, _flow[key, k]


def upload(t, lay, cur, prev):
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.flow.set_pixels(lay.base())


def draw_flow(t, lay, cur, prev, want, pipeline=1):
    """one draw of the flow pass, from the base field: fragments, bits, pipeline, which bins were large"""
    upload(t, lay, cur, prev)
    t.draw()
    got = t.flow.read()
    crowded = pr.crowded_fragments(lay.view, lay.plan) if pipeline == 1 else 0
    assert t.fragments == lay.fragments
    same = bits_equal(got, want).all(-1)
    assert same.all(), [(int(x), int(y)) for y, x in np.argwhere(~same)]
    assert query(t) == (pipeline, lay.fragments, crowded), query(t)


# ---- what each layout is named for, asserted from its plan -----------------------------------------------------------------
def main_bins(name):
    """the bins of a layout in reading order, without the bins that only hold a corner's little run"""
    view, plan = pr.LAYOUTS[name]
    return [v for _, v in sorted(pr.bins_of(view, plan).items(), key=lambda b: (b[0][1], b[0][0])) if sum(v) > 3]


def check_A(bins):
    assert sorted(sum(b) for b in bins + [[1]]) == [1, 255, 256, 257, 4095, 4096]          # (the bin of 1 is a corner's)
    assert max(max(b) for b in bins) == pr.RANK_MAX_RUN and [256] * 16 in bins and [256] * 15 + [255] in bins
    assert all(sum(b) <= pr.BIN_CAP for b in bins)


def check_B(bins):
    assert bins == [[256, 5, 5], [5, 257, 5]]
    assert max(bins[0]) == pr.RANK_MAX_RUN and max(bins[1]) == pr.RANK_MAX_RUN + 1 and pr.batches(bins[1]) == [[5, 257, 5]]


def check_C_2048(bins):
    (b,) = bins
    first, second = pr.batches(b)
    assert sum(b) == pr.BIN_CAP and sum(first) == pr.CROWD_CAP and max(first) <= pr.RANK_MAX_RUN      # the counting branch of bin_crowded
    assert second == [257, 1791] and sum(second) == pr.CROWD_CAP                                      # bitonic, no padding


def check_C_2047(bins):
    (b,) = bins
    first, second, third = pr.batches(b)
    assert sum(b) == pr.BIN_CAP and sum(first) == pr.CROWD_CAP - 1 and max(first) <= pr.RANK_MAX_RUN
    assert second == [257] and third == [1792]


def check_C_pad(bins):
    assert [pr.batches(b) for b in bins] == [[[300, 1748]], [[257, 1790]], [[1025]], [[2000], [60, 5], [2000]]]
    assert [sum(b) for b in bins[:3]] == [2048, 2047, 1025] and all(sum(b) <= pr.BIN_CAP and max(b) > pr.RANK_MAX_RUN for b in bins)


def check_D(bins):
    assert [pr.batches(b) for b in bins] == [[[3], [None, 2049], [3]], [[None, 4096]], [[2048], [2048]]]
    assert all(sum(b) <= pr.BIN_CAP for b in bins)


def check_E1(bins):
    assert bins == [[241] * 17] and sum(bins[0]) == pr.BIN_CAP + 1 and max(bins[0]) <= pr.RANK_MAX_RUN


def check_E2(bins):
    (b,) = bins
    assert sum(b) > pr.BIN_CAP
    assert sorted(l for l in b if l <= pr.RANK_MAX_RUN) == [1, 255, 256]                                # crowd_sort / crowd_walk
    assert sorted(l for l in b if pr.RANK_MAX_RUN < l <= pr.GIANT_RUN) == [257, 1023, 1024]             # long_sort / run_walk
    assert sorted(l for l in b if l > pr.GIANT_RUN) == [1025, 2048, 2049]                               # giants: one window, one, two


def check_E3(bins):
    assert bins == [[4097], [4096, 1]]


def check_E4(bins):
    assert bins == [[256] * 16, [256] * 16 + [1]] and sum(bins[0]) == pr.BIN_CAP and sum(bins[1]) == pr.BIN_CAP + 1


CHECKS = dict(A=check_A, B=check_B, C_2048=check_C_2048, C_2047=check_C_2047, C_pad=check_C_pad, D=check_D, E1=check_E1,
              E2=check_E2, E3=check_E3, E4=check_E4, F_B=check_B, F_E2=check_E2)
CROWDED = dict(A=0, B=0, C_2048=0, C_2047=0, C_pad=0, D=0, E1=4097, E2=7938, E3=8194, E4=4097, F_B=0, F_E2=7938)


@pytest.mark.parametrize("ids", ["spread", "rows"])
@pytest.mark.parametrize("name", sorted(pr.LAYOUTS))
def test_every_position_of_every_run_is_blended_in_order(oracle, name, ids):
    """one context, one draw per window of the layout's longest run: every draw's fragments, flow bits, pipeline and large bins"""
    CHECKS[name](main_bins(name))
    view, plan = pr.LAYOUTS[name]
    assert pr.crowded_fragments(view, plan) == CROWDED[name]
    lay = pr.planted(oracle, name, ids)
    t = make(lay.n, lay.view, "bins")
    try:
        for k in range(lay.draws):
            draw_flow(t, lay, *inputs(oracle, lay, (name, ids), k))
    finally:
        t.dispose()


def view_alone(t):
    from tendrils_amd import _capi
    u, n = t.render_uniforms(), C.c_uint64(0)
    _capi.call("th_view_draw", t.particles._ctx, C.byref(u), C.byref(n))
    return int(n.value)


@pytest.mark.parametrize("ids", ["spread", "rows"])
@pytest.mark.parametrize("name", ["B", "C_2048", "C_2047", "C_pad", "E2", "E3"])
def test_view_target_alone_and_both_targets_in_one_pass(oracle, name, ids):
    """the same runs into the RGBA8 view buffer - alone (MODE 1), and with the flow field in one pass (MODE 2: two varyings a
    fragment, the giants walked by two waves a run) - at the first, a middle and the last velocity set: the view's bytes against
    the restatement's view pass, the flow's bits as before"""
    lay = pr.planted(oracle, name, ids)
    blank = np.zeros((lay.view[1], lay.view[0], 4), np.uint8)
    t = make(lay.n, lay.view, "bins")
    try:
        for k in (0, lay.draws // 2, lay.draws - 1):
            cur, prev, want = inputs(oracle, lay, (name, ids), k)
            want_view, frags = oracle.view_render(cur, prev, blank, pr.TIME, view_size=pr.view_size(lay.view), **RENDER)
            assert frags == lay.fragments and want_view.any()
            upload(t, lay, cur, prev)
            t.clearView()
            assert view_alone(t) == lay.fragments
            assert (t.read_view() == want_view).all() and bits_equal(t.flow.read(), lay.base()).all()
            assert query(t) == (1, lay.fragments, CROWDED[name])
            t.clearView()
            t.renderView = True
            draw_flow(t, lay, cur, prev, want)
            t.renderView = False
            assert t.view_fragments == lay.fragments and (t.read_view() == want_view).all()
    finally:
        t.dispose()


@pytest.mark.parametrize("name", ["B", "E2"])
def test_stream_ordered_pipeline_sees_the_same_order(oracle, name):
    """the stream-ordered pipeline (a stable radix sort by texel, a gather, the same blend) over the same velocity sets"""
    lay = pr.planted(oracle, name, "spread")
    t = make(lay.n, lay.view, "stream")
    try:
        for k in range(lay.draws):
            draw_flow(t, lay, *inputs(oracle, lay, (name, "spread"), k), pipeline=0)
    finally:
        t.dispose()


def test_giants_fallback_windows_that_narrow(oracle):
    """Case G (planted_runs.giant_fallback): 4164 fragments on one texel, 2050 of them in the first of giant_part_kernel's
    buckets.  The first window, two in the middle and the last."""
    lay, most, shift = pr.giant_fallback(oracle)
    m, i = lay.runs[0]
    stream = i.astype(np.int64) * lay.n + m
    assert lay.n * lay.n >= 1 << 22 and stream.max() - stream.min() >= (1 << 22) - (1 << 12) and shift == 12
    assert most > pr.CROWD_CAP and lay.fragments > pr.BIN_CAP               # giant_part_kernel refuses: most > kGiantWindow
    assert np.count_nonzero(stream < (1 << shift)) > pr.CROWD_CAP           # ... and so must blend_texel_windows' first 4096-wide bucket
    t = make(lay.n, lay.view, "bins")
    try:
        for k in pr.giant_sets(lay):
            cur, prev = pr.velocities(lay, k)
            want, frags = pr.deposit(oracle, cur, prev, lay.base(), lay.view)
            assert frags == lay.fragments
            draw_flow(t, lay, cur, prev, want)
    finally:
        t.dispose()
