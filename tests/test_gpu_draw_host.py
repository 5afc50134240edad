"""The host code every draw() goes through (tendrils_amd/csrc/th_draw.hip, the draw half of th_shard.hip, the loop of
th_drawprog.hip): what the neighbouring suites leave between them.  test_gpu_binned_draw.py has the pool's growth, bins_pages < 0
and crowded shares; test_gpu_loopback.py the sharded paths and the injected failures; test_gpu_view.py draw_reuse.  Here: a frame
whose first binned pass gives up, the four callers of the pass loop side by side, both blend topologies of the binned pass, and the
refusals' texts.  Everything is compared on the bits with the oracle or with the other pipeline; what a pass reports
(th_draw_query) is asserted as the constants the library printed before its draw host was folded (profiles/draw_host.txt)."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal
from test_gpu_draw_program import make, program_uniforms, programs  # noqa: F401
from test_gpu_loopback import inputs
from test_gpu_loopback import make as band_context

pytestmark = pytest.mark.gpu

BINS, STREAM = 1, 0          # th_draw_info.pipeline: TH_DRAW_BINS, TH_DRAW_STREAM
RENDER = dict(speedLimit=0.01, flowDecay=0.005, speedAlpha=0.5, colorMapAlpha=0.0, baseColor=[1, 0.6, 0.2, 0.5], flowColor=[0.3, 1, 0.8, 0.4])


def query(t):
    from tendrils_amd import _capi
    q = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(q))
    return int(q.pipeline), int(q.fragments), int(q.crowded_fragments)


def slot_order(t):
    from tendrils_amd import _capi
    info = _capi.SlotOrderInfo()
    _capi.call("th_slot_order", t.particles._ctx, C.byref(info))
    return int(info.sorted_buffers), int(info.sorts)


def context(n, view, cur, prev, base, time, **options):
    t = make(n, view, (1.0, view[0] / view[1]), **options)
    t.state.update(RENDER)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.flow.set_pixels(base)
    t.timer.time = time
    t.line_widths()
    return t


def flow_deposit(t):
    return t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"])


def view_draw(t):
    from tendrils_amd import _capi
    u, n = t.render_uniforms(), C.c_uint64(0)
    _capi.call("th_view_draw", t.particles._ctx, C.byref(u), C.byref(n))
    return int(n.value)


def draw_both(t):
    from tendrils_amd import _capi
    d = _capi.DepositUniforms(time=float(t.timer.time), speedLimit=float(t.state["speedLimit"]))
    d.viewSize[0], d.viewSize[1] = float(t.viewSize[0]), float(t.viewSize[1])
    u, n = t.render_uniforms(), C.c_uint64(0)
    _capi.call("th_draw", t.particles._ctx, C.byref(d), C.byref(u), C.byref(n))
    return int(n.value)


def oracle_frame(oracle, cur, prev, base, time, view):
    """(flow, view image, fragments) of both passes over fresh targets"""
    size = (1.0, view[0] / view[1])
    flow, n = oracle.flow_deposit(cur, prev, base, time, view_size=size, speedLimit=RENDER["speedLimit"])
    image, k = oracle.view_render(cur, prev, np.zeros((view[1], view[0], 4), np.uint8), time, view_size=size, **RENDER)
    assert n == k
    return flow, image, n


@pytest.fixture(scope="module")
def crowded(oracle):
    """256 x 256 particles within 0.15 of the middle of a 96 x 54 view: bins of tens of thousands of fragments"""
    view = (96, 54)
    cur, prev, base = inputs(256, view, 97, 0.15)
    return view, cur, prev, base, oracle_frame(oracle, cur, prev, base, 2500.0, view)


# ---- 1. one frame, one pipeline, after a give-up ----------------------------------------------------------------------------------
def test_a_frame_whose_first_binned_pass_gives_up_stays_stream_ordered(oracle, crowded, monkeypatch):
    """TH_DRAW=bins (the policy, counted in frames - th_draw_pipeline would ask every pass anew) and lists of two pages - the
    fewest the option takes - that may not widen: the flow pass's bins give up before anything is blended, the pass is repeated
    in stream order, and the view pass of the same frame does not try the bins.  After a step the next frame asks the policy
    again: uncrowded lines go through the bins, in both passes."""
    monkeypatch.setenv("TH_DRAW", "bins")
    view, cur, prev, base, (want_flow, want_view, want_n) = crowded
    t = context(256, view, cur, prev, base, 2500.0)
    t.particles.option("bins_pages", -2)
    n = flow_deposit(t)
    first = query(t)
    k = view_draw(t)
    second = query(t)
    got_flow, got_view = t.flow.read(), t.read_view()
    print("give-up frame: flow pass %r, view pass %r" % (first, second))
    assert n == k == want_n and first == second == (STREAM, want_n, 0)
    assert bits_equal(got_flow, want_flow).all()
    assert (got_view == want_view).all() and got_view.any()
    # the next frame: lines all over the view (no list outgrows its page)
    t.timer.tick()
    t.step()
    after_step = slot_order(t)
    cur2, prev2, base2 = inputs(256, view, 98, 0.9)
    t.particles.upload_texels(cur2, 0)
    t.particles.upload_texels(prev2, 1)
    t.flow.set_pixels(base2)
    t.clearView()
    want_flow, want_view, want_n = oracle_frame(oracle, cur2, prev2, base2, t.timer.time, view)
    n = flow_deposit(t)
    first = query(t)
    k = view_draw(t)
    second = query(t)
    print("next frame: slot order after the step %r, flow pass %r, view pass %r" % (after_step, first[:1], second[:1]))
    assert n == k == want_n
    assert (after_step, first[0], second[0]) == NEXT_FRAME
    assert bits_equal(t.flow.read(), want_flow).all()
    assert (t.read_view() == want_view).all()
    t.dispose()


NEXT_FRAME = ((0, 0), BINS, BINS)          # (sorted buffers, sorts) after the step; the pipelines of the next frame's two passes


# ---- 2. the four callers of the pass loop agree -------------------------------------------------------------------------------------
# the pipeline each pass reports, by policy: the same for one width and for two (lines up to 2 wide stay with the bins)
REPORTED = dict(auto=BINS, bins=BINS, stream=STREAM)


@pytest.fixture(scope="module")
def stepped():
    """64 x 64 particles over a 40 x 40 view, one step on: the ring of a context whose integrator runs over sorted slots"""
    rng = np.random.default_rng(5)
    st = np.zeros((64, 64, 4), np.float32)
    st[..., :2] = rng.uniform(-0.9, 0.9, (64, 64, 2))
    st[..., 2:] = rng.uniform(-.008, .008, (64, 64, 2))
    base = np.zeros((40, 40, 4), np.float32)
    base[..., :2] = rng.uniform(-.01, .01, (40, 40, 2))
    base[..., 3] = rng.uniform(0, 1, (40, 40))
    return st, base


def sorted_context(st, base, policy, widths):
    options = dict(lineWidthRange=(1, 2)) if widths else {}
    t = make(64, (40, 40), (1.0, 1.0), **options)
    assert t.particles.option("bucket", 1) == 1
    t.particles.draw_pipeline(policy)
    t.state.update(RENDER)
    if widths:
        t.state["flowWidth"], t.state["lineWidth"] = widths
    t.particles.upload_texels(st)
    t.timer.time = 1000.0
    t.timer.tick()
    t.step()
    assert slot_order(t)[0] > 0
    t.flow.set_pixels(base)
    t.line_widths()
    return t


@pytest.mark.parametrize("widths", [None, (2, 1)], ids=["one_width", "two_widths"])
def test_the_callers_of_the_pass_loop_agree(oracle, programs, stepped, widths):
    """th_draw (two widths: its two-rasterisation branch), th_flow_deposit + th_view_draw and the library's two stages restated as
    draw programs, under each policy: one flow field, one view image, one fragment count; each pass on the pipeline its policy names"""
    from tendrils_amd import _capi
    st, base = stepped
    outs, reported = [], {}
    for policy in ("auto", "bins", "stream"):
        for how in ("th_draw", "two passes", "programs"):
            t = sorted_context(st, base, policy, widths)
            if how == "th_draw":
                n = draw_both(t)
                pipes, k = (query(t)[0],), query(t)[1]          # (two widths: the count it returns is the flow pass's, the last pass the view's)
            elif how == "two passes":
                n = flow_deposit(t)
                pipes = (query(t)[0],)
                k = view_draw(t)
                pipes += (query(t)[0],)
            else:
                u = dict(program_uniforms(t), sinTerm=t.render_uniforms().sinTerm)
                n = t._draw_program(programs["flow"], _capi.TH_PASS_FLOW, u)
                pipes = (query(t)[0],)
                k = t._draw_program(programs["view"], _capi.TH_PASS_VIEW, u)
                pipes += (query(t)[0],)
            reported[policy, how] = pipes
            frags = query(t)[1]
            flow, image = t.flow.read(), t.read_view()
            outs.append((policy, how, flow, image, n, k, frags, t.particles.read(0), t.particles.read(1), t.timer.time))
            t.dispose()
    print("pass loop, %s: pipelines %r" % ("widths %r" % (widths,) if widths else "one width", reported))
    for (policy, how), pipes in reported.items():
        assert set(pipes) == {REPORTED[policy]}, (policy, how, pipes)
    _, _, flow, image, n, k, _, cur, prev, time = outs[0]
    assert n > 1000 and image.any() and (n == k or widths)
    for policy, how, f, i, nn, kk, frags, c, p, _ in outs[1:]:
        assert (nn, kk) == (n, k) and frags == kk, (policy, how)
        assert bits_equal(f, flow).all() and (i == image).all(), (policy, how)
        assert bits_equal(c, cur).all() and bits_equal(p, prev).all()
    if not widths:          # (lines one texel wide: what the restatement pins)
        want_flow, want_view, want_n = oracle_frame(oracle, cur, prev, base, time, (40, 40))
        assert n == want_n and bits_equal(flow, want_flow).all() and (image == want_view).all()


# ---- 3. both blend topologies ---------------------------------------------------------------------------------------------------------
def test_both_blend_topologies_equal_the_oracle(crowded):
    """the same crowded draw twice through the bins: the first has no crowded draw behind it and sends the ordinary bins' blend
    out early, beside the totals' read-back; the second sees more than half of the last draw's fragments in crowded bins and
    keeps the crowded bins' chain on the main stream (th_draw.hip: kEarlyBlendShare)"""
    view, cur, prev, base, (want_flow, want_view, want_n) = crowded
    t = context(256, view, cur, prev, base, 2500.0)
    t.particles.draw_pipeline("bins")
    shares = []
    for _ in range(2):
        t.flow.set_pixels(base)
        t.clearView()
        n = draw_both(t)
        pipe, frags, crowd = query(t)
        shares.append(crowd / max(frags, 1))
        assert pipe == BINS and n == frags == want_n
        assert bits_equal(t.flow.read(), want_flow).all()
        assert (t.read_view() == want_view).all()
    print("blend topologies: crowded share of draw 1 and 2: %r of %d fragments" % (shares, want_n))
    assert shares[0] > 0.5 and shares[1] == shares[0]
    t.dispose()


# ---- 4. the refusals' texts -------------------------------------------------------------------------------------------------------------
HALO = ("a line of this row band looks up a particle row outside the band (rows 53..100 of 100) and no halo row was supplied "
        "(th_deposit_set_halo)")
SHARED = "the two passes of one draw share viewSize, time and speedLimit"


def refused(call):
    from tendrils_amd import _capi
    with pytest.raises(_capi.TendrilsHipError) as e:
        call()
    text = str(e.value)
    assert text.startswith("tendrils_hip status %d: " % e.value.status)
    return e.value.status, text.split(": ", 1)[1]


@pytest.fixture()
def band():
    """rows 53..100 of 100 x 100 particles: the vertices of row 53 read the row above, which this band does not hold"""
    n, view = 100, (16, 9)
    cur, prev, base = inputs(n, view, 1236)
    t = band_context(n, view, cur, prev, base, (53, 47))
    yield t
    t.dispose()


def test_a_band_without_halo_rows_is_refused_with_one_text(band):
    """th_deposit_emit, and both passes of th_draw_sharded in a world of ONE rank over loopback (which exchanges no halo rows): the
    error is the same text, and it survives the count exchange word for word.
    n = 100, rows 53..100: the stream-ordered count fetches both vertices of every line and meets row 53's, which read row 52.
    The binned pass walks only the slots whose lines can draw (th_bins.hip: slot_particle, row_draws) - and both vertices of rows 53
    and 59 read the SAME texel of `current`: lines without length, never set up, so dep_fetch never reports them.  Through the bins
    the text is reached where a line that draws reads across the edge: n = 41, whose rows 1, 2, 4, 8 and 16 are drawn from the row
    above (previous -> current of row m - 1), in a band that begins at row 8."""
    from tendrils_amd import _capi, sharding
    t = band
    assert refused(lambda: sharding.emit_fragments(t)) == (_capi.TH_ERR_UNSUPPORTED, HALO)
    sharding.comm_join(t.particles._ctx, sharding.loopback_id(), 0, 1)
    t.particles.draw_pipeline("stream")
    for view in (False, True):
        assert refused(lambda: sharding.draw_sharded_native(t, view=view)) == (_capi.TH_ERR_UNSUPPORTED, HALO)
        assert query(t) == (STREAM, 0, 0)
    n, view = 41, (16, 9)
    assert drawn_from_the_row_above(n) == [1, 2, 4, 8, 16]
    cur, prev, base = inputs(n, view, 1237)
    b = band_context(n, view, cur, prev, base, (8, 33))
    b.particles.draw_pipeline("bins")
    sharding.comm_join(b.particles._ctx, sharding.loopback_id(), 0, 1)
    for view in (False, True):
        assert refused(lambda: sharding.draw_sharded_native(b, view=view)) == (_capi.TH_ERR_UNSUPPORTED, HALO.replace("53..100 of 100", "8..41 of 41"))
        assert query(b)[0] == STREAM            # (no binned pass has finished: bins_pass_finish alone reports TH_DRAW_BINS)
    assert bits_equal(b.flow.read(), base).all()
    b.dispose()


def drawn_from_the_row_above(n):
    """the rows of an n x n texture whose lines have a length and are made of ANOTHER row's texels (th_stream.inc in numpy's fp32)"""
    uvy = (np.arange(2 * n) * (1.0 / (max(2 * n, 2) - 1))).astype(np.float32)
    near = uvy * np.float32(n)
    fl = np.floor(near)
    from_cur = (near - fl) > np.float32(0.25)
    row = np.clip(np.floor((fl / np.float32(n)).astype(np.float32) * np.float32(n)), 0, n - 1).astype(int)
    m = np.arange(n)
    draws = ~((row[0::2] == row[1::2]) & (from_cur[0::2] == from_cur[1::2]))
    return np.flatnonzero(draws & ((row[0::2] != m) | (row[1::2] != m))).tolist()


def test_a_band_is_refused_by_each_local_entry_point_in_its_own_words(band, programs):
    from tendrils_amd import _capi
    t = band
    base = t.flow.read()
    texts = {
        "th_draw": "draw on a row-band shard (47 of 100 rows): the passes go through th_deposit_emit / th_deposit_merge and "
                   "th_view_emit / th_view_merge with the owners' exchange in between",
        "th_flow_deposit": "flow deposit on a row-band shard (47 of 100 rows): use th_deposit_emit / th_deposit_merge with the "
                           "exchange of tendrils_amd/sharding.py",
        "th_view_draw": "view pass on a row-band shard (47 of 100 rows): use th_view_emit / th_view_merge with the owners' "
                        "exchange in between",
        "th_draw_program_run": "draw program on a row-band shard (47 of 100 rows): a band's pass goes through the owners' "
                               "exchange, which carries the built-in stages alone",
    }
    calls = {
        "th_draw": lambda: draw_both(t),
        "th_flow_deposit": lambda: flow_deposit(t),
        "th_view_draw": lambda: view_draw(t),
        "th_draw_program_run": lambda: t._draw_program(programs["flow"], _capi.TH_PASS_FLOW, program_uniforms(t)),
    }
    for name, call in calls.items():
        assert refused(call) == (_capi.TH_ERR_UNSUPPORTED, texts[name]), name
    assert bits_equal(t.flow.read(), base).all()


def test_passes_that_disagree_on_the_time_are_refused(band):
    from tendrils_amd import _capi
    n, view = 64, (40, 40)
    cur, prev, base = inputs(n, view, 3)
    whole = context(n, view, cur, prev, base, 2500.0)
    for t, entry in ((whole, "th_draw"), (band, "th_draw_emit")):
        d = _capi.DepositUniforms(time=float(t.timer.time), speedLimit=float(t.state["speedLimit"]))
        d.viewSize[0], d.viewSize[1] = float(t.viewSize[0]), float(t.viewSize[1])
        u, count, keys, colors = t.render_uniforms(), C.c_uint64(0), C.c_void_p(), C.c_void_p()
        u.time = d.time + 1.0
        rest = (C.byref(count),) if entry == "th_draw" else (C.byref(count), C.byref(keys), C.byref(colors))
        assert refused(lambda: _capi.call(entry, t.particles._ctx, C.byref(d), C.byref(u), *rest)) == (_capi.TH_ERR_INVALID, SHARED), entry
    assert bits_equal(whole.flow.read(), base).all()
    whole.dispose()
