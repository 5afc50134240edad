"""Draw programs through the binned draw() pipeline (tendrils_amd/csrc/th_drawprog.hip, th_bins.hip: the PROGRAM instantiations,
th_draw_prelude.inc: th_draw_vertex_slots_kernel).  A program pass takes the bins where the built-in pass of the same
context would, and leaves a tile-sorted ring in its slot order.  Everything is compared on the bits, against the stream-ordered
program pass, the library's own stages and the oracle; the policy is forced, so nothing here depends on what `auto` chooses.
Shapes: 64 x 64 particles; a 40 x 40 view where the step must run over sorted slots (the state needs twice the flow's texels),
96 x 54 where it need not."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal, golden, load
from test_deposit_oracle import deposit_inputs
from test_gpu_draw_program import (INERT, builtin_view, flow_pass, make, program_uniforms, programs, random_lines,  # noqa: F401
                                   stream_states, tap, view_frame)

pytestmark = pytest.mark.gpu

BINS, STREAM = 1, 0          # th_draw_info.pipeline: TH_DRAW_BINS, TH_DRAW_STREAM


def pipeline(t):
    from tendrils_amd import _capi
    q = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(q))
    return q.pipeline, q.fragments, q.crowded_fragments


def sorted_buffers(t):
    from tendrils_amd import _capi
    info = _capi.SlotOrderInfo()
    _capi.call("th_slot_order", t.particles._ctx, C.byref(info))
    return info.sorted_buffers


def lookups_are_local(n):
    """does every vertex of every line of an n x n texture read the line's own texel?  (th_stream.inc in numpy's fp32)"""
    uvx = (np.arange(n) * (1.0 / (max(n, 2) - 1))).astype(np.float32)
    uvy = (np.arange(2 * n) * (1.0 / (max(2 * n, 2) - 1))).astype(np.float32)
    row = tap(np.floor(uvy * np.float32(n)) / np.float32(n), n)
    return bool((tap(uvx, n) == np.arange(n)).all() and (row == np.arange(2 * n) // 2).all())


def forced(which):
    return lambda t: t.particles.draw_pipeline(which)


def program_pass(cur, prev, base, time, view_res, program, which, view_size=None, speed_limit=None, render=None, prepare=None, **options):
    """flow_pass of test_gpu_draw_program with the policy forced, and the pipeline the pass reports: (flow, fragments, pipeline)"""
    t = make(cur.shape[0], view_res, view_size, speed_limit, renderView=False, flowShader=program, **options)
    t.particles.draw_pipeline(which)
    if prepare:
        prepare(t)
    t.uniforms["render"].update(render or {})
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.flow.set_pixels(base)
    t.timer.time = time
    t.draw()
    out = t.flow.read(), t.fragments, pipeline(t)[0]
    t.dispose()
    return out


def spread_state(n, seed, spread=0.9, far=0.0):
    """positions over the view, velocities small; `far`: that share of the particles outside the view, at 1.1 < |x| < 1.9"""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, n, 4), np.float32)
    st[..., :2] = rng.uniform(-spread, spread, (n, n, 2))
    st[..., 2:] = rng.uniform(-.008, .008, (n, n, 2))
    if far:
        out = rng.random((n, n)) < far
        st[out, 0] = (rng.uniform(1.1, 1.9, (n, n)) * rng.choice([-1.0, 1.0], (n, n)))[out]
    return st


def sorted_loop(st, frames=3, view=(40, 40), render=None, **options):
    """a context with bins forced after `frames` x (tick, step, draw) minus the last draw: the ring lies in tile-sorted slots"""
    t = make(st.shape[0], view, **options)
    t.uniforms["render"].update(render or {})
    assert t.particles.option("bucket", 1) == 1
    t.particles.draw_pipeline("bins")
    t.state["speedAlpha"] = 0.0005
    t.particles.upload_texels(st)
    t.timer.time = 1000.0
    for k in range(frames):
        t.timer.tick()
        t.step()
        if k + 1 < frames:
            t.draw()
    assert sorted_buffers(t) > 0
    return t


def twin(t, cur, prev, **options):
    """a stream-ordered context fed the ring, the flow, the clock and the state of `t`"""
    s = make(cur.shape[0], tuple(t.viewRes), **options)
    s.particles.draw_pipeline("stream")
    s.state.update({k: v for k, v in t.state.items()})
    s.uniforms["render"].update(t.uniforms["render"])
    s.particles.upload_texels(cur, 0)
    s.particles.upload_texels(prev, 1)
    s.flow.set_pixels(t.flow.read())
    s.timer.time = t.timer.time
    s.line_widths()
    return s


# ---- 1. the pipeline a program pass takes -------------------------------------------------------------------------------------
def test_a_program_pass_takes_the_pipeline_the_policy_names(programs):
    from tendrils_amd import _capi
    cur, prev = random_lines(64, 3, spread=1.0, aspect=54 / 96)
    for which, want in (("bins", BINS), ("stream", STREAM)):
        t = make(64, (96, 54))
        t.particles.draw_pipeline(which)
        t.particles.upload_texels(cur, 0)
        t.particles.upload_texels(prev, 1)
        t.timer.time = 50.0
        t.line_widths()
        u = dict(program_uniforms(t), sinTerm=t.render_uniforms().sinTerm)
        n = t._draw_program(programs["flow"], _capi.TH_PASS_FLOW, u)
        assert pipeline(t)[:2] == (want, n) and n > 1000
        n = t._draw_program(programs["view"], _capi.TH_PASS_VIEW, u)
        assert pipeline(t)[:2] == (want, n) and n > 1000
        t.dispose()
    t = make(32, (96, 54))                           # auto where no step runs over sorted slots: the stream-ordered pipeline
    cur, prev = random_lines(32, 4, spread=1.0, aspect=54 / 96)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.line_widths()
    assert t._draw_program(programs["flow"], _capi.TH_PASS_FLOW, program_uniforms(t)) > 100
    assert pipeline(t)[0] == STREAM
    t.dispose()


# ---- 2. a frame loop with both stages as programs stays on the sorted slots ------------------------------------------------------
def test_frame_loop_over_sorted_slots_stays_sorted_and_equals_the_library(programs):
    n, view = 64, (40, 40)
    st = spread_state(n, 5)
    runs = []
    for options in (dict(flowShader=programs["flow"], renderShader=programs["view"]), dict()):
        t = make(n, view, **options)
        assert t.particles.option("bucket", 1) == 1
        t.particles.draw_pipeline("bins")
        t.state["speedAlpha"] = 0.0005
        t.particles.upload_texels(st)
        t.timer.time = 1000.0
        frames = []
        for _ in range(5):
            t.timer.tick()
            t.step()
            t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
            t.draw()
            order, pipe = sorted_buffers(t), pipeline(t)[0]        # (before the read-backs: they take the ring to texel order)
            frames.append((t.particles.read(0), t.particles.read(1), t.flow.read(), t.read_view(), t.fragments, t.view_fragments, order, pipe))
        t.dispose()
        runs.append(frames)
    assert any(want[6] > 0 for want in runs[1])
    for got, want in zip(*runs):
        assert got[6] == want[6] and got[7] == want[7] == BINS
        assert bits_equal(got[0], want[0]).all() and bits_equal(got[1], want[1]).all()
        assert bits_equal(got[2], want[2]).all()
        assert (got[3] == want[3]).all()
        assert got[4] == want[4] and got[5] == want[5]
    assert (runs[1][-1][2][..., 3] != 0).sum() > 300 and runs[1][-1][3].any()


def test_frame_loop_without_read_backs_never_leaves_the_sorted_order(programs):
    """the loop a host runs: nothing between the frames takes the ring to texel order, and no program pass does"""
    t = sorted_loop(spread_state(64, 6), frames=1, flowShader=programs["flow"], renderShader=programs["view"])
    for _ in range(4):
        t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
        t.draw()
        assert sorted_buffers(t) >= 2 and pipeline(t)[0] == BINS
        t.timer.tick()
        t.step()
        assert sorted_buffers(t) > 0
    t.dispose()


# ---- 3. the golden fixtures through the bins -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", golden("deposit"), ids=lambda p: p.split("/")[-1][:-4])
def test_golden_fixtures_through_the_bins(oracle, programs, path):
    fx = load(path)
    m, base, _ = deposit_inputs(fx)
    args = (fx["current"], fx["previous"], base, m["time"], m["viewRes"], programs["flow"])
    got, frags, pipe = program_pass(*args, "bins", m["viewSize"], m["speedLimit"])
    same, same_frags, stream_pipe = program_pass(*args, "stream", m["viewSize"], m["speedLimit"])
    want, n = oracle.flow_deposit(fx["current"], fx["previous"], base, m["time"], view_size=m["viewSize"], speedLimit=m["speedLimit"])
    assert pipe == (BINS if lookups_are_local(m["N"]) else STREAM) and stream_pipe == STREAM
    assert frags == same_frags == n and n > 0
    assert bits_equal(got, same).all()
    assert bits_equal(got, want).all()


def test_some_golden_fixture_takes_the_bins():
    assert any(lookups_are_local(load(p)["meta"]["N"]) for p in golden("deposit"))


# ---- 4. the view stage --------------------------------------------------------------------------------------------------------------
def binned_view_frame(program, cur, prev, cmap, time, which):
    """view_frame of test_gpu_draw_program with the policy forced"""
    t = make(cur.shape[0], (96, 54), renderShader=program)
    t.particles.draw_pipeline(which)
    t.state.update(speedAlpha=0.5, fadeColor=[0.1333, 0.1333, 0.1333, 0.3], baseColor=[1, 0.6, 0.2, 0.5], flowColor=[0.3, 1, 0.8, 0.4])
    t.colorMap.set_pixels(cmap)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = time
    t.drawFill([0.9, 0.2, 0.4, 0.7])
    t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
    t.draw()
    out = t.read_view(), t.flow.read(), t.view_fragments, pipeline(t)[0]
    t.dispose()
    return out


def test_view_stage_through_the_bins_equals_th_view_draw(programs):
    cur, prev = random_lines(64, 15, spread=0.9, step=.08, inert=0.03, aspect=54 / 96)
    cmap = np.random.default_rng(16).uniform(0, 1, (11, 13, 4)).astype(np.float32)
    got, got_flow, frags, pipe = binned_view_frame(programs["view"], cur, prev, cmap, 1016.5, "bins")
    want, want_flow, n = view_frame(None, cur, prev, cmap, 1016.5)
    assert pipe == BINS and frags == n and n > 3000
    assert (got == want).all() and len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    assert bits_equal(got_flow, want_flow).all()


# ---- 5. positions that are not the built-in stage's, over a sorted ring ----------------------------------------------------------
@pytest.mark.parametrize("name,render", [("mirror", {}), ("zoom", dict(zoom=0.5)), ("zoom", dict(zoom=2.0)), ("even", {})],
                         ids=["mirror", "zoom_half", "zoom_two", "even_lines"])
def test_other_positions_over_a_sorted_ring_equal_the_stream_pass(programs, name, render):
    """a third of the particles lie beyond the view's left and right edge: the step sees whole blocks of the sorted order draw
    nothing - of the BUILT-IN stage's lines; a program's are elsewhere (zoom 0.5 brings them all into view)"""
    st = spread_state(64, 21, far=0.35)
    t = sorted_loop(st, render=render, renderView=False, flowShader=programs[name])
    before = t.flow.read()
    t.draw()
    assert pipeline(t)[0] == BINS and sorted_buffers(t) >= 2
    got, frags = t.flow.read(), t.fragments
    t.flow.set_pixels(before)
    cur, prev = t.particles.read(0), t.particles.read(1)
    s = twin(t, cur, prev, renderView=False, flowShader=programs[name])
    s.draw()
    assert pipeline(s)[0] == STREAM
    want, n = s.flow.read(), s.fragments
    # ... and what the library's own stage draws of this ring: fewer lines than the zoomed-out program, more than the zoomed-in
    s.flow.set_pixels(before)
    builtin = s.particles.deposit_flow(s.viewSize, s.timer.time, s.state["speedLimit"])
    t.dispose(), s.dispose()
    assert (np.abs(cur[..., 0]) > 1.05).sum() > 1000
    assert frags == n and n > 0                     # (zoomed in, a quarter of the view's particles are left: a few hundred fragments)
    assert bits_equal(got, want).all() and not bits_equal(got, before).all()
    if render.get("zoom") == 0.5:
        assert n > builtin                          # (lines the step saw outside the view are drawn)


# ---- 6. a frame that mixes a program pass with a built-in pass ----------------------------------------------------------------------
def test_mixed_frames_over_a_sorted_ring_equal_the_stream_contexts(programs):
    from tendrils_amd import _capi
    st = spread_state(64, 41)
    # the mirror program into the flow, then the library's view pass
    t = sorted_loop(st)
    t.clearView()                                   # (the loop's earlier frames drew into it; the twin's is fresh)
    t.state.update(speedAlpha=0.5, baseColor=[1, 0.6, 0.2, 0.5])
    t.line_widths()
    before = t.flow.read()
    mirrored = t._draw_program(programs["mirror"], _capi.TH_PASS_FLOW, program_uniforms(t))
    first = pipeline(t)[0]
    n = builtin_view(t)
    assert first == pipeline(t)[0] == BINS and sorted_buffers(t) >= 2
    got, got_flow = t.read_view(), t.flow.read()
    t.flow.set_pixels(before)
    cur, prev = t.particles.read(0), t.particles.read(1)
    s = twin(t, cur, prev)
    assert s._draw_program(programs["mirror"], _capi.TH_PASS_FLOW, program_uniforms(s)) == mirrored > 500
    assert builtin_view(s) == n and pipeline(s)[0] == STREAM
    assert (got == s.read_view()).all() and got.any()
    assert bits_equal(got_flow, s.flow.read()).all()
    t.dispose(), s.dispose()
    # the converse: the library's flow pass, then the mirror program into the view
    t = sorted_loop(st)
    t.clearView()                                   # (the loop's earlier frames drew into it; the twin's is fresh)
    t.state.update(speedAlpha=0.5, baseColor=[1, 0.6, 0.2, 0.5])
    t.line_widths()
    before = t.flow.read()
    frags = t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"])
    first = pipeline(t)[0]
    n = t._draw_program(programs["mirror"], _capi.TH_PASS_VIEW, program_uniforms(t))
    assert first == pipeline(t)[0] == BINS and sorted_buffers(t) >= 2
    got, got_flow = t.read_view(), t.flow.read()
    t.flow.set_pixels(before)
    cur, prev = t.particles.read(0), t.particles.read(1)
    s = twin(t, cur, prev)
    assert s.particles.deposit_flow(s.viewSize, s.timer.time, s.state["speedLimit"]) == frags
    assert s._draw_program(programs["mirror"], _capi.TH_PASS_VIEW, program_uniforms(s)) == n == mirrored
    assert (got == s.read_view()).all() and got.any()
    assert bits_equal(got_flow, s.flow.read()).all()
    t.dispose(), s.dispose()


# ---- 7. one crowded bin, and a store that has to grow under it ----------------------------------------------------------------------
def one_bin_lines(n=64, view=(96, 54)):
    """every line inside the 16 x 16-texel bin around texel (40, 24) of the view, all starting in ONE texel, up to three texels long
    (the varyings as test_crowded_texels_are_order_exact_through_a_program draws them)"""
    rng = np.random.default_rng(77)
    centre = np.array([(40.5 / view[0]) * 2 - 1, (24.5 / view[1]) * 2 - 1])
    texel = np.array([2 / view[0], 2 / view[1]])
    prev = np.zeros((n, n, 4), np.float32)
    prev[..., :2] = centre + rng.uniform(-0.3, 0.3, (n, n, 2)) * texel
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] = prev[..., :2] + (rng.uniform(-3, 3, (n, n, 2)) * texel).astype(np.float32)
    cur[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    return cur, prev


@pytest.mark.parametrize("small", [False, True], ids=["defaults", "small_store"])
def test_one_crowded_bin_equals_the_stream_pass(oracle, programs, small):
    view = (96, 54)
    cur, prev = one_bin_lines()
    base = np.zeros((view[1], view[0], 4), np.float32)

    def prepare(t):             # (two pool pages, lists of two pages: the emit is repeated with a larger pool and a wider table)
        if small:
            t.particles.option("bins_pool", 2)
            t.particles.option("bins_pages", 2)
    t = make(64, view, (1.0, 1.0), renderView=False, flowShader=programs["flow"])
    t.particles.draw_pipeline("bins")
    prepare(t)
    t.particles.upload_texels(cur, 0)
    t.particles.upload_texels(prev, 1)
    t.timer.time = 2500.0
    outs = []
    for _ in range(2):                              # (the second pass: over the store the first one left)
        t.flow.set_pixels(base)
        t.draw()
        outs.append((t.flow.read(), t.fragments) + pipeline(t))
    t.dispose()
    want, n, stream_pipe = program_pass(cur, prev, base, 2500.0, view, programs["flow"], "stream", (1.0, 1.0))
    oracle_flow, oracle_n, cov = oracle.flow_deposit(cur, prev, base, 2500.0, view_size=(1.0, 1.0), coverage=True)
    assert stream_pipe == STREAM and n == oracle_n
    assert n > 4096 and cov.max() > 300             # more places than one workgroup orders in LDS; hundreds on one texel
    assert (cov[16:32, 32:48] > 0).sum() == (cov > 0).sum()        # ... all in one bin
    for flow, frags, pipe, reported, crowded in outs:
        assert pipe == BINS and frags == reported == n and crowded > 0
        assert bits_equal(flow, want).all()
        assert bits_equal(flow, oracle_flow).all()


# ---- 8. the gates -------------------------------------------------------------------------------------------------------------------
def test_drifting_lookups_keep_to_the_stream_ordered_path(programs):
    cur, prev = random_lines(100, 6)
    base = np.zeros((54, 96, 4), np.float32)
    assert not lookups_are_local(100)
    got, frags, pipe = program_pass(cur, prev, base, 321.0, (96, 54), programs["flow"], "bins")
    want, n = flow_pass(cur, prev, base, 321.0, (96, 54), prepare=forced("stream"))
    assert pipe == STREAM and frags == n and n > 3000
    assert bits_equal(got, want).all()


def test_a_packed_ring_keeps_to_the_stream_ordered_path(programs):
    from tendrils_amd import _capi
    cur, prev = random_lines(64, 16, spread=1.0, aspect=54 / 96)
    base = np.zeros((54, 96, 4), np.float32)
    got, frags, pipe = program_pass(cur, prev, base, 321.0, (96, 54), programs["flow"], "bins", stateFormat=_capi.TH_STATE_F16)
    want, n = flow_pass(cur, prev, base, 321.0, (96, 54), prepare=forced("stream"), stateFormat=_capi.TH_STATE_F16)
    assert pipe == STREAM and frags == n and n > 1000
    assert bits_equal(got, want).all()


def test_a_wide_pass_under_auto_keeps_to_the_stream_ordered_path(programs):
    cur, prev = random_lines(64, 17, spread=0.9)
    base = np.zeros((40, 40, 4), np.float32)

    def wide(t):
        assert t.particles.option("bucket", 1) == 1        # (a sortable shape: the built-in pass of width <= 2 would take the bins)
        t.state["flowWidth"] = 3
    got, frags, pipe = program_pass(cur, prev, base, 321.0, (40, 40), programs["flow"], "auto", prepare=wide, lineWidthRange=(1, 4))
    want, n, _ = program_pass(cur, prev, base, 321.0, (40, 40), programs["flow"], "stream", prepare=wide, lineWidthRange=(1, 4))
    thin = program_pass(cur, prev, base, 321.0, (40, 40), programs["flow"], "stream")[1]
    assert pipe == STREAM and frags == n and n > 2 * thin > 0
    assert bits_equal(got, want).all()


def test_a_row_band_is_still_unsupported_with_the_bins_forced(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    t = make(64, (96, 54), row0=16, rows=32, globalHeight=64)
    t.particles.draw_pipeline("bins")
    base = np.random.default_rng(63).uniform(0, 1, (54, 96, 4)).astype(np.float32)
    t.flow.set_pixels(base)
    block, n = programs["flow"].pack(program_uniforms(t)), C.c_uint64(7)
    for which in (_capi.TH_PASS_FLOW, _capi.TH_PASS_VIEW):
        status = lib.th_draw_program_run(t.particles._ctx, programs["flow"].handle, C.byref(block), C.sizeof(block), which, C.byref(n))
        assert status == _capi.TH_ERR_UNSUPPORTED, lib.th_last_error()
        assert b"row-band" in lib.th_last_error()
    assert n.value == 7 and bits_equal(t.flow.read(), base).all()
    t.dispose()


# ---- 9. the state is untouched --------------------------------------------------------------------------------------------------------
def test_a_binned_program_pass_leaves_the_state_and_the_steps_that_follow_alone(programs):
    st = spread_state(64, 51)
    runs = []
    for with_pass in (True, False):
        t = sorted_loop(st, renderView=False, flowShader=programs["mirror"])
        kept = t.flow.read()
        respawned = t.particles.stats(0.01)["respawned"]
        if with_pass:
            t.draw()
            assert pipeline(t)[0] == BINS and t.fragments > 500 and sorted_buffers(t) >= 2
            assert t.particles.stats(0.01)["respawned"] == respawned
            t.flow.set_pixels(kept)                 # (the steps below read the flow: the pass's own deposit is not under test)
        ring = t.particles.read(0), t.particles.read(1)
        for _ in range(3):
            t.timer.tick()
            t.step()
        runs.append(ring + (t.particles.read(0), t.particles.read(1), t.particles.stats(0.01)["respawned"]))
        t.dispose()
    with_pass, without = runs
    for a, b in zip(with_pass[:4], without[:4]):
        assert bits_equal(a, b).all()
    assert with_pass[4] == without[4]
    assert not bits_equal(with_pass[0], with_pass[2]).all()


# ---- 10. th_flow in a binned pass -----------------------------------------------------------------------------------------------------
def test_th_flow_reads_the_field_as_it_was_before_a_binned_pass(programs):
    n, view = 64, (96, 54)
    cur, prev = random_lines(n, 51, spread=1.0, aspect=54 / 96)
    rng = np.random.default_rng(52)
    base = rng.uniform(-1, 1, (54, 96, 4)).astype(np.float32)
    base[..., 3] = rng.uniform(0, 1, (54, 96))
    got, frags, pipe = program_pass(cur, prev, base, 10.0, view, programs["tap"], "bins")
    st = stream_states(cur, prev)
    px, py = st[..., 0] * np.float32(1.0), st[..., 1] * np.float32(96 / 54)
    u, w = px * np.float32(0.5) + np.float32(0.5), py * np.float32(0.5) + np.float32(0.5)
    colours = base[tap(w, 54), tap(u, 96)]
    want, n_want, _ = program_pass(cur, prev, base, 10.0, view, programs["from_map"], "stream", prepare=lambda t: t.colorMap.set_pixels(colours))
    assert pipe == BINS and frags == n_want and frags > 1000
    assert bits_equal(got, want).all() and not bits_equal(got, base).all()
