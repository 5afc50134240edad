"""th_line(f) through the binned draw() (TH_OPT_LINE_BINS beside TH_OPT_STAGE_BINS; tendrils_amd/csrc/th_fragline.hip:
fragment_line_ends_kernel, fragment_lines_bins_kernel; th_fragment_prelude.inc: th_fragment_line_bins_kernel; th_fragprog.hip:
fragment_stage_run_bins).  With both options on, a pass whose fragment stage reads the line takes the pipeline the pass without
the stage would take; through the bins its line records lie beside the page store's places.  No expected value comes from the
code under test.  Every pass is compared, bit for bit on the flow field and byte for byte on the RGBA8 view, with references
the option does not touch: the same pass on a second context with line_bins off (the stream-ordered path), the numpy
restatement of tests/test_gpu_fragment_program_line.py (the existing emit, the record in numpy's fp32 and Python integers, the
existing merge) and the pass without a stage (which must differ).  Every case runs with policy "bins" and stage_bins = 1."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, deposit_hashed_inputs, load
from test_fragment_program_build import FragUniforms  # noqa: F401  (what `programs` packs the vignette's block from)
from test_fragment_program_line_build import FALLOFF
from test_gpu_fragment_program import (base_flow, color_map, kernel_launches, last_draw, make, plain_run, same, sorted_buffers,
                                       stages_run, target, uniforms_of)
from test_gpu_fragment_program_bins import PASS_IDS, PASSES, crowd_inputs, draw_info, loop_state, looped, one_bin_inputs
from test_gpu_fragment_program_line import RESTATED, emit_plain, ends_of_export, ends_of_state, merge, programs, wide  # noqa: F401  (programs: the fixture)

pytestmark = pytest.mark.gpu

FLOW_PASS, VIEW_PASS = 0, 1          # TH_PASS_FLOW, TH_PASS_VIEW
STREAM, BINS = 0, 1                  # TH_DRAW_STREAM, TH_DRAW_BINS
NAMES = ("fields", "line_id")
f32 = np.float32


def lined(t, line_bins, tune=None, stage_bins=1):
    """policy "bins", both options as asked, whatever else the case sets before the first draw"""
    t.particles.draw_pipeline("bins")
    assert t.particles.option("stage_bins", stage_bins) == stage_bins
    assert t.particles.option("line_bins", line_bins) == line_bins
    for name, value in (tune or {}).items():
        t.particles.option(name, value)
    return t


def check_line_pass(programs, name, which, with_vertex, view, cur, prev, base, expect=BINS, fmt="f32", tune=None, least=300,  # noqa: F811
                    most=None, again=False, crowded=False, width=None, restated=True, **made):
    """One pass with the stage `name` and both options on, against line_bins off, the restatement and the pass without the
    stage; the ring's bits afterwards.  expect: the pipeline the pass must report; again: a second draw afterwards runs clean;
    restated: the numpy restatement applies (shapes whose every vertex reads its line's own texel)."""
    import torch
    if width is not None:
        made = dict(made, lineWidthRange=(1, 8))

    def context(c, p, f):
        t = make(view, c, p, base, color_map(), fmt=f, **made)
        return wide(t, width) if width is not None else t

    got, off = lined(context(cur, prev, fmt), 1, tune), lined(context(cur, prev, fmt), 0, tune)
    ring = (off.particles.read(0), off.particles.read(1)) if fmt == "f16" else (cur, prev)       # (what the stored texels decode to)
    ref = context(ring[0], ring[1], "f32")
    vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(got)
    n = stages_run(got, which, vertex, programs[name], u)
    assert last_draw(got) == (expect, n), (last_draw(got), expect, n)
    info = draw_info(got)
    n_off = stages_run(off, which, vertex, programs[name], u)
    assert last_draw(off) == (STREAM, n_off)         # (line_bins off: stream-ordered whatever stage_bins says)
    assert n == n_off >= least, (n, n_off)
    assert most is None or n <= most, n
    assert not crowded or info.crowded_fragments > 0
    drawn = target(got, which)
    assert same(drawn, target(off, which)), (name, which, with_vertex, "against the option off")
    if restated:
        ends = ends_of_state(ring[0], ring[1], got.viewSize) if with_vertex else ends_of_export(ref, which, ring[0], ring[1])
        keys, colors = emit_plain(ref, which, vertex, u)
        k = keys.cpu().numpy().astype(np.uint64)
        assert len(k) == n
        want = np.ascontiguousarray(RESTATED[name](k, colors.cpu().numpy(), ends, view), f32)
        merge(ref, which, keys.clone(), torch.from_numpy(want).cuda().contiguous())
        assert same(drawn, target(ref, which)), (name, which, with_vertex, "against the restatement")
    ref.flow.set_pixels(base)
    ref.clearView()
    assert plain_run(ref, which, vertex, u) == n
    assert not same(drawn, target(ref, which))       # the stage did something
    for b in range(2):
        assert bits_equal(got.particles.read(b), ring[b]).all()
    if again:
        got.flow.set_pixels(base)
        got.clearView()
        assert stages_run(got, which, vertex, programs[name], u) == n
        assert same(target(got, which), target(off, which))
    for t in (got, off, ref):
        t.dispose()
    return n


# ---- 1. ordinary bins, a target that is no multiple of 16 ----------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_ordinary_bins_on_an_odd_target(programs, which, with_vertex):  # noqa: F811
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 22))


# ---- 2. one list of several pages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_list_of_several_pages_in_an_ordinary_bin(programs, which, with_vertex):  # noqa: F811
    """one list, more than a page of fragments and at most 4096: the records beyond the list's first page come through the table"""
    view = (97, 61)
    cur, prev = one_bin_inputs(view)
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 32), least=257, most=4096)


# ---- 3. a crowded bin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_crowded_bin(programs, which, with_vertex):  # noqa: F811
    """65536 lines within a texel or two of the centre: more than 4096 places in a bin, texel runs longer than 256 (the inputs are
    shown to be that in tests/test_gpu_fragment_program_bins.py); the regroup and the long and giant runs blend what the stage wrote"""
    view = (96, 54)
    cur, prev = crowd_inputs(256, 0.02, 7)
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 41), least=20_000, crowded=True)


# ---- 4. lines the fused kernel does not rasterise itself ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
@pytest.mark.parametrize("fixture", ["deposit_border_48", "deposit_long_lines_32"])
def test_clipped_lines_and_lines_that_span_the_view(programs, fixture, which, with_vertex):  # noqa: F811
    fx = load(os.path.join(GOLDEN, fixture + ".npz"))
    m = fx["meta"]
    view = tuple(m["viewRes"])
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, fx["current"], fx["previous"], base_flow(view, 51), least=1000,
                        time=m["time"], view_size=m["viewSize"], speed_limit=m["speedLimit"])


@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_lines_five_texels_wide(programs, which, with_vertex):  # noqa: F811
    """more fragments than a line's record holds: the long list, a place at a time"""
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 52), least=1500, width=5)


# ---- 5. the repeats ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pool", "widen", "abandon"])
@pytest.mark.parametrize("which,with_vertex", [(FLOW_PASS, False), (VIEW_PASS, True)], ids=["flow-builtin", "view-program"])
def test_repeated_and_abandoned_passes_apply_the_stage_once(programs, case, which, with_vertex):  # noqa: F811
    """a pool of 8 pages runs dry and the pass is repeated over a larger store - the records follow it; lists of 2 pages at first are
    widened and the pass is repeated; lists of 2 pages that may not be widened leave the pass to the stream-ordered pipeline and its
    own line kernel"""
    view = (96, 54)
    spread, seed, tune, expect = dict(pool=(0.2, 5, dict(bins_pool=8), BINS), widen=(0.2, 5, dict(bins_pool=8, bins_pages=2), BINS),
                                      abandon=(0.02, 7, dict(bins_pool=8, bins_pages=-2), STREAM))[case]
    cur, prev = crowd_inputs(256, spread, seed)
    for name in NAMES:
        check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 61), expect=expect, tune=tune,
                        least=20_000, again=True)


# ---- 6. a packed ring and a drifting shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [FLOW_PASS, VIEW_PASS], ids=["flow", "view"])
@pytest.mark.parametrize("shape", ["packed", "drifting"])
def test_packed_rings_and_drifting_shapes(programs, shape, which):  # noqa: F811
    """with the library's vertex stage both go through the bins; with a vertex program the gate of deposit_prepare sends the same
    inputs stream-ordered - with the same bits.  (n = 100: some vertices read other lines' texels, which the restatement of these
    tests does not follow - that shape is compared with the option off and with the pass without a stage)"""
    n, view, fmt = (48, (97, 61), "f16") if shape == "packed" else (100, (160, 90), "f32")
    cur, prev = deposit_hashed_inputs(n, 71 + n, 1.05, 0.08, 11)
    for with_vertex, expect in ((False, BINS), (True, STREAM)):
        for name in NAMES:
            check_line_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 72), expect=expect, fmt=fmt,
                            restated=shape == "packed")


# ---- 7. the point of it: the ring keeps its sorted slots -----------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_tile_sorted_ring_stays_sorted_and_draws_the_same_bits(programs, which, with_vertex):  # noqa: F811
    view, st = (33, 31), loop_state()
    held, read = looped(view, st), looped(view, st)
    assert held.particles.option("stage_bins", 1) == 1 and held.particles.option("line_bins", 1) == 1
    assert read.particles.option("stage_bins", 1) == 1              # (line_bins off: stream-ordered, through texel order)
    assert sorted_buffers(held) > 0
    ring = read.particles.read(0), read.particles.read(1)           # (reading takes `read` to texel order)
    assert sorted_buffers(read) == 0 and sorted_buffers(held) > 0
    vertex, u = (programs["parity"] if with_vertex else None), uniforms_of(held)
    blank = np.zeros((view[1], view[0], 4), f32)
    for name in NAMES:
        for t in (held, read):
            t.flow.set_pixels(blank)
            t.clearView()
        want_n = stages_run(read, which, vertex, programs[name], u)
        assert last_draw(read) == (STREAM, want_n)
        assert stages_run(held, which, vertex, programs[name], u) == want_n > 300
        assert last_draw(held) == (BINS, want_n)
        assert sorted_buffers(held) > 0 and sorted_buffers(read) == 0       # the ring is still in its sorted slots
        assert same(target(held, which), target(read, which)), name
        assert target(held, which).any()
    for b in range(2):
        assert bits_equal(held.particles.read(b), ring[b]).all()
        assert bits_equal(read.particles.read(b), ring[b]).all()
    held.dispose()
    read.dispose()


# ---- 8. a frame loop -----------------------------------------------------------------------------------------------------------------
def test_a_frame_loop_with_the_falloff_equals_the_loop_with_the_option_off():
    """step(); draw() with FALLOFF (the reference's "SDF from line" @todo) as the flow pass's fragment stage, on lines five texels
    wide as the reference's flowWidth asks: target for target, every frame; only the loop with the option keeps its sorted slots"""
    import ctypes as C
    from tendrils_amd.particles import FragmentProgram

    class Falloff(C.Structure):
        _fields_ = [("halfWidth", C.c_float)]

    falloff = FragmentProgram.from_source(FALLOFF, Falloff, "falloff")
    view, st = (33, 31), loop_state()
    loops = []
    for line_bins in (1, 0):
        t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map(), flowShader=(None, falloff), lineWidthRange=(1, 8))
        assert t.particles.option("bucket", 1) == 1
        lined(t, line_bins)
        t.uniforms["render"]["halfWidth"] = 3.0
        t.timer.time = 1000.0
        loops.append(t)
    on, off = loops
    for frame in range(3):
        for t in loops:
            t.timer.tick()
            t.step()
            t.draw()
        assert (on.fragments, on.view_fragments) == (off.fragments, off.view_fragments) and on.fragments > 300, frame
        assert last_draw(on) == (BINS, on.view_fragments)
        assert bits_equal(on.flow.read(), off.flow.read()).all(), frame
        assert (on.read_view() == off.read_view()).all() and on.read_view().any(), frame
    assert sorted_buffers(on) > 0 and sorted_buffers(off) == 0
    for b in range(2):
        assert bits_equal(on.particles.read(b), off.particles.read(b)).all()
    for t in loops:
        t.dispose()
    falloff.dispose()


# ---- 9. routing ----------------------------------------------------------------------------------------------------------------------
def test_routing(programs):  # noqa: F811
    from tendrils_amd import _capi
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 51, 1.05, 0.08, 11)
    base = base_flow(view, 52)
    fresh = make(view, cur, prev, base, color_map())
    assert fresh.particles.option("line_bins") == 0 and fresh.particles.option("stage_bins") == 0       # the defaults
    fresh.dispose()
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            vertex = programs["parity"] if with_vertex else None
            made = {}
            for stage_bins, line_bins, pipeline in ((1, 0, STREAM), (0, 1, STREAM), (1, 1, BINS)):
                t = lined(make(view, cur, prev, base, color_map()), line_bins, stage_bins=stage_bins)
                u = uniforms_of(t)
                count = stages_run(t, which, vertex, programs["fields"], u)
                assert count > 300 and last_draw(t) == (pipeline, count), (stage_bins, line_bins, last_draw(t))
                made[stage_bins, line_bins] = t
            drawn = [target(t, which) for t in made.values()]
            assert same(drawn[0], drawn[1]) and same(drawn[0], drawn[2])
            # VIGNETTE's pipeline and its single timed launch do not depend on line_bins; a line pass brackets one launch too,
            # through the bins as in stream order (the line kernels are the raster's side)
            for (stage_bins, line_bins), t in made.items():
                t.flow.set_pixels(base)
                t.clearView()
                _capi.call("th_kernel_timing", t.particles._ctx, 1)
                n_v = stages_run(t, which, None, programs["vignette"], u)
                assert last_draw(t) == (BINS if stage_bins else STREAM, n_v) and n_v > 300
                assert kernel_launches(t) == 1
                n_f = stages_run(t, which, None, programs["fields"], u)
                assert last_draw(t) == (BINS if stage_bins and line_bins else STREAM, n_f)
                assert kernel_launches(t) == 1
            vignetted = [target(t, which) for t in made.values()]
            assert same(vignetted[0], vignetted[1]) and same(vignetted[0], vignetted[2])
            for t in made.values():
                t.dispose()
