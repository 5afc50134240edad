"""Both passes' fragment stages over one rasterisation on the GPU (include/tendrils_hip.h: th_draw_stages_pair;
tendrils_amd/csrc/th_fragment_pair_prelude.inc).  The yardstick of every case is a TWIN context that runs the existing calls one
after the other - th_draw_stages_run (or, for a slot without a fragment program, the built-in call) for the flow pass, then for
the view pass - never the pair call against itself.  Every comparison is bit for bit on the flow field, byte for byte on the RGBA8
view, and the ring is read back unchanged."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, deposit_hashed_inputs, load
from test_draw_program_build import FLOW
from test_fragment_program_build import IDENTITY, VIGNETTE, FragUniforms
from test_fragment_program_line_build import FALLOFF
from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms
from test_gpu_fragment_program import (base_flow, color_map, kernel_launches, last_draw, make, plain_run, sorted_buffers, stages_of,
                                       stages_run, uniforms_of)
from test_gpu_fragment_program_bins import MIRROR, binned, crowd_inputs, loop_state, looped, one_bin_inputs

pytestmark = pytest.mark.gpu

FLOW_PASS, VIEW_PASS = 0, 1          # TH_PASS_FLOW, TH_PASS_VIEW
STREAM, BINS = 0, 1                  # TH_DRAW_STREAM, TH_DRAW_BINS
INERT = [-1e6, -1e6, 0, 0]
f32 = np.float32

# the varying scaled by a uniform, from a block of its own: `gain` is its FIRST field (in VIGNETTE's block it is the last) - a
# stage handed the other stage's block scales by another number.  Not idempotent: a stage applied twice shows.
GAIN = """struct GainUniforms { float gain; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const float k = th_uniforms<GainUniforms>(f).gain;
    float4 o = f.color;
    o.x = o.x * k;
    o.y = o.y * k;
    o.w = o.w * k;
    return o;
}
"""


class GainUniforms(C.Structure):
    _fields_ = [("gain", C.c_float)]


class FalloffUniforms(C.Structure):
    _fields_ = [("halfWidth", C.c_float)]


@pytest.fixture(scope="module")
def programs():
    from tendrils_amd.particles import DrawProgram, FragmentProgram
    made = dict(identity=FragmentProgram.from_source(IDENTITY, name="identity"),
                vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"),
                gain=FragmentProgram.from_source(GAIN, GainUniforms, "gain"),
                mirror=FragmentProgram.from_source(MIRROR, FragUniforms, "mirror"),
                falloff=FragmentProgram.from_source(FALLOFF, FalloffUniforms, "falloff"),
                flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"),
                view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"))
    yield made
    for p in made.values():
        p.dispose()


def block_of(t):
    """what every program's block is packed from (by field name)"""
    return dict(uniforms_of(t), halfWidth=1.5)


def pair_run(t, flow_fragment, view_fragment, u, flow_vertex=None, view_vertex=None):
    """th_draw_stages_pair: (fragments, rasterisations)"""
    from tendrils_amd import _capi
    flow, _keep_flow = stages_of(t, FLOW_PASS, flow_vertex, flow_fragment, u)
    view, _keep_view = stages_of(t, VIEW_PASS, view_vertex, view_fragment, u)
    n, ran = C.c_uint64(0), C.c_int32(0)
    _capi.call("th_draw_stages_pair", t.particles._ctx, C.byref(flow), C.byref(view), C.byref(n), C.byref(ran))
    return int(n.value), int(ran.value)


def twin_run(t, flow_fragment, view_fragment, u, flow_vertex=None, view_vertex=None):
    """the yardstick: the flow pass, then the view pass, each through the call that has always drawn it: their fragments"""
    counts = []
    for which, vertex, fragment in ((FLOW_PASS, flow_vertex, flow_fragment), (VIEW_PASS, view_vertex, view_fragment)):
        counts.append(stages_run(t, which, vertex, fragment, u) if fragment is not None else plain_run(t, which, vertex, u))
    return counts


def builtin_draw(t):
    """th_draw: both passes with the library's own stages"""
    from tendrils_amd import _capi
    d, u, n = t.deposit_uniforms(), t.render_uniforms(), C.c_uint64(0)
    _capi.call("th_draw", t.particles._ctx, C.byref(d), C.byref(u), C.byref(n))
    return int(n.value)


def check_pair(programs, flow_name, view_name, view, cur, prev, base, cmap, ran=1, expect=STREAM, bins=False, tune=None, fmt="f32",
               least=300, vertex=(False, False), **made):
    """The pair call on one context against the twin's two passes and against th_draw of a third; the ring and the counters
    afterwards.  ran: the rasterisations the call must report; expect: the pipeline th_draw_query must name; bins: policy bins
    with stage_bins on (tune: further options, set before the first draw)."""
    got, twin, plain = (make(view, cur, prev, base, cmap, fmt=fmt, **made) for _ in range(3))
    if bins:
        for t in (got, twin, plain):
            binned(t, 1, tune)
    ring = (plain.particles.read(0), plain.particles.read(1)) if fmt == "f16" else (cur, prev)       # (what the stored texels decode to)
    u = block_of(got)
    frag = [programs[name] if name else None for name in (flow_name, view_name)]
    vert = [programs["flow"] if vertex[0] else None, programs["view"] if vertex[1] else None]
    n, reported = pair_run(got, frag[0], frag[1], u, vert[0], vert[1])
    n_flow, n_view = twin_run(twin, frag[0], frag[1], u, vert[0], vert[1])
    assert reported == ran, (reported, ran)
    assert n == n_flow >= least, (n, n_flow, n_view)
    assert last_draw(got) == (expect, n_view), (last_draw(got), expect, n_view)
    if ran == 1:
        assert n_flow == n_view
    flow, image = got.flow.read(), got.read_view()
    assert bits_equal(flow, twin.flow.read()).all(), (flow_name, view_name, "the flow field against the two passes")
    assert (image == twin.read_view()).all(), (flow_name, view_name, "the view against the two passes")
    # the stages did something - and only to their own targets
    if not any(vertex):
        assert builtin_draw(plain) == n
        for name, mine, builtin in ((flow_name, flow, plain.flow.read()), (view_name, image, plain.read_view())):
            same = (mine == builtin).all() if mine.dtype == np.uint8 else bits_equal(mine, builtin).all()
            assert same == (name in (None, "identity")), (flow_name, view_name, name)
    assert not bits_equal(flow, base).all() and image.any()
    for b in range(2):                               # the ring is untouched
        assert bits_equal(got.particles.read(b), ring[b]).all()
    limit = got.state["speedLimit"]
    assert got.particles.stats(limit) == twin.particles.stats(limit)
    for t in (got, twin, plain):
        t.dispose()
    return n


# ---- 1. identity in both slots ---------------------------------------------------------------------------------------------------------
def test_identity_in_both_slots_is_th_draw_and_the_two_plain_passes(programs):
    n, view = 48, (96, 54)
    cur, prev = deposit_hashed_inputs(n, 11, 1.1, 0.06, 13)
    base, cmap = base_flow(view, 12), color_map()
    check_pair(programs, "identity", "identity", view, cur, prev, base, cmap)
    # ... and against the two passes WITHOUT a stage
    got, plain = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
    frags, ran = pair_run(got, programs["identity"], programs["identity"], block_of(got))
    want = twin_run(plain, None, None, block_of(plain))
    assert ran == 1 and frags == want[0] == want[1] > 300
    assert last_draw(got) == (STREAM, frags)
    assert bits_equal(got.flow.read(), plain.flow.read()).all() and (got.read_view() == plain.read_view()).all()
    got.dispose()
    plain.dispose()


# ---- 2. two different programs with different uniform blocks -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,view,widths", [(32, (64, 64), None), (48, (96, 54), None), (48, (97, 61), None), (32, (97, 61), (3, 3))],
                         ids=["32-64x64", "48-96x54", "48-97x61", "32-97x61-wide"])
@pytest.mark.parametrize("flow_name,view_name", [("vignette", "gain"), ("gain", "vignette"), ("vignette", None), (None, "vignette")],
                         ids=["vignette-gain", "gain-vignette", "flow-alone", "view-alone"])
def test_two_programs_each_on_its_own_half_with_its_own_block(programs, flow_name, view_name, n, view, widths):
    """a stage on the wrong half, or one block serving both, changes bits; 97 x 61: a wrong stride shows; equal wide lines: still 1"""
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    check_pair(programs, flow_name, view_name, view, cur, prev, base_flow(view, 22), color_map(), widths=widths)


def test_no_colour_map(programs):
    n, view = 32, (64, 64)
    cur, prev = deposit_hashed_inputs(n, 23, 1.0, 0.05, 0)
    check_pair(programs, "vignette", "vignette", view, cur, prev, base_flow(view, 24), None)


# ---- 3. long and clipped lines -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["deposit_long_lines_32", "deposit_border_48"])
def test_long_and_clipped_lines(programs, fixture):
    fx = load(os.path.join(GOLDEN, fixture + ".npz"))
    m = fx["meta"]
    view = tuple(m["viewRes"])
    check_pair(programs, "vignette", "gain", view, fx["current"], fx["previous"], base_flow(view, 31), color_map(), least=1000,
               time=m["time"], view_size=m["viewSize"], speed_limit=m["speedLimit"])


# ---- 4. through the bins -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow_name,view_name", [("gain", "vignette"), ("vignette", "gain"), (None, "gain")],
                         ids=["gain-vignette", "vignette-gain", "view-alone"])
def test_ordinary_bins_on_an_odd_target(programs, flow_name, view_name):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    check_pair(programs, flow_name, view_name, view, cur, prev, base_flow(view, 22), color_map(), expect=BINS, bins=True)


def test_a_list_of_several_pages_in_one_bin(programs):
    view = (97, 61)
    cur, prev = one_bin_inputs(view)
    n = check_pair(programs, "gain", "vignette", view, cur, prev, base_flow(view, 32), color_map(), expect=BINS, bins=True, least=257)
    assert n <= 4096


def test_a_crowded_bin(programs):
    view = (96, 54)
    cur, prev = crowd_inputs(256, 0.02, 7)
    check_pair(programs, "gain", "vignette", view, cur, prev, base_flow(view, 41), color_map(), expect=BINS, bins=True, least=20_000)


@pytest.mark.parametrize("case", ["pool", "widen", "abandon"])
def test_repeated_and_abandoned_passes_apply_each_stage_once(programs, case):
    """a pool of 8 pages runs dry and the pass is repeated; lists of 2 pages at first are widened and the pass is repeated; lists
    of 2 pages that may not be widened leave the pass to the stream-ordered pipeline - both stages ran over every attempt's store"""
    view = (96, 54)
    spread, seed, tune, expect = dict(pool=(0.2, 5, dict(bins_pool=8), BINS), widen=(0.2, 5, dict(bins_pool=8, bins_pages=2), BINS),
                                      abandon=(0.02, 7, dict(bins_pool=8, bins_pages=-2), STREAM))[case]
    cur, prev = crowd_inputs(256, spread, seed)
    check_pair(programs, "gain", "gain", view, cur, prev, base_flow(view, 61), color_map(), expect=expect, bins=True, tune=tune, least=20_000)


@pytest.mark.parametrize("shape", ["packed", "drifting"])
def test_packed_rings_and_drifting_shapes(programs, shape):
    n, view, fmt = (48, (97, 61), "f16") if shape == "packed" else (100, (160, 90), "f32")
    cur, prev = deposit_hashed_inputs(n, 71 + n, 1.05, 0.08, 11)
    check_pair(programs, "vignette", "gain", view, cur, prev, base_flow(view, 72), color_map(), expect=BINS, bins=True, fmt=fmt)


def test_a_tile_sorted_ring_stays_sorted_and_draws_the_same_bits(programs):
    view, st = (33, 31), loop_state()
    held, read = looped(view, st), looped(view, st)
    for t in (held, read):
        assert t.particles.option("stage_bins", 1) == 1
    assert sorted_buffers(held) == 2
    ring = read.particles.read(0), read.particles.read(1)          # (reading takes `read` to texel order)
    assert sorted_buffers(read) == 0 and sorted_buffers(held) == 2
    u = block_of(held)
    want = twin_run(read, programs["gain"], programs["vignette"], u)
    n, ran = pair_run(held, programs["gain"], programs["vignette"], u)
    assert ran == 1 and n == want[0] == want[1] > 300
    assert last_draw(held) == (BINS, n)
    assert sorted_buffers(held) == 2                                # the ring is still in its sorted slots
    assert bits_equal(held.flow.read(), read.flow.read()).all() and (held.read_view() == read.read_view()).all()
    for b in range(2):
        assert bits_equal(held.particles.read(b), ring[b]).all()
    held.dispose()
    read.dispose()


# ---- 5. the fallbacks: two rasterisations, the sequential bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["falloff-flow", "falloff-view", "widths", "vertex-flow", "vertex-view"])
def test_what_one_rasterisation_cannot_give_runs_as_two_passes(programs, case):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    flow_name, view_name = dict(**{"falloff-flow": ("falloff", "gain"), "falloff-view": ("vignette", "falloff")}).get(case, ("vignette", "gain"))
    check_pair(programs, flow_name, view_name, view, cur, prev, base_flow(view, 22), color_map(), ran=2,
               widths=(3, 1) if case == "widths" else None, vertex=(case == "vertex-flow", case == "vertex-view"))


def tapping_state(view):
    """a base field with structure everywhere and lines all over the target: the flow pass changes texels the mirrored tap reads"""
    n = 48
    cur, prev = deposit_hashed_inputs(n, 91, 1.05, 0.08, 11)
    return cur, prev, base_flow(view, 92)


def test_a_view_stage_that_taps_the_flow_runs_as_two_passes(programs):
    view = (97, 61)
    cur, prev, base = tapping_state(view)
    cmap = color_map()
    # the case proves something only if the view stage's taps see the flow pass: on the twin's side, the view drawn over the field
    # as it was BEFORE the flow pass differs from the view drawn after it
    before, after = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
    u = block_of(before)
    assert stages_run(before, VIEW_PASS, None, programs["mirror"], u) > 300
    counts = twin_run(after, programs["gain"], programs["mirror"], u)
    assert counts[0] == counts[1] > 300
    assert not (before.read_view() == after.read_view()).all()
    got = make(view, cur, prev, base, cmap)
    n, ran = pair_run(got, programs["gain"], programs["mirror"], u)
    assert ran == 2 and n == counts[0] and last_draw(got) == (STREAM, counts[1])
    assert bits_equal(got.flow.read(), after.flow.read()).all() and (got.read_view() == after.read_view()).all()
    for t in (before, after, got):
        t.dispose()


def test_the_same_tap_in_the_flow_slot_runs_as_one(programs):
    view = (97, 61)
    cur, prev, base = tapping_state(view)
    check_pair(programs, "mirror", "gain", view, cur, prev, base, color_map())
    check_pair(programs, "mirror", "gain", view, cur, prev, base, color_map(), expect=BINS, bins=True)


# ---- 6. refusals draw nothing and launch nothing -----------------------------------------------------------------------------------------
def test_refusals_draw_nothing_and_launch_nothing(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    n, view = 32, (64, 64)
    cur, prev = deposit_hashed_inputs(n, 71, 1.0, 0.05, 0)
    base = base_flow(view, 72)
    t = make(view, cur, prev, base, color_map())
    _capi.call("th_kernel_timing", t.particles._ctx, 1)
    u = block_of(t)
    view_before = t.read_view()
    frag, vert = programs["vignette"], programs["flow"]

    def slot(which, vertex=None, fragment=None, builtin=True, time=None):
        s, keep = stages_of(t, which, vertex, fragment, u)
        if time is not None:
            keep[0].time = time
        if not builtin:
            s.builtin = None
        return s, keep

    def refused(flow, view_, status, words):
        count, ran = C.c_uint64(7), C.c_int32(7)
        got = lib.th_draw_stages_pair(t.particles._ctx, C.byref(flow[0]) if flow else None, C.byref(view_[0]) if view_ else None, C.byref(count), C.byref(ran))
        message = lib.th_last_error().decode()
        assert got == status and all(re.search(r"\b%s\b" % re.escape(w), message) for w in words), (got, message)
        assert bits_equal(t.flow.read(), base).all() and (t.read_view() == view_before).all(), message
        assert kernel_launches(t) == 0

    ok_flow, ok_view = slot(FLOW_PASS, fragment=frag), slot(VIEW_PASS, fragment=frag)
    refused(None, ok_view, _capi.TH_ERR_INVALID, ["null"])
    refused(ok_flow, None, _capi.TH_ERR_INVALID, ["null"])
    refused(slot(FLOW_PASS), slot(VIEW_PASS), _capi.TH_ERR_INVALID, ["th_draw"])
    refused(slot(FLOW_PASS, vertex=vert), slot(VIEW_PASS, vertex=programs["view"]), _capi.TH_ERR_INVALID, ["th_draw"])
    refused(slot(FLOW_PASS, fragment=vert), ok_view, _capi.TH_ERR_INVALID, ["draw program", "fragment program"])
    refused(ok_flow, slot(VIEW_PASS, vertex=frag), _capi.TH_ERR_INVALID, ["draw program", "fragment program"])
    refused(slot(FLOW_PASS, fragment=frag, builtin=False), ok_view, _capi.TH_ERR_INVALID, ["builtin", "th_deposit_uniforms"])
    refused(ok_flow, slot(VIEW_PASS, fragment=frag, builtin=False), _capi.TH_ERR_INVALID, ["builtin", "th_render_uniforms"])
    refused(ok_flow, slot(VIEW_PASS, fragment=frag, time=float(t.timer.time) + 1.0), _capi.TH_ERR_INVALID, ["time"])
    # ... and the same slots, in order, draw
    frags, ran = pair_run(t, frag, frag, u)
    assert ran == 1 and frags > 300 and kernel_launches(t) == 2
    t.dispose()
    # a row band: unsupported, nothing launched
    band = make(view, cur, prev, base, color_map(), band=(0, 16))
    flow, _k1 = stages_of(band, FLOW_PASS, None, frag, u)
    view_, _k2 = stages_of(band, VIEW_PASS, None, frag, u)
    count, ran = C.c_uint64(0), C.c_int32(0)
    assert lib.th_draw_stages_pair(band.particles._ctx, C.byref(flow), C.byref(view_), C.byref(count), C.byref(ran)) == _capi.TH_ERR_UNSUPPORTED
    assert b"th_draw_stages_emit" in lib.th_last_error()
    assert bits_equal(band.flow.read(), base).all()
    band.dispose()


def test_launches_none_without_fragments_two_for_two_stages_one_for_one(programs):
    from tendrils_amd import _capi
    n, view = 32, (64, 64)
    inert = np.tile(np.array(INERT, f32), (n, n, 1))
    base = base_flow(view, 41)
    t = make(view, inert, inert, base, color_map())
    _capi.call("th_kernel_timing", t.particles._ctx, 1)
    before = t.read_view()
    u = block_of(t)
    assert pair_run(t, programs["vignette"], programs["gain"], u) == (0, 1)
    assert last_draw(t) == (STREAM, 0) and kernel_launches(t) == 0
    assert bits_equal(t.flow.read(), base).all() and (t.read_view() == before).all()
    live, _ = deposit_hashed_inputs(n, 42, 1.0, 0.05, 0)
    t.particles.upload_texels(live, 0)
    t.particles.upload_texels(live * f32(0.5), 1)
    frags, ran = pair_run(t, programs["vignette"], programs["gain"], u)
    assert frags > 0 and ran == 1 and kernel_launches(t) == 2
    assert pair_run(t, None, programs["gain"], u) == (frags, 1) and kernel_launches(t) == 1
    assert pair_run(t, programs["gain"], None, u) == (frags, 1) and kernel_launches(t) == 1
    t.dispose()


# ---- 7. nothing of a pair call outlives it -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["stream", "bins"])
def test_builtin_calls_after_a_pair_call_are_a_fresh_contexts(programs, policy):
    n, view = 16, (64, 48)
    cur, prev = deposit_hashed_inputs(n, 55, 1.05, 0.08, 3)
    base, cmap = base_flow(view, 56), color_map()
    staged, fresh = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
    for t in (staged, fresh):
        t.particles.draw_pipeline(policy)
    assert staged.particles.option("stage_bins", 1) == 1
    u = block_of(staged)
    pipeline = BINS if policy == "bins" else STREAM

    def builtin_runs(t):
        out = []
        for calls in ("draw", "passes"):
            t.flow.set_pixels(base)
            t.clearView()
            counts = [builtin_draw(t)] if calls == "draw" else [plain_run(t, which, None, u) for which in (FLOW_PASS, VIEW_PASS)]
            assert last_draw(t) == (pipeline, counts[-1])
            out.append((counts, t.flow.read(), t.read_view()))
        return out

    want = builtin_runs(fresh)
    assert want[0][0][0] == want[1][0][0] == want[1][0][1] > 50
    for view_name in ("gain", "mirror"):                  # one rasterisation, then the two passes of the fallback
        count, ran = pair_run(staged, programs["vignette"], programs[view_name], u)
        assert count > 50 and ran == (1 if view_name == "gain" else 2) and last_draw(staged) == (pipeline, count)
        got = builtin_runs(staged)
        for (gc, gf, gv), (wc, wf, wv) in zip(got, want):
            assert gc == wc and bits_equal(gf, wf).all() and (gv == wv).all(), view_name
    assert not bits_equal(want[0][1], base).all() and want[0][2].any()
    staged.dispose()
    fresh.dispose()


# ---- 8. the host -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage_bins", [1, 0], ids=["stage-bins", "stream"])
def test_a_frame_loop_with_paired_stages_equals_the_loop_without(programs, stage_bins):
    view, st = (33, 31), loop_state()
    frag = programs["vignette"]
    loops = []
    for paired in (True, False):
        t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map(), flowShader=(None, frag), renderShader=(None, frag),
                 **(dict(pairedStages=True) if paired else {}))
        assert t.pairedStages is paired and t.rasterisations is None           # (off unless asked for)
        assert t.particles.option("bucket", 1) == 1
        binned(t, stage_bins)
        t.timer.time = 1000.0
        loops.append(t)
    on, off = loops
    u = uniforms_of(on)
    for t in loops:
        t.uniforms["render"].update({k: u[k] for k in ("tint", "invRes", "edge", "gain")})
    for frame in range(6):
        for t in loops:
            t.timer.tick()
            t.step()
            t.draw()
        assert on.rasterisations == 1 and off.rasterisations is None
        assert (on.fragments, on.view_fragments) == (off.fragments, off.view_fragments) and on.fragments > 300, frame
        assert last_draw(on) == last_draw(off) == (BINS if stage_bins else STREAM, on.view_fragments)
        assert bits_equal(on.flow.read(), off.flow.read()).all(), frame
        assert (on.read_view() == off.read_view()).all() and on.read_view().any(), frame
        for b in range(2):
            assert bits_equal(on.particles.read(b), off.particles.read(b)).all(), (frame, b)
    for t in loops:
        t.dispose()
