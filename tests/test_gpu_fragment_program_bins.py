"""Fragment programs through the binned draw() (TH_OPT_STAGE_BINS; tendrils_amd/csrc/th_fragment_prelude.inc:
th_fragment_bins_kernel, th_fragprog.hip: fragment_stage_run_bins, th_draw.hip: bins_pass_emit).  With the option on, a pass
with a caller's fragment stage takes the pipeline the same pass without the stage would take; through the bins the stage runs
over the page store, in place, between the emitting pass and the blends.  No expected value comes from the code under test.
Every pass is compared, bit for bit on the flow field and byte for byte on the RGBA8 view, with two references this option
does not touch: the same pass on a second context with the option off (the stream-ordered path), and the numpy restatement of
tests/test_gpu_fragment_program.py (reference_pass: the existing emit, the fragment function in numpy's fp32, the existing
merge).  Besides VIGNETTE a second program, MIRROR, taps th_flow at the mirrored window position: in the flow pass a blend
that started before every fragment had run would hand it texels the pass had already written."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, deposit_hashed_inputs, load
from test_draw_program_build import FLOW
from test_fragment_program_build import VIGNETTE, FragUniforms
from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms
from test_gpu_fragment_program import (RESTATED, base_flow, color_map, last_draw, make, plain_run, reference_pass, same,
                                       sorted_buffers, stages_run, tap_nearest, target, uniforms_of)

pytestmark = pytest.mark.gpu

FLOW_PASS, VIEW_PASS = 0, 1          # TH_PASS_FLOW, TH_PASS_VIEW
STREAM, BINS = 0, 1                  # TH_DRAW_STREAM, TH_DRAW_BINS
PASSES = [(FLOW_PASS, False), (FLOW_PASS, True), (VIEW_PASS, False), (VIEW_PASS, True)]      # (pass, with a vertex program)
PASS_IDS = ["flow-builtin", "flow-program", "view-builtin", "view-program"]
f32 = np.float32

# the flow field, as it was before the pass, at the window position mirrored through the target's centre: + - *, fminf / fmaxf
# only (numpy restates it exactly with contraction off)
MIRROR = """struct FragUniforms { float tint[4]; float invRes[2]; float edge; float gain; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const FragUniforms &u = th_uniforms<FragUniforms>(f);
    const float4 m = th_flow(f, (f.viewRes.x - f.coord.x) * u.invRes[0], (f.viewRes.y - f.coord.y) * u.invRes[1]);
    float4 o;
    o.x = f.color.x + m.x * u.gain;
    o.y = f.color.y - m.y * u.gain;
    o.z = f.color.z;
    o.w = fminf(fmaxf(f.color.w * u.tint[3] + m.w * 0.125f, 0.0f), 1.0f);
    return o;
}
"""


def mirror_np(color, x, y, view_res, which, u, cmap, flow):
    """MIRROR in fp32, operation for operation; `flow`: the field before the pass"""
    cx, cy = x.astype(f32) + f32(0.5), y.astype(f32) + f32(0.5)
    mu, mv = (f32(view_res[0]) - cx) * f32(u["invRes"][0]), (f32(view_res[1]) - cy) * f32(u["invRes"][1])
    m = flow[tap_nearest(mv, flow.shape[0]), tap_nearest(mu, flow.shape[1])]
    out = np.empty_like(color)
    out[:, 0] = color[:, 0] + m[:, 0] * f32(u["gain"])
    out[:, 1] = color[:, 1] - m[:, 1] * f32(u["gain"])
    out[:, 2] = color[:, 2]
    out[:, 3] = np.minimum(np.maximum(color[:, 3] * f32(u["tint"][3]) + m[:, 3] * f32(0.125), f32(0.0)), f32(1.0))
    return out


@pytest.fixture(scope="module")
def programs():
    from tendrils_amd.particles import DrawProgram, FragmentProgram
    made = dict(vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"),
                mirror=FragmentProgram.from_source(MIRROR, FragUniforms, "mirror"),
                flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"),
                view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"))
    yield made
    for p in made.values():
        p.dispose()


def vertex_of(programs, which, with_vertex):
    return (programs["view"] if which == VIEW_PASS else programs["flow"]) if with_vertex else None


def crowd_inputs(n, spread, seed):
    """the input recipe of tests/test_gpu_binned_draw.py::test_pool_growth_and_overfull_bins_exactly"""
    rng = np.random.default_rng(seed)
    prev = np.zeros((n, n, 4), f32)
    prev[..., :2] = rng.uniform(-spread, spread, (n, n, 2))
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] += rng.uniform(-.03, .03, (n, n, 2)).astype(f32)
    return cur, prev


def draw_info(t):
    from tendrils_amd import _capi
    info = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(info))
    return info


def binned(t, stage_bins, tune=None):
    """policy "bins", the option as asked, whatever else the case sets before the first draw"""
    t.particles.draw_pipeline("bins")
    assert t.particles.option("stage_bins", stage_bins) == stage_bins
    for name, value in (tune or {}).items():
        t.particles.option(name, value)
    return t


def check_pass(programs, name, which, with_vertex, view, cur, prev, base, cmap, expect=BINS, fmt="f32", tune=None, least=300,
               most=None, again=False, crowded=False, **made):
    """One pass with the stage `name` and the option on, against the option off, the restatement and the pass without the stage;
    the ring's bits afterwards.  expect: the pipeline the pass must report; again: a second draw afterwards runs clean."""
    got, off = binned(make(view, cur, prev, base, cmap, fmt=fmt, **made), 1, tune), binned(make(view, cur, prev, base, cmap, fmt=fmt, **made), 0, tune)
    ring = (off.particles.read(0), off.particles.read(1)) if fmt == "f16" else (cur, prev)       # (what the stored texels decode to)
    ref = make(view, ring[0], ring[1], base, cmap, **made)
    vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(got)
    RESTATED["mirror"] = functools.partial(mirror_np, flow=base)
    n = stages_run(got, which, vertex, programs[name], u)
    assert last_draw(got) == (expect, n), (last_draw(got), expect, n)
    info = draw_info(got)
    n_off = stages_run(off, which, vertex, programs[name], u)
    assert last_draw(off) == (STREAM, n_off)         # (the option off: stream-ordered under every policy)
    n_ref = reference_pass(ref, which, vertex, name, u, cmap)
    assert n == n_off == n_ref >= least, (n, n_off, n_ref)
    assert most is None or n <= most, n
    assert not crowded or info.crowded_fragments > 0
    drawn = target(got, which)
    assert same(drawn, target(off, which)), (name, which, with_vertex, "against the option off")
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


# ---- (a) ordinary bins, a target that is no multiple of 16 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vignette", "mirror"])
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_ordinary_bins_on_an_odd_target(programs, name, which, with_vertex):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    check_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 22), color_map())


def one_bin_inputs(view):
    """256 particles (one block of 256 slots: one list of the bin) whose lines lie inside the bin of texels 32..47 x 16..31"""
    n = 16
    rng = np.random.default_rng(31)
    size = [max(view) / view[0], max(view) / view[1]]             # (viewSize: position x viewSize is the window position in -1 .. 1)
    lo = np.array([-1 + 2 * 34.5 / view[0], -1 + 2 * 18.5 / view[1]]) / size
    hi = np.array([-1 + 2 * 45.5 / view[0], -1 + 2 * 29.5 / view[1]]) / size
    prev = np.zeros((n, n, 4), f32)
    prev[..., :2] = rng.uniform(lo, hi, (n, n, 2))
    prev[..., 2:] = rng.uniform(-.012, .012, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] += (rng.uniform(-2.0, 2.0, (n, n, 2)) * 2 / np.array(view) / size).astype(f32)      # (up to two texels each way)
    return cur.astype(f32), prev.astype(f32)


@pytest.mark.parametrize("name", ["vignette", "mirror"])
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_list_of_several_pages_in_an_ordinary_bin(programs, name, which, with_vertex):
    """one list, more than a page of fragments and at most 4096: the places beyond the list's first page come through the table"""
    view = (97, 61)
    cur, prev = one_bin_inputs(view)
    if (name, which, with_vertex) == ("vignette", FLOW_PASS, False):          # the inputs are what they are meant to be
        from tendrils_amd import sharding
        t = make(view, cur, prev, base_flow(view, 32), color_map())
        keys, _colors = sharding.emit_fragments(t)
        texel = ((keys.cpu().numpy().astype(np.uint64) >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.int64)
        assert set((texel % view[0]) >> 4) == {2} and set((texel // view[0]) >> 4) == {1}
        t.dispose()
    check_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 32), color_map(), least=257, most=4096)


# ---- (b) a crowded bin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vignette", "mirror"])
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_crowded_bin(programs, name, which, with_vertex):
    """65536 lines within a texel or two of the centre: far more than 4096 places in a bin - some list spans pages - and texels
    with runs of far more than 256 fragments; the crowd's kernels fetch the staged varyings"""
    view = (96, 54)
    cur, prev = crowd_inputs(256, 0.02, 7)
    if (name, which, with_vertex) == ("vignette", FLOW_PASS, False):          # the inputs are what they are meant to be
        from tendrils_amd import sharding
        t = make(view, cur, prev, base_flow(view, 41), color_map())
        keys, _colors = sharding.emit_fragments(t)
        texel = ((keys.cpu().numpy().astype(np.uint64) >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.int64)
        per_bin = np.bincount(((texel // view[0]) >> 4) * ((view[0] + 15) >> 4) + ((texel % view[0]) >> 4))
        assert per_bin.max() > 4096 and np.bincount(texel).max() > 256
        t.dispose()
    check_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 41), color_map(), least=20_000, crowded=True)


# ---- (c) lines clipped at the view's edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_lines_clipped_at_the_edge(programs, which, with_vertex):
    fx = load(os.path.join(GOLDEN, "deposit_border_48.npz"))
    m = fx["meta"]
    view = tuple(m["viewRes"])
    assert np.abs(fx["current"][..., :2]).max() > 1.0            # positions reach beyond the view
    for name in ("vignette", "mirror"):
        check_pass(programs, name, which, with_vertex, view, fx["current"], fx["previous"], base_flow(view, 51), color_map(), least=1000,
                   time=m["time"], view_size=m["viewSize"], speed_limit=m["speedLimit"])


# ---- (d) the repeats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pool", "widen", "abandon"])
@pytest.mark.parametrize("which,with_vertex", [(FLOW_PASS, False), (VIEW_PASS, True)], ids=["flow-builtin", "view-program"])
def test_repeated_and_abandoned_passes_apply_the_stage_once(programs, case, which, with_vertex):
    """a pool of 8 pages runs dry and the pass is repeated; lists of 2 pages at first are widened and the pass is repeated; lists
    of 2 pages that may not be widened leave the pass to the stream-ordered pipeline - the stage ran over every attempt's store"""
    view = (96, 54)
    spread, seed, tune, expect = dict(pool=(0.2, 5, dict(bins_pool=8), BINS), widen=(0.2, 5, dict(bins_pool=8, bins_pages=2), BINS),
                                      abandon=(0.02, 7, dict(bins_pool=8, bins_pages=-2), STREAM))[case]
    cur, prev = crowd_inputs(256, spread, seed)
    for name in ("vignette", "mirror"):
        check_pass(programs, name, which, with_vertex, view, cur, prev, base_flow(view, 61), color_map(), expect=expect, tune=tune,
                   least=20_000, again=True)


# ---- (e) ring formats and shapes through the bins ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [FLOW_PASS, VIEW_PASS], ids=["flow", "view"])
@pytest.mark.parametrize("shape", ["packed", "drifting"])
def test_packed_rings_and_drifting_shapes(programs, shape, which):
    """with the library's vertex stage both go through the bins; a vertex program reads the slot's own f32 texel, so the same
    inputs go stream-ordered (the gate of deposit_prepare) - with the same bits"""
    n, view, fmt = (48, (97, 61), "f16") if shape == "packed" else (100, (160, 90), "f32")
    cur, prev = deposit_hashed_inputs(n, 71 + n, 1.05, 0.08, 11)
    for with_vertex, expect in ((False, BINS), (True, STREAM)):
        check_pass(programs, "vignette", which, with_vertex, view, cur, prev, base_flow(view, 72), color_map(), expect=expect, fmt=fmt)


# ---- (f) the point of it: the ring keeps its sorted slots ----------------------------------------------------------------------------
def loop_state(n=48):
    st = np.zeros((n, n, 4), f32)
    rng = np.random.default_rng(63)
    st[..., :2] = rng.uniform(-.9, .9, (n, n, 2))
    st[..., 2:] = rng.uniform(-.008, .008, (n, n, 2))
    return st


def looped(view, st, **made):
    """built-in steps and binned draws: the ring lies in tile-sorted slots (the recipe of
    tests/test_gpu_fragment_program.py::test_a_tile_sorted_ring_goes_to_texel_order_and_draws_the_same_bits)"""
    t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map(), **made)
    assert t.particles.option("bucket", 1) == 1
    t.particles.draw_pipeline("bins")
    t.timer.time = 1000.0
    for k in range(3):
        t.timer.tick()
        t.step()
        if k < 2:
            t.draw()
    return t


@pytest.mark.parametrize("which,with_vertex", PASSES, ids=PASS_IDS)
def test_a_tile_sorted_ring_stays_sorted_and_draws_the_same_bits(programs, which, with_vertex):
    view, st = (33, 31), loop_state()
    held, read = looped(view, st), looped(view, st)
    assert held.particles.option("stage_bins", 1) == 1
    assert sorted_buffers(held) > 0
    ring = read.particles.read(0), read.particles.read(1)          # (reading takes `read` to texel order)
    assert sorted_buffers(read) == 0 and sorted_buffers(held) > 0
    vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(held)
    want_n = stages_run(read, which, vertex, programs["vignette"], u)
    assert last_draw(read) == (STREAM, want_n)
    assert stages_run(held, which, vertex, programs["vignette"], u) == want_n > 300
    assert last_draw(held) == (BINS, want_n)
    assert sorted_buffers(held) > 0                                 # the ring is still in its sorted slots
    assert same(target(held, which), target(read, which))
    for b in range(2):
        assert bits_equal(held.particles.read(b), ring[b]).all()
    held.dispose()
    read.dispose()


def test_a_frame_loop_with_stages_equals_the_loop_with_the_option_off(programs):
    """step(); draw() with a fragment stage in both passes, a vertex program in the view pass: target for target, every frame"""
    view, st = (33, 31), loop_state()
    frag, render = programs["vignette"], programs["view"]
    loops = []
    for stage_bins in (1, 0):
        t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map(), flowShader=(None, frag), renderShader=(render, frag))
        assert t.particles.option("bucket", 1) == 1
        binned(t, stage_bins)
        t.timer.time = 1000.0
        loops.append(t)
    on, off = loops
    u = uniforms_of(on)
    for t in loops:
        t.uniforms["render"].update({k: u[k] for k in ("tint", "invRes", "edge", "gain")})
    for frame in range(3):
        for t in loops:
            t.timer.tick()
            t.step()
            t.draw()
        assert (on.fragments, on.view_fragments) == (off.fragments, off.view_fragments) and on.fragments > 300, frame
        assert last_draw(on) == (BINS, on.view_fragments) and last_draw(off) == (STREAM, off.view_fragments)
        assert bits_equal(on.flow.read(), off.flow.read()).all(), frame
        assert (on.read_view() == off.read_view()).all() and on.read_view().any(), frame
    assert sorted_buffers(on) > 0 and sorted_buffers(off) == 0
    for b in range(2):
        assert bits_equal(on.particles.read(b), off.particles.read(b)).all()
    for t in loops:
        t.dispose()


# ---- (g) nothing of a stage outlives its pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["auto", "bins"])
def test_builtin_passes_after_a_binned_stage_pass_are_a_fresh_contexts(programs, policy):
    n, view = 16, (64, 48)
    cur, prev = deposit_hashed_inputs(n, 55, 1.05, 0.08, 3)
    base, cmap = base_flow(view, 56), color_map()
    staged, fresh = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
    for t in (staged, fresh):
        t.particles.draw_pipeline(policy)
    assert staged.particles.option("stage_bins", 1) == 1
    u = uniforms_of(staged)
    pipeline = BINS if policy == "bins" else STREAM  # (auto: 256 particles are never tile-sorted)

    def builtin_run(t):
        t.flow.set_pixels(base)
        t.clearView()
        counts = []
        for which in (FLOW_PASS, VIEW_PASS):
            counts.append(plain_run(t, which, None, u))
            assert last_draw(t) == (pipeline, counts[-1])
        return counts, t.flow.read(), t.read_view()

    want = builtin_run(fresh)
    assert want[0][0] == want[0][1] > 50
    for vertex_too in (False, True):
        for which in (FLOW_PASS, VIEW_PASS):
            count = stages_run(staged, which, vertex_of(programs, which, vertex_too), programs["vignette"], u)
            assert count > 50 and last_draw(staged) == (pipeline, count)      # the stage pass takes the built-in pass's pipeline
        got = builtin_run(staged)
        assert got[0] == want[0] and bits_equal(got[1], want[1]).all() and (got[2] == want[2]).all(), vertex_too
    assert not bits_equal(want[1], base).all() and want[2].any()
    staged.dispose()
    fresh.dispose()


def test_with_the_option_off_a_stage_pass_is_stream_ordered_under_policy_bins(programs):
    n, view = 16, (64, 48)
    cur, prev = deposit_hashed_inputs(n, 55, 1.05, 0.08, 3)
    t = make(view, cur, prev, base_flow(view, 56), color_map())
    t.particles.draw_pipeline("bins")
    assert t.particles.option("stage_bins") == 0                    # the default
    for which in (FLOW_PASS, VIEW_PASS):
        count = stages_run(t, which, None, programs["vignette"], uniforms_of(t))
        assert count > 50 and last_draw(t) == (STREAM, count)
    assert t.particles.option("stage_bins", 1) == 1
    count = stages_run(t, FLOW_PASS, None, programs["vignette"], uniforms_of(t))
    assert last_draw(t) == (BINS, count)
    t.dispose()
