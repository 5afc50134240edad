"""Fragment programs on the GPU (include/tendrils_hip.h "fragment programs"; tendrils_amd/csrc/th_fragprog.hip and
th_fragment_prelude.inc): a caller's fragment stage in the passes of draw().  No expected value comes from the code under test:
the reference of a pass is the EXISTING emit of a whole-texture context (th_deposit_emit / th_view_emit / th_draw_program_emit),
its fragments taken to the host, the fragment function restated here in numpy's fp32 and applied with x, y from the key's texel
field, and the fragments put back and blended by the existing th_deposit_merge / th_view_merge.  The programs use + - *, fminf /
fmaxf and selects only, which numpy reproduces exactly with contraction off: every comparison is bit for bit on the flow field
and byte for byte on the RGBA8 view."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, deposit_hashed_inputs, load
from test_draw_program_build import FLOW
from test_fragment_program_build import IDENTITY, VIGNETTE, FragUniforms
from test_gpu_draw_program import VIEW, FlowUniforms, ViewUniforms
from test_program_build import DRIFT

pytestmark = pytest.mark.gpu

FLOW_PASS, VIEW_PASS = 0, 1          # TH_PASS_FLOW, TH_PASS_VIEW
STREAM = 0                           # TH_DRAW_STREAM
INERT = [-1e6, -1e6, 0, 0]
f32 = np.float32


@pytest.fixture(scope="module")
def programs():
    """every program of this module, compiled once"""
    from tendrils_amd.particles import DrawProgram, FragmentProgram, Program
    made = dict(identity=FragmentProgram.from_source(IDENTITY, name="identity"),
                vignette=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"),
                flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"),
                view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"),
                state=Program.from_source(DRIFT, name="drift"))
    yield made
    for p in made.values():
        p.dispose()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def tap_nearest(u, n):
    """th_tap_nearest (th_taps.inc)"""
    f = np.floor(u * f32(n))
    return np.where(~(f > 0), 0, np.where(f > f32(n - 1), n - 1, f.astype(np.int64))).astype(np.int64)


def vignette_np(color, x, y, view_res, which, u, cmap):
    """VIGNETTE (tests/test_fragment_program_build.py) in fp32, operation for operation"""
    cx, cy = x.astype(f32) + f32(0.5), y.astype(f32) + f32(0.5)
    dx, dy = cx - f32(0.5) * f32(view_res[0]), cy - f32(0.5) * f32(view_res[1])
    fall = np.maximum(f32(1.0) - (dx * dx + dy * dy) * f32(u["edge"]), f32(0.25))
    m = cmap[tap_nearest(cy * f32(u["invRes"][1]), cmap.shape[0]), tap_nearest(cx * f32(u["invRes"][0]), cmap.shape[1])]
    stripe = np.where((x + 3 * y) & 1, f32(u["gain"]), f32(1.0)).astype(f32)
    k = fall * stripe
    tint = [f32(v) for v in u["tint"]]
    out = np.empty_like(color)
    out[:, 0] = color[:, 0] * k + m[:, 0] * tint[0]
    out[:, 1] = color[:, 1] * k + m[:, 1] * tint[1]
    out[:, 2] = color[:, 2] * k + m[:, 2] * tint[2] if which == VIEW_PASS else color[:, 2]
    out[:, 3] = np.minimum(color[:, 3] * tint[3] + m[:, 3] * f32(0.125), f32(1.0))
    return out


def identity_np(color, x, y, view_res, which, u, cmap):
    return color


RESTATED = dict(identity=identity_np, vignette=vignette_np)


# ---- contexts and calls ------------------------------------------------------------------------------------------------------------
def color_map(seed=77, shape=(7, 13)):
    return np.random.default_rng(seed).uniform(0, 1, shape + (4,)).astype(f32)


def base_flow(view, seed):
    rng = np.random.default_rng(seed)
    base = np.zeros((view[1], view[0], 4), f32)
    base[..., :2] = rng.uniform(-.01, .01, (view[1], view[0], 2))
    base[..., 2] = 2400.0
    base[..., 3] = rng.uniform(0, 1, (view[1], view[0]))
    return base


def make(view, cur, prev, base, cmap=None, widths=None, fmt="f32", band=None, time=2500.0, view_size=None, speed_limit=None, **options):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    n = cur.shape[1]
    opts = ta.defaults()
    opts.update(options)
    if widths:                                      # a GL that honours gl.lineWidth up to 4: (flowWidth, lineWidth)
        opts["lineWidthRange"] = (1, 4)
        opts["state"]["flowWidth"], opts["state"]["lineWidth"] = widths
    row0, rows = band if band else (0, n)
    opts.update(row0=row0, rows=rows, globalHeight=n, stateFormat=ta._capi.TH_STATE_F16 if fmt == "f16" else ta._capi.TH_STATE_F32)
    t = ta.Tendrils(View(*view), opts)
    t.resize()
    t.setup(n)
    if view_size is not None:
        t.viewSize[:] = view_size
    if speed_limit is not None:
        t.state["speedLimit"] = speed_limit
    t.particles.upload_texels(cur[row0:row0 + rows], 0)
    t.particles.upload_texels(prev[row0:row0 + rows], 1)
    t.flow.set_pixels(base)
    if cmap is not None:
        t.colorMap.set_pixels(cmap)
    t.timer.time = time
    t.state["baseColor"] = [1, 0.7, 0.3, 0.2]
    t.state["flowColor"] = [0.2, 1, 0.9, 0.1]
    t.state["speedAlpha"] = 0.0005
    t.line_widths()
    return t


def uniforms_of(t):
    """what both stages' blocks are packed from: the vertex programs' fields and the fragment program's"""
    fw, fh = t.viewRes
    return dict(t.state, time=float(t.timer.time), viewSize=t.viewSize, sinTerm=t.render_uniforms().sinTerm,
                tint=[0.5, 0.25, 0.75, 0.875], invRes=[f32(1.0) / f32(fw), f32(1.0) / f32(fh)], edge=f32(3.5) / f32(fw * fw + fh * fh), gain=0.625)       # (edge: the vignette's floor binds in the corners)


def last_draw(t):
    from tendrils_amd import _capi
    info = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(info))
    return info.pipeline, info.fragments


def stages_of(t, which, vertex, fragment, uniforms):
    from tendrils_amd.particles import draw_stages
    builtin = t.render_uniforms() if which == VIEW_PASS else t.deposit_uniforms()
    return draw_stages(vertex, fragment, uniforms, builtin)


def stages_run(t, which, vertex, fragment, uniforms):
    """th_draw_stages_run: the fragments it reports"""
    from tendrils_amd import _capi
    stages, _keep = stages_of(t, which, vertex, fragment, uniforms)
    n = C.c_uint64(0)
    _capi.call("th_draw_stages_run", t.particles._ctx, C.byref(stages), which, C.byref(n))
    return int(n.value)


def plain_run(t, which, vertex, uniforms):
    """the pass without a fragment stage, through the call that has always drawn it"""
    from tendrils_amd import _capi
    n = C.c_uint64(0)
    if vertex is not None:
        return t._draw_program(vertex, which, uniforms)
    if which == VIEW_PASS:
        u = t.render_uniforms()
        _capi.call("th_view_draw", t.particles._ctx, C.byref(u), C.byref(n))
    else:
        u = t.deposit_uniforms()
        _capi.call("th_flow_deposit", t.particles._ctx, C.byref(u), C.byref(n))
    return int(n.value)


def target(t, which):
    return t.read_view() if which == VIEW_PASS else t.flow.read()


def same(a, b):
    return (a == b).all() if a.dtype == np.uint8 else bits_equal(a, b).all()


def reference_pass(t, which, vertex, name, uniforms, cmap):
    """steps 1 - 4 of the module's docstring on the whole-texture context `t`: the fragments blended"""
    import torch
    from tendrils_amd import sharding
    if vertex is not None:
        keys, colors = sharding.emit_program_fragments(t, vertex, which, uniforms)
    else:
        keys, colors = sharding.emit_view_fragments(t) if which == VIEW_PASS else sharding.emit_fragments(t)
    if not keys.numel():
        return 0
    k = keys.cpu().numpy().astype(np.uint64)
    texel = ((k >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.int64)
    fw, fh = t.viewRes
    assert texel.max() < fw * fh
    made = RESTATED[name](colors.cpu().numpy(), texel % fw, texel // fw, (fw, fh), which, uniforms,
                          cmap if cmap is not None else np.zeros((1, 1, 4), f32))
    put = torch.from_numpy(np.ascontiguousarray(made, f32)).cuda().contiguous()
    (sharding.merge_view_fragments if which == VIEW_PASS else sharding.merge_fragments)(t, keys.clone(), put)
    return int(keys.numel())


def vertex_of(programs, which, with_vertex):
    return (programs["view"] if which == VIEW_PASS else programs["flow"]) if with_vertex else None


def check_against_reference(programs, name, view, cur, prev, base, cmap, least=300, **options):
    """both passes, with the built-in vertex stage and with a vertex program: th_draw_stages_run against the reference"""
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            got, ref = make(view, cur, prev, base, cmap, **options), make(view, cur, prev, base, cmap, **options)
            vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(got)
            n = stages_run(got, which, vertex, programs[name], u)
            want_n = reference_pass(ref, which, vertex, name, u, cmap)
            assert n == want_n >= least, (which, with_vertex, n, want_n)
            assert last_draw(got) == (STREAM, n)
            assert same(target(got, which), target(ref, which)), (name, which, with_vertex)
            if name != "identity":                  # the stage did something: the pass without it leaves other bits
                ref.flow.set_pixels(base)
                ref.clearView()
                plain_run(ref, which, vertex, u)
                assert not same(target(got, which), target(ref, which))
            for b in range(2):                      # the ring is untouched
                assert bits_equal(got.particles.read(b), (cur, prev)[b]).all()
            got.dispose()
            ref.dispose()


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------
def test_the_identity_stage_draws_what_the_pass_without_it_draws(programs):
    n, view = 48, (96, 54)
    cur, prev = deposit_hashed_inputs(n, 11, 1.1, 0.06, 13)
    base, cmap = base_flow(view, 12), color_map()
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            got, plain = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
            vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(got)
            frags = stages_run(got, which, vertex, programs["identity"], u)
            want = plain_run(plain, which, vertex, u)
            assert frags == want > 300
            assert last_draw(got) == (STREAM, frags)
            assert same(target(got, which), target(plain, which))
            assert not same(target(got, which), np.zeros_like(target(got, which)) if which == VIEW_PASS else base)
            for b in range(2):
                assert bits_equal(got.particles.read(b), (cur, prev)[b]).all()
            if vertex is not None:                  # no fragment program in the slot: the call is th_draw_program_run
                got.flow.set_pixels(base)
                got.clearView()
                assert stages_run(got, which, vertex, None, u) == want
                assert same(target(got, which), target(plain, which))
            got.dispose()
            plain.dispose()
    check_against_reference(programs, "identity", view, cur, prev, base, cmap)


# ---- 2. a stage that uses everything it is handed ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,view,widths", [(32, (64, 64), None), (48, (97, 61), None), (48, (160, 90), None), (32, (97, 61), (3, 3))],
                         ids=["32-64x64", "48-97x61", "48-160x90", "32-97x61-wide"])
def test_a_stage_of_position_uniforms_and_a_tap_equals_its_restatement(programs, n, view, widths):
    """97 x 61: neither a power of two nor square - a wrong row stride, or x and y swapped, shows; width 1, and one wide run"""
    cur, prev = deposit_hashed_inputs(n, 21 + n, 1.05, 0.08, 11)
    check_against_reference(programs, "vignette", view, cur, prev, base_flow(view, 22), color_map(), widths=widths)


def test_a_stage_without_a_colour_map_taps_the_zero_texture(programs):
    n, view = 32, (64, 64)
    cur, prev = deposit_hashed_inputs(n, 23, 1.0, 0.05, 0)
    check_against_reference(programs, "vignette", view, cur, prev, base_flow(view, 24), None)


# ---- 3. long and clipped lines: the emit-long and slow lists -----------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["deposit_long_lines_32", "deposit_border_48"])
def test_long_and_clipped_lines(programs, fixture):
    fx = load(os.path.join(GOLDEN, fixture + ".npz"))
    m = fx["meta"]
    view = tuple(m["viewRes"])
    check_against_reference(programs, "vignette", view, fx["current"], fx["previous"], base_flow(view, 31), color_map(), least=1000,
                            time=m["time"], view_size=m["viewSize"], speed_limit=m["speedLimit"])


# ---- 4. nothing to draw ----------------------------------------------------------------------------------------------------------------
def kernel_launches(t):
    from tendrils_amd import _capi
    ms, launches = C.c_float(0), C.c_int32(0)
    _capi.call("th_kernel_timing_read", t.particles._ctx, C.byref(ms), C.byref(launches))
    return launches.value


def test_an_all_inert_state_has_no_fragments_and_launches_nothing(programs):
    from tendrils_amd import _capi
    n, view = 32, (64, 64)
    inert = np.tile(np.array(INERT, f32), (n, n, 1))
    base = base_flow(view, 41)
    t = make(view, inert, inert, base, color_map())
    _capi.call("th_kernel_timing", t.particles._ctx, 1)
    before = t.read_view()
    for which in (FLOW_PASS, VIEW_PASS):
        assert stages_run(t, which, None, programs["vignette"], uniforms_of(t)) == 0
        assert last_draw(t) == (STREAM, 0)
    assert kernel_launches(t) == 0                 # (the event pair sits around the fragment kernel alone here)
    assert bits_equal(t.flow.read(), base).all() and (t.read_view() == before).all()
    live, _ = deposit_hashed_inputs(n, 42, 1.0, 0.05, 0)
    t.particles.upload_texels(live, 0)
    t.particles.upload_texels(live * f32(0.5), 1)
    assert stages_run(t, FLOW_PASS, None, programs["vignette"], uniforms_of(t)) > 0
    assert kernel_launches(t) == 1                 # ... and one launch covers a pass that has fragments
    t.dispose()


# ---- 5. emit + merge: the 64-bit keys ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owners", [1, 3])
def test_emit_and_merge_equal_the_run(programs, owners):
    from tendrils_amd import sharding
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 51, 1.05, 0.08, 11)
    base, cmap = base_flow(view, 52), color_map()
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            run, em = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
            sharding.set_owners(em, owners)
            vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(run)
            want_n = stages_run(run, which, vertex, programs["vignette"], u)
            keys, colors = sharding.emit_stage_fragments(em, vertex, programs["vignette"], which, u)        # th_draw_stages_emit
            assert int(keys.numel()) == want_n > 300 and last_draw(em) == (STREAM, want_n)
            seen = set((keys.cpu().numpy().astype(np.uint64) >> np.uint64(56)).tolist())
            assert seen == set(range(owners))       # the keys carry their owners, and every owner has fragments
            (sharding.merge_view_fragments if which == VIEW_PASS else sharding.merge_fragments)(em, keys, colors)
            assert same(target(em, which), target(run, which)), (which, with_vertex)
            run.dispose()
            em.dispose()


# ---- 5b. a stage is its pass's alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["auto", "bins"])
def test_builtin_passes_after_a_stage_pass_are_a_fresh_contexts(programs, policy):
    """After passes with a fragment stage - run, and emitted as the band of all rows - the built-in flow pass and view pass of the
    same context draw the bits, report the fragments and take the pipeline of a context that never saw a stage: nothing of a
    stage outlives its pass (a stage pass itself is stream-ordered whatever the policy; reuses nothing, leaves nothing to reuse)"""
    from tendrils_amd import sharding
    n, view = 16, (64, 48)
    cur, prev = deposit_hashed_inputs(n, 55, 1.05, 0.08, 3)
    base, cmap = base_flow(view, 56), color_map()
    staged, fresh = make(view, cur, prev, base, cmap), make(view, cur, prev, base, cmap)
    for t in (staged, fresh):
        t.particles.draw_pipeline(policy)
    u = uniforms_of(staged)
    pipeline = 1 if policy == "bins" else STREAM     # (TH_DRAW_BINS; auto: 256 particles are never tile-sorted)

    def builtin_run(t):
        t.flow.set_pixels(base)
        t.clearView()
        counts = []
        for which in (FLOW_PASS, VIEW_PASS):         # (the view pass may reuse the flow pass's geometry: c->drawn)
            counts.append(plain_run(t, which, None, u))
            assert last_draw(t) == (pipeline, counts[-1])
        return counts, t.flow.read(), t.read_view()

    def builtin_emit(t):
        t.flow.set_pixels(base)
        t.clearView()
        counts = []
        for emit, merge in ((sharding.emit_fragments, sharding.merge_fragments), (sharding.emit_view_fragments, sharding.merge_view_fragments)):
            keys, colors = emit(t)
            counts.append(int(keys.numel()))
            merge(t, keys, colors)
        return counts, t.flow.read(), t.read_view()

    want_run, want_emit = builtin_run(fresh), builtin_emit(fresh)
    assert want_run[0][0] == want_run[0][1] == want_emit[0][0] == want_emit[0][1] > 50
    for vertex_too in (False, True):
        for which in (FLOW_PASS, VIEW_PASS):
            assert stages_run(staged, which, vertex_of(programs, which, vertex_too), programs["vignette"], u) > 50
            assert last_draw(staged)[0] == STREAM
        got = builtin_run(staged)
        assert got[0] == want_run[0] and bits_equal(got[1], want_run[1]).all() and (got[2] == want_run[2]).all(), vertex_too
        for which in (FLOW_PASS, VIEW_PASS):
            keys, _colors = sharding.emit_stage_fragments(staged, vertex_of(programs, which, vertex_too), programs["vignette"], which, u)
            assert int(keys.numel()) > 50
        got = builtin_emit(staged)
        assert got[0] == want_emit[0] and bits_equal(got[1], want_emit[1]).all() and (got[2] == want_emit[2]).all(), vertex_too
    assert not bits_equal(want_run[1], base).all() and want_run[2].any()
    staged.dispose()
    fresh.dispose()


# ---- 6. packed rings and tile-sorted rings -------------------------------------------------------------------------------------------
def sorted_buffers(t):
    from tendrils_amd import _capi
    info = _capi.SlotOrderInfo()
    _capi.call("th_slot_order", t.particles._ctx, C.byref(info))
    return info.sorted_buffers


def test_a_packed_ring_draws_what_its_texels_decode_to(programs):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 61, 1.05, 0.08, 11)
    base, cmap = base_flow(view, 62), color_map()
    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            packed = make(view, cur, prev, base, cmap, fmt="f16")
            decoded = packed.particles.read(0), packed.particles.read(1)
            plain = make(view, decoded[0], decoded[1], base, cmap)
            vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(plain)
            want_n = stages_run(plain, which, vertex, programs["vignette"], u)
            assert stages_run(packed, which, vertex, programs["vignette"], u) == want_n > 300
            assert same(target(packed, which), target(plain, which))
            assert sorted_buffers(packed) == 0
            for b in range(2):
                assert bits_equal(packed.particles.read(b), decoded[b]).all()
            packed.dispose()
            plain.dispose()


def test_a_tile_sorted_ring_goes_to_texel_order_and_draws_the_same_bits(programs):
    n, view = 48, (33, 31)                         # (slots are sorted only where the texture has twice the field's texels)
    st = np.zeros((n, n, 4), f32)
    rng = np.random.default_rng(63)
    st[..., :2] = rng.uniform(-.9, .9, (n, n, 2))
    st[..., 2:] = rng.uniform(-.008, .008, (n, n, 2))

    def looped():
        """built-in steps and binned draws: the ring lies in tile-sorted slots"""
        t = make(view, st, st, np.zeros((view[1], view[0], 4), f32), color_map())
        assert t.particles.option("bucket", 1) == 1
        t.particles.draw_pipeline("bins")
        t.timer.time = 1000.0
        for k in range(3):
            t.timer.tick()
            t.step()
            if k < 2:
                t.draw()
        return t

    for which in (FLOW_PASS, VIEW_PASS):
        for with_vertex in (False, True):
            held, read = looped(), looped()
            assert sorted_buffers(held) > 0
            ring = read.particles.read(0), read.particles.read(1)          # (reading takes `read` to texel order)
            assert sorted_buffers(read) == 0 and sorted_buffers(held) > 0
            vertex, u = vertex_of(programs, which, with_vertex), uniforms_of(held)
            want_n = stages_run(read, which, vertex, programs["vignette"], u)
            assert stages_run(held, which, vertex, programs["vignette"], u) == want_n > 300
            assert last_draw(held) == (STREAM, want_n)
            assert sorted_buffers(held) == 0                                # afterwards the ring is in texel order
            assert same(target(held, which), target(read, which))
            for b in range(2):
                assert bits_equal(held.particles.read(b), ring[b]).all()
            held.dispose()
            read.dispose()


# ---- 7. what is refused ------------------------------------------------------------------------------------------------------------
def test_refusals_draw_nothing(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    n, view = 32, (64, 64)
    cur, prev = deposit_hashed_inputs(n, 71, 1.0, 0.05, 0)
    base = base_flow(view, 72)
    t = make(view, cur, prev, base, color_map())
    u = uniforms_of(t)
    view_before = t.read_view()
    frag, vert = programs["vignette"], programs["flow"]
    fblock, vblock = frag.pack(u), vert.pack(u)
    big = (C.c_uint8 * 1025)()
    d = t.deposit_uniforms()

    def stages(vertex=None, vu=None, vn=0, fragment=None, fu=None, fn=0, builtin=None):
        s = _capi.DrawStages()
        s.vertex, s.fragment = (vertex.handle if vertex else None), (fragment.handle if fragment else None)
        s.vertex_uniforms = C.cast(C.pointer(vu), C.c_void_p) if vu is not None else None
        s.fragment_uniforms = C.cast(C.pointer(fu), C.c_void_p) if fu is not None else None
        s.vertex_uniform_bytes, s.fragment_uniform_bytes = vn, fn
        s.builtin = C.cast(C.pointer(builtin), C.c_void_p) if builtin is not None else None
        return s

    fsize, vsize = C.sizeof(fblock), C.sizeof(vblock)
    cases = [("both stages null", stages(builtin=d), FLOW_PASS, ["th_flow_deposit", "th_view_draw"]),
             ("a draw program as the fragment stage", stages(fragment=vert, fu=vblock, fn=vsize, builtin=d), FLOW_PASS, ["draw program", "fragment program"]),
             ("a fragment program as the vertex stage", stages(vertex=frag, vu=fblock, vn=fsize), FLOW_PASS, ["draw program", "fragment program"]),
             ("a state program as the fragment stage", stages(fragment=programs["state"], builtin=d), FLOW_PASS, ["state program", "fragment program"]),
             ("1025 fragment uniform bytes", stages(fragment=frag, fu=big, fn=1025, builtin=d), FLOW_PASS, ["1025"]),
             ("1025 vertex uniform bytes", stages(vertex=vert, vu=big, vn=1025, fragment=frag, fu=fblock, fn=fsize), FLOW_PASS, ["1025"]),
             ("null fragment uniforms with a size", stages(fragment=frag, fn=fsize, builtin=d), FLOW_PASS, ["null"]),
             ("null vertex uniforms with a size", stages(vertex=vert, vn=vsize, fragment=frag, fu=fblock, fn=fsize), FLOW_PASS, ["null"]),
             ("no vertex program and no builtin", stages(fragment=frag, fu=fblock, fn=fsize), FLOW_PASS, ["builtin"]),
             ("an unknown pass", stages(fragment=frag, fu=fblock, fn=fsize, builtin=d), 2, ["pass 2"])]
    for what, s, which, words in cases:
        count, kp, cp = C.c_uint64(7), C.c_void_p(), C.c_void_p()
        for status in (lib.th_draw_stages_run(t.particles._ctx, C.byref(s), which, C.byref(count)),
                       lib.th_draw_stages_emit(t.particles._ctx, C.byref(s), which, C.byref(count), C.byref(kp), C.byref(cp))):
            assert status == _capi.TH_ERR_INVALID, what
            message = lib.th_last_error().decode()
            assert all(w in message for w in words) or (what == "both stages null" and "th_deposit_emit" in message), (what, message)
        assert not kp.value and not cp.value
        assert bits_equal(t.flow.read(), base).all() and (t.read_view() == view_before).all(), what
    assert lib.th_draw_stages_run(t.particles._ctx, None, FLOW_PASS, None) == _capi.TH_ERR_INVALID
    ok = stages(fragment=frag, fu=fblock, fn=fsize, builtin=d)
    assert lib.th_draw_stages_emit(t.particles._ctx, C.byref(ok), FLOW_PASS, None, None, None) == _capi.TH_ERR_INVALID      # null outputs
    # the other kinds' calls refuse a fragment program by name
    n_out = C.c_uint64(0)
    assert lib.th_draw_program_run(t.particles._ctx, frag.handle, C.byref(fblock), fsize, FLOW_PASS, C.byref(n_out)) == _capi.TH_ERR_INVALID
    assert b"fragment program" in lib.th_last_error() and b"draw program" in lib.th_last_error()
    assert lib.th_program_run(t.particles._ctx, frag.handle, None, 0, -1, -1) == _capi.TH_ERR_INVALID
    assert b"fragment program" in lib.th_last_error()
    assert bits_equal(t.flow.read(), base).all() and (t.read_view() == view_before).all()
    # ... while th_program_query serves it: no scratch, no LDS
    for name in ("identity", "vignette"):
        q = programs[name].query(t.particles)
        assert q["scratch_bytes"] == 0 and q["lds_bytes"] == 0 and q["code_bytes"] > 0, (name, q)
    t.dispose()
    # a row band: the local run is refused, nothing launched
    band = make(view, cur, prev, base, color_map(), band=(0, 16))
    s = stages(fragment=frag, fu=fblock, fn=fsize, builtin=d)
    assert lib.th_draw_stages_run(band.particles._ctx, C.byref(s), FLOW_PASS, C.byref(n_out)) == _capi.TH_ERR_UNSUPPORTED
    assert b"th_draw_stages_emit" in lib.th_last_error()
    assert bits_equal(band.flow.read(), base).all()
    # ... and draw() over the library-issued exchange names the host's route
    band.flowShader = frag
    with pytest.raises(NotImplementedError) as e:
        band.draw()
    assert "draw_sharded_programs" in str(e.value) and "th_draw_stages_emit" in str(e.value)
    assert bits_equal(band.flow.read(), base).all()
    band.dispose()


# ---- 8. the Python surface ---------------------------------------------------------------------------------------------------------
def test_tendrils_takes_fragment_programs_pairs_and_none(programs):
    n, view = 48, (97, 61)
    cur, prev = deposit_hashed_inputs(n, 81, 1.05, 0.08, 11)
    base, cmap = base_flow(view, 82), color_map()
    frag, flow, render = programs["vignette"], programs["flow"], programs["view"]
    for flow_shader, render_shader in (((None, frag), (render, frag)), (frag, [None, frag]), ((flow, None), frag)):
        t = make(view, cur, prev, base, cmap, flowShader=flow_shader, renderShader=render_shader)
        c = make(view, cur, prev, base, cmap)
        u = uniforms_of(c)
        t.uniforms["render"].update({k: u[k] for k in ("sinTerm", "tint", "invRes", "edge", "gain")})
        t.draw()
        from tendrils_amd.particles import shader_stages
        (fv, ff), (rv, rf) = shader_stages(flow_shader), shader_stages(render_shader)
        want_flow = stages_run(c, FLOW_PASS, fv, ff, u) if ff is not None else plain_run(c, FLOW_PASS, fv, u)
        c._bind_view(None)
        c.clearView()
        want_view = stages_run(c, VIEW_PASS, rv, rf, u)
        assert (t.fragments, t.view_fragments) == (want_flow, want_view) and want_flow > 300 and want_view > 300
        assert bits_equal(t.flow.read(), c.flow.read()).all() and (t.read_view() == c.read_view()).all()
        assert last_draw(t) == (STREAM, want_view)
        # the shaders removed: draw() is th_draw's again - one rasterisation for both passes, the bits of a context that never had any
        t.flowShader = t.renderShader = None
        never = make(view, cur, prev, base, cmap)
        for x in (t, never):
            x.flow.set_pixels(base)
            x.clearView()
            x.draw()
        assert t.fragments == t.view_fragments == never.fragments > 300
        assert bits_equal(t.flow.read(), never.flow.read()).all() and (t.read_view() == never.read_view()).all()
        for x in (t, c, never):
            x.dispose()
