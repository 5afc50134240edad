"""Draw programs on row-band shards (include/tendrils_hip.h: th_draw_program_emit, th_draw_program_sharded;
tendrils_amd/csrc/th_draw_prelude.inc: th_draw_vertex_band_kernel): a caller's vertex stage in the passes of a sharded draw().
Every comparison is on the bits, and the reference of every one is the same programs through th_draw_program_run on an unsharded
context: the primitives in a world of one, two bands driven by the host (with and without their halo rows), the library's own
exchange over the in-process transport - through Tendrils.draw() -, mixed passes and widths, what the program sees of the
global stream on a band, a draw after steps over sorted slots, a rank-local failure, the refusals."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal
from test_gpu_draw_program import EVEN_LINES, FLOW, FROM_MAP, TAP_FLOW, VIEW, FlowUniforms, ViewUniforms, program_uniforms
from test_gpu_loopback import in_threads, inputs, make, world_of
from test_program_build import DRIFT
from test_screen_program_build import COPY

pytestmark = pytest.mark.gpu

# the flow stage's positions, and a colour that says what the program was handed: the line's stream index and the texture's
# height (r), vertex, column and the stream's height (g), the attribute and the buffer the lookup chose (b); opaque - a covered
# texel holds what the last line over it made.  (n <= 100: every integer here is exact in fp32.)
COORDS = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const FlowUniforms &u = th_uniforms<FlowUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(s.x * u.viewSize[0], s.y * u.viewSize[1]);
    o.color = make_float4((float)v.line + 16384.0f * v.dataRes.y,
                          (float)v.vertex + 512.0f * (float)v.column + 65536.0f * v.geomRes.y,
                          v.uv.x + 2.0f * v.uv.y + (v.from_current ? 4.0f : 0.0f), 1.0f);
    return o;
}
"""


@pytest.fixture(scope="module")
def programs():
    """every program of this module, compiled once"""
    from tendrils_amd.particles import DrawProgram, Program, ScreenProgram
    made = dict(flow=DrawProgram.from_source(FLOW, FlowUniforms, "flow_stage"),
                view=DrawProgram.from_source(VIEW, ViewUniforms, "view_stage"),
                even=DrawProgram.from_source(EVEN_LINES, FlowUniforms, "even_lines"),
                from_map=DrawProgram.from_source(FROM_MAP, FlowUniforms, "from_map"),
                tap=DrawProgram.from_source(TAP_FLOW, FlowUniforms, "tap_flow"),
                coords=DrawProgram.from_source(COORDS, FlowUniforms, "coords"),
                state=Program.from_source(DRIFT, name="drift"),
                screen=ScreenProgram.from_source(COPY, name="copy"))
    yield made
    for p in made.values():
        p.dispose()


def last_draw(t):
    from tendrils_amd import _capi
    info = _capi.DrawInfo()
    _capi.call("th_draw_query", t.particles._ctx, C.byref(info))
    return info


def with_shaders(t, flow=None, render=None):
    """the two shaders of a Tendrils; the restated view stage takes the sinTerm the built-in one computes"""
    t.flowShader, t.renderShader = flow, render
    t.uniforms["render"]["sinTerm"] = t.render_uniforms().sinTerm
    return t


# ---- 1. a world of one: the primitives -------------------------------------------------------------------------------------------
def test_emit_and_merge_on_a_whole_texture_equal_the_program_run(programs):
    from tendrils_amd import _capi, sharding
    n, view = 64, (96, 54)
    cur, prev, base = inputs(n, view, 101)
    cmap = np.random.default_rng(102).uniform(0, 1, (2 * n, n, 4)).astype(np.float32)
    one, em = make(n, view, cur, prev, base), make(n, view, cur, prev, base)
    for t in (one, em):
        t.colorMap.set_pixels(cmap)
    sharding.set_owners(em, 1)
    for name in ("flow", "even", "from_map", "tap", "coords"):
        for t in (one, em):
            t.flow.set_pixels(base)
        want_n = one._draw_program(programs[name], _capi.TH_PASS_FLOW, program_uniforms(one))
        keys, colors = sharding.emit_program_fragments(em, programs[name], _capi.TH_PASS_FLOW, program_uniforms(em))
        assert int(keys.numel()) == want_n > 500, name
        info = last_draw(em)
        assert info.pipeline == 0 and info.fragments == want_n         # TH_DRAW_STREAM
        sharding.merge_fragments(em, keys, colors)
        want = one.flow.read()
        assert not bits_equal(want, base).all()
        assert bits_equal(em.flow.read(), want).all(), name
    want_n = one._draw_program(programs["view"], _capi.TH_PASS_VIEW, program_uniforms(one))
    keys, colors = sharding.emit_program_fragments(em, programs["view"], _capi.TH_PASS_VIEW, program_uniforms(em))
    assert int(keys.numel()) == want_n > 500
    sharding.merge_view_fragments(em, keys, colors)
    want = one.read_view()
    assert want.any() and (em.read_view() == want).all()
    for b in range(2):                             # the ring is untouched
        assert bits_equal(em.particles.read(b), (cur, prev)[b]).all()
    for t in (one, em):
        t.dispose()


# ---- 2. two bands driven by the host: the halo rows ------------------------------------------------------------------------------
def test_two_bands_need_and_use_their_halo_rows(programs):
    """Texture height 100: the lookup of line 53's vertices lands on row 52.  A band that starts at row 53 cannot run the program
    without the neighbour's last row - the error of the built-in emit, nothing handed out - and is exact with it."""
    import torch
    import tendrils_amd as ta
    from tendrils_amd import _capi, sharding
    lib = _capi.load()
    n, view, world = 100, (96, 54), 2
    cur, prev, base = inputs(n, view, 103)
    bands = [(0, 53), (53, 47)]
    shards = [make(n, view, cur, prev, base, band) for band in bands]
    for t in shards:
        sharding.set_owners(t, world)
    with pytest.raises(ta.TendrilsHipError) as e:          # the precondition: this split does read across the bands
        sharding.emit_fragments(shards[1])
    assert e.value.status == _capi.TH_ERR_UNSUPPORTED and "halo" in str(e.value)
    block = programs["flow"].pack(program_uniforms(shards[1]))
    count, kp, cp = C.c_uint64(7), C.c_void_p(1), C.c_void_p(1)
    status = lib.th_draw_program_emit(shards[1].particles._ctx, programs["flow"].handle, C.byref(block), C.sizeof(block), _capi.TH_PASS_FLOW,
                                      C.byref(count), C.byref(kp), C.byref(cp))
    assert status == _capi.TH_ERR_UNSUPPORTED and b"halo" in lib.th_last_error(), lib.th_last_error()
    assert count.value == 0 and not kp.value and not cp.value
    edges = [sharding.edge_rows(t) for t in shards]
    sharding.set_halo(shards[0], None, edges[1][0].contiguous())
    sharding.set_halo(shards[1], edges[0][1].contiguous(), None)
    texels = view[0] * view[1]
    chunk = sharding.owner_chunk(texels, world)
    one = make(n, view, cur, prev, base)
    for name in ("flow", "coords"):
        for t in [one] + shards:
            t.flow.set_pixels(base)
        want_n = one._draw_program(programs[name], _capi.TH_PASS_FLOW, program_uniforms(one))
        want = one.flow.read().reshape(-1, 4)
        emitted = []
        for t in shards:
            keys, colors = sharding.emit_program_fragments(t, programs[name], _capi.TH_PASS_FLOW, program_uniforms(t))
            emitted.append((keys.clone(), colors.clone()))
        assert sum(int(k.numel()) for k, _ in emitted) == want_n > 1000
        sends = [sharding.split_by_owner(k, texels, world) for k, _ in emitted]
        for d, t in enumerate(shards):             # the all-to-all by hand: from every source in rank order, the part addressed to d
            lo = [sum(sends[s][:d]) for s in range(world)]
            rk = torch.cat([emitted[s][0][lo[s]:lo[s] + sends[s][d]] for s in range(world)]).contiguous()
            rc = torch.cat([emitted[s][1][lo[s]:lo[s] + sends[s][d]] for s in range(world)]).contiguous()
            sharding.merge_fragments(t, rk, rc)
            got = t.flow.read().reshape(-1, 4)
            assert bits_equal(got[d * chunk:(d + 1) * chunk], want[d * chunk:(d + 1) * chunk]).all(), (name, d)
    for t in [one] + shards:
        t.dispose()


# ---- 3. the library's exchange over the in-process transport, through Tendrils.draw() -------------------------------------------
@pytest.mark.parametrize("n,view,world,fmt", [(64, (96, 54), 2, "f32"), (100, (50, 27), 3, "f32"), (128, (50, 27), 4, "f32"),
                                              (100, (50, 27), 4, "f16")])
def test_draw_with_programs_over_loopback_equals_unsharded(programs, n, view, world, fmt):
    cur, prev, base = inputs(n, view, 7 * n + world)
    one = with_shaders(make(n, view, cur, prev, base, None, fmt), programs["flow"], programs["view"])
    if fmt == "f16":                               # what the packed texels decode to is what everybody draws
        cur, prev = one.particles.read(0), one.particles.read(1)
    one.draw()
    want_flow, want_view, want_frags, want_view_frags = one.flow.read(), one.read_view(), one.fragments, one.view_fragments
    one.dispose()
    built_in = make(n, view, cur, prev, base, None, fmt)
    built_in.draw()                                # these programs restate the library's stages
    assert bits_equal(built_in.flow.read(), want_flow).all() and (built_in.read_view() == want_view).all()
    assert built_in.fragments == want_frags == want_view_frags > 1000 and want_view.any()
    built_in.dispose()
    shards = [with_shaders(t, programs["flow"], programs["view"]) for t in world_of(n, view, world, cur, prev, base, fmt)]
    for frame in range(2):                         # (the second draw: over the buffers the first one left)
        _, err = in_threads(world, lambda r: shards[r].draw())
        assert err == [None] * world, err
        if frame == 0:
            assert sum(t.fragments for t in shards) == want_frags and sum(t.view_fragments for t in shards) == want_view_frags
            for t in shards:
                assert last_draw(t).pipeline == 0              # TH_DRAW_STREAM
                assert bits_equal(t.flow.read(), want_flow).all()
                assert (t.read_view() == want_view).all()
    for t in shards:
        t.dispose()


# ---- 4. a program in one pass alone; two widths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["flow shader alone", "render shader alone", "both, two widths"])
def test_mixed_passes_and_widths_equal_unsharded(programs, how):
    n, view, world = 64, (96, 54), 2
    widths = (2, 1) if how == "both, two widths" else None
    flow = None if how == "render shader alone" else programs["flow"]
    render = None if how == "flow shader alone" else programs["view"]
    cur, prev, base = inputs(n, view, 104)
    one = with_shaders(make(n, view, cur, prev, base, widths=widths), flow, render)
    one.draw()
    want_flow, want_view = one.flow.read(), one.read_view()
    assert one.fragments > 1000 and one.view_fragments > 1000 and want_view.any()
    from tendrils_amd import sharding
    ident = sharding.loopback_id()
    shards = [with_shaders(make(n, view, cur, prev, base, sharding.shard_rows(n, world, r), widths=widths), flow, render) for r in range(world)]
    _, err = in_threads(world, lambda r: sharding.comm_join(shards[r].particles._ctx, ident, r, world))
    assert err == [None] * world, err
    _, err = in_threads(world, lambda r: shards[r].draw())
    assert err == [None] * world, err
    assert sum(t.fragments for t in shards) == one.fragments and sum(t.view_fragments for t in shards) == one.view_fragments
    for t in shards:
        assert bits_equal(t.flow.read(), want_flow).all() and (t.read_view() == want_view).all()
    for t in [one] + shards:
        t.dispose()


# ---- 5. what the program is handed on a band: the global stream ------------------------------------------------------------------
@pytest.mark.parametrize("how", ["coords", "even lines"])
def test_a_band_hands_the_program_the_global_stream(programs, how):
    """a local row, a local `line` or the band's height in dataRes / geomRes would show here"""
    n, view, world = 100, (50, 27), 3
    flow, render = (programs["coords"], programs["coords"]) if how == "coords" else (programs["even"], None)
    cur, prev, base = inputs(n, view, 105)
    one = with_shaders(make(n, view, cur, prev, base), flow, render)
    one.draw()
    want_flow, want_view = one.flow.read(), one.read_view()
    assert one.fragments > 1000 and not bits_equal(want_flow, base).all()
    shards = [with_shaders(t, flow, render) for t in world_of(n, view, world, cur, prev, base)]
    _, err = in_threads(world, lambda r: shards[r].draw())
    assert err == [None] * world, err
    assert sum(t.fragments for t in shards) == one.fragments
    for t in shards:
        assert bits_equal(t.flow.read(), want_flow).all() and (t.read_view() == want_view).all()
    for t in [one] + shards:
        t.dispose()


# ---- 6. after a step over sorted slots -------------------------------------------------------------------------------------------
def test_a_program_draw_after_a_step_over_sorted_slots(programs):
    n, view, world = 128, (50, 27), 2
    cur, prev, base = inputs(n, view, 106)
    one = with_shaders(make(n, view, cur, prev, base), programs["flow"], programs["view"])
    shards = [with_shaders(t, programs["flow"], programs["view"]) for t in world_of(n, view, world, cur, prev, base)]
    everybody = [one] + shards
    for t in everybody:
        t.particles.option("bucket", 1)
        t.state["noiseWeight"] = 0.0005
        t.timer.tick()
        t.step()
    one.draw()
    _, err = in_threads(world, lambda r: shards[r].draw())
    assert err == [None] * world, err
    want_flow, want_view = one.flow.read(), one.read_view()
    assert sum(t.fragments for t in shards) == one.fragments > 1000
    for t in shards:
        assert bits_equal(t.flow.read(), want_flow).all() and (t.read_view() == want_view).all()
    for b in range(2):
        whole = np.concatenate([t.particles.read(b) for t in shards])
        assert bits_equal(whole, one.particles.read(b)).all()
    for t in everybody:
        t.dispose()


# ---- 7. a rank-local failure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [2, 3])
def test_a_rank_local_failure_ends_the_program_draw_on_every_rank(programs, stage):
    """the host-side status injection of the built-in sharded draw's test (TH_OPT_INJECT_FAILURE: while rasterising / making
    room): the rank reports it, the others name the rank, nothing is blended, nobody waits - and the next draw works"""
    import tendrils_amd as ta
    from tendrils_amd import sharding
    n, view, world, bad = 64, (96, 54), 3, 1
    cur, prev, base = inputs(n, view, 5)
    one = with_shaders(make(n, view, cur, prev, base), programs["flow"], programs["view"])
    one.draw()
    want_flow, want_view = one.flow.read(), one.read_view()
    one.dispose()
    shards = [with_shaders(t, programs["flow"], programs["view"]) for t in world_of(n, view, world, cur, prev, base)]
    shards[bad].particles.option("inject_failure", stage)
    _, err = in_threads(world, lambda r: sharding.draw_sharded_native(shards[r], view=True))
    assert all(isinstance(e, ta.TendrilsHipError) for e in err), err
    assert "injected failure" in str(err[bad])
    for r in range(world):
        if r != bad:
            assert "rank %d failed" % bad in str(err[r]), str(err[r])
    for t in shards:
        assert bits_equal(t.flow.read(), base).all() and not t.read_view().any()
    assert shards[bad].particles.option("inject_failure") == 0
    _, err = in_threads(world, lambda r: sharding.draw_sharded_native(shards[r], view=True))
    assert err == [None] * world, err
    for t in shards:
        assert bits_equal(t.flow.read(), want_flow).all() and (t.read_view() == want_view).all()
        t.dispose()


# ---- 8. refusals: nothing launched, the targets untouched -------------------------------------------------------------------------
def test_refusals_launch_nothing(programs):
    from tendrils_amd import _capi
    lib = _capi.load()
    n, view = 64, (96, 54)
    cur, prev, base = inputs(n, view, 107)
    t, = world_of(n, view, 1, cur, prev, base)
    alone = make(n, view, cur, prev, base)         # no communicator
    ctx = t.particles._ctx
    flow, block = programs["flow"].handle, programs["flow"].pack(program_uniforms(t))
    ref, size = C.byref(block), C.sizeof(block)
    big = (C.c_uint8 * 1025)()
    d = _capi.DepositUniforms(time=2500.0, speedLimit=0.01)
    d.viewSize[0] = d.viewSize[1] = 1.0
    u = t.render_uniforms()
    a, b = C.c_uint64(7), C.c_uint64(7)

    def sharded(ctx, fp, fu, fb, du, vp, vu, vb, ru):
        return lib.th_draw_program_sharded(ctx, fp, fu, fb, du, vp, vu, vb, ru, C.byref(a), C.byref(b))
    cases = [("both programs null", lambda: sharded(ctx, None, None, 0, C.byref(d), None, None, 0, C.byref(u)), b"th_draw_sharded"),
             ("a state program", lambda: sharded(ctx, programs["state"].handle, None, 0, None, None, None, 0, None), b"state program"),
             ("a screen program", lambda: sharded(ctx, flow, ref, size, None, programs["screen"].handle, None, 0, None), b"screen program"),
             ("1025 bytes", lambda: sharded(ctx, flow, C.byref(big), 1025, None, None, None, 0, None), b"1025"),
             ("null uniforms with a size", lambda: sharded(ctx, flow, None, 16, None, None, None, 0, None), b"null uniforms"),
             ("null uniforms with a size, view", lambda: sharded(ctx, flow, ref, size, None, flow, None, 16, None), b"null uniforms"),
             ("no built-in uniforms", lambda: sharded(ctx, None, None, 0, None, flow, ref, size, None), b"null uniforms"),
             ("no communicator", lambda: sharded(alone.particles._ctx, flow, ref, size, None, None, None, 0, None), b"th_comm_init")]
    n_out, kp, cp = C.c_uint64(7), C.c_void_p(1), C.c_void_p(1)
    outs = (C.byref(n_out), C.byref(kp), C.byref(cp))
    cases += [("unknown pass", lambda: lib.th_draw_program_emit(ctx, flow, ref, size, 2, *outs), b"unknown pass"),
              ("null outputs", lambda: lib.th_draw_program_emit(ctx, flow, ref, size, 0, None, None, None), b"null outputs"),
              ("a state program, emit", lambda: lib.th_draw_program_emit(ctx, programs["state"].handle, None, 0, 0, *outs), b"state program"),
              ("1025 bytes, emit", lambda: lib.th_draw_program_emit(ctx, flow, C.byref(big), 1025, 0, *outs), b"1025")]
    for name, call, says in cases:
        assert call() == _capi.TH_ERR_INVALID, (name, lib.th_last_error())
        assert says in lib.th_last_error(), (name, lib.th_last_error())
    assert a.value == 7 and b.value == 7 and n_out.value == 7 and kp.value == 1 and cp.value == 1
    for c in (t, alone):
        assert bits_equal(c.flow.read(), base).all() and not c.read_view().any()
        c.dispose()
