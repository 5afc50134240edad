"""Tendrils.draw() on the host, the part that needs no GPU: which library calls each route of draw() makes, in which order and
with which arguments.  `call` is replaced by a recorder in the three modules that draw (tendrils_amd._capi - what sharding.py
calls through -, tendrils_amd.tendrils, tendrils_amd.particles); the programs are real DrawProgram / FragmentProgram objects
compiled through hiprtc.  Every expected sequence is written out: the whole texture and the band whose exchange the library
issues, no shaders / a flow DrawProgram / a render FragmentProgram / a (vertex, fragment) pair on both passes, renderView on
and off, 0 and 2 view buffers under autoClearView and a fade, equal and unequal line widths.  (The torch.distributed route needs
CUDA tensors: the GPU suite has it.)"""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

from test_draw_program_build import FLOW
from test_fragment_program_build import VIGNETTE, FragUniforms

FLOW_PASS, VIEW_PASS = 0, 1
CTX, OUT = "ctx", "out"
TIME, FADE = 12.5, [0.25, 0.5, 0.75, 0.125]
RENDER = dict(tint=[1.0, 2.0, 3.0, 4.0], invRes=[0.5, 0.25], edge=0.125, gain=0.5)      # Tendrils.uniforms["render"]: the fragment stage's block


class FlowUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("time", C.c_float), ("speedLimit", C.c_float)]


@pytest.fixture(scope="module")
def programs():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    from tendrils_amd.particles import DrawProgram, FragmentProgram
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    made = dict(vertex=DrawProgram.from_source(FLOW, FlowUniforms, "flow"), bare=DrawProgram.from_source(FLOW, None, "flow_bare"),
                fragment=FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette"))
    yield made
    for program in made.values():
        program.dispose()


class Recorder:
    """call(name, *args) that runs nothing: the name and a digest of the arguments - integers and floats as they are, a context
    as "ctx", a program as its kind, a float array as its values, a byref structure as (type name, bytes), any other byref
    as "out"; a th_draw_stages as what its three slots hold"""

    def __init__(self, programs):
        self.kinds = {p.handle.value: p.kind for p in programs.values()}
        self.calls = []

    def digest(self, arg, view_pass=False):
        from tendrils_amd import _capi
        if arg is None or isinstance(arg, (int, float)):
            return arg
        if isinstance(arg, C.c_void_p):
            return self.kinds[arg.value] if arg.value else CTX
        if isinstance(arg, C.Array):
            return tuple(arg)
        held = arg._obj                             # (byref)
        if isinstance(held, _capi.DrawStages):
            builtin = _capi.RenderUniforms if view_pass else _capi.DepositUniforms
            return ("DrawStages",
                    self.kinds.get(held.vertex), C.string_at(held.vertex_uniforms, held.vertex_uniform_bytes) if held.vertex_uniforms else None,
                    self.kinds.get(held.fragment), C.string_at(held.fragment_uniforms, held.fragment_uniform_bytes) if held.fragment_uniforms else None,
                    (builtin.__name__, C.string_at(held.builtin, C.sizeof(builtin))) if held.builtin else None)
        if isinstance(held, C.Structure):
            return (type(held).__name__, bytes(held))
        return OUT

    def __call__(self, name, *args):
        view_pass = name == "th_draw_stages_run" and args[2] == VIEW_PASS
        self.calls.append((name,) + tuple(self.digest(a, view_pass) for a in args))
        return 0


@pytest.fixture
def recorder(programs, monkeypatch):
    from tendrils_amd import _capi, particles, tendrils
    rec = Recorder(programs)
    for module in (_capi, tendrils, particles):
        monkeypatch.setattr(module, "call", rec)
    return rec


def drawn(recorder, band=False, buffers=0, view=True, widths=(5, 1), flow=None, render=None, prologue=False):
    """the calls of one draw() of a 16 x 16 (band: 16 x 8 of 16 rows) Tendrils on a 64 x 48 view, and the Tendrils"""
    from tendrils_amd.tendrils import Tendrils, View, defaults
    state = dict(defaults()["state"], rootNum=16, flowWidth=widths[0], lineWidth=widths[1])
    if prologue:
        state.update(autoClearView=True, autoFade=True, fadeColor=FADE)
    else:
        state.update(autoClearView=False, autoFade=False)
    options = dict(state=state, numBuffers=buffers, renderView=view, flowShader=flow, renderShader=render)
    if band:
        options.update(row0=0, rows=8, globalHeight=16)
    t = Tendrils(View(64, 48), options)
    t.setup()
    t.resize()
    t.timer.time = TIME
    t.uniforms["render"].update(RENDER)
    del recorder.calls[:]
    return t


# the structures a frame's calls carry, written out: th_deposit_uniforms (viewSize = the cover aspect of 64 x 48, time, speedLimit
# - the vertex program's block has the same four floats), th_render_uniforms (... flowDecay, speedAlpha, colorMapAlpha, sinTerm,
# baseColor, flowColor: the defaults), the fragment program's block (tint, invRes, edge, gain)
SIN_TERM = math.sin(float(np.float32(TIME)) * float(np.float32(0.005)))
VBLOCK = struct.pack("<4f", 1.0, 64 / 48, TIME, 0.01)
D = ("DepositUniforms", VBLOCK)
R = ("RenderUniforms", struct.pack("<16f", 1.0, 64 / 48, TIME, 0.01, 0.005, 0.000001, 0.4, SIN_TERM, 1, 1, 1, 0.5, 1, 1, 1, 0.04))
FBLOCK = struct.pack("<8f", 1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 0.125, 0.5)


def widths(flow, view):
    return [("th_line_width", CTX, FLOW_PASS, float(flow)), ("th_line_width", CTX, VIEW_PASS, float(view))]


FILL = ("th_view_fill", CTX, tuple(C.c_float(v).value for v in FADE))
# autoClearView + a fade with no buffers: the screen bound, cleared (clearView binds it again), filled
PROLOGUE_0 = [("th_view_bind", CTX, -1), ("th_view_bind", CTX, -1), ("th_view_clear", CTX), FILL]
# ... with two buffers: buffers[0] bound; clearView clears both and the screen - which it leaves bound -, then the fill
PROLOGUE_2 = [("th_view_bind", CTX, 0), ("th_view_bind", CTX, 0), ("th_view_clear", CTX), ("th_view_bind", CTX, 1), ("th_view_clear", CTX),
              ("th_view_bind", CTX, -1), ("th_view_clear", CTX), FILL]


# ---- the whole texture -----------------------------------------------------------------------------------------------------------
def test_local_builtin_draw_binds_then_draws_both_passes_in_one_call(recorder):
    t = drawn(recorder)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_view_bind", CTX, -1), ("th_draw", CTX, D, R, OUT)]


def test_local_builtin_draw_runs_the_prologue_before_th_draw(recorder):
    t = drawn(recorder, prologue=True, widths=(1, 1))
    t.draw()
    assert recorder.calls == widths(1, 1) + PROLOGUE_0 + [("th_draw", CTX, D, R, OUT)]
    t = drawn(recorder, prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + PROLOGUE_2 + [("th_draw", CTX, D, R, OUT)]


def test_local_builtin_draw_without_a_view_is_the_flow_pass(recorder):
    t = drawn(recorder, view=False, prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_flow_deposit", CTX, D, OUT)]


def test_local_flow_program_runs_before_the_prologue_and_the_builtin_view_pass(recorder, programs):
    t = drawn(recorder, flow=programs["vertex"], prologue=True)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_program_run", CTX, "draw", ("FlowUniforms", VBLOCK), 16, FLOW_PASS, OUT)] + PROLOGUE_0 + \
        [("th_view_draw", CTX, R, OUT)]
    t = drawn(recorder, flow=programs["vertex"], prologue=True, buffers=2, widths=(2, 2))
    t.draw()
    assert recorder.calls == widths(2, 2) + [("th_draw_program_run", CTX, "draw", ("FlowUniforms", VBLOCK), 16, FLOW_PASS, OUT)] + PROLOGUE_2 + \
        [("th_view_draw", CTX, R, OUT)]


def test_local_flow_program_without_a_block_or_a_view(recorder, programs):
    t = drawn(recorder, flow=programs["bare"], view=False, prologue=True)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_program_run", CTX, "draw", None, 0, FLOW_PASS, OUT)]


def test_local_render_fragment_program_follows_the_builtin_flow_pass_and_the_prologue(recorder, programs):
    t = drawn(recorder, render=programs["fragment"], prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_flow_deposit", CTX, D, OUT)] + PROLOGUE_2 + \
        [("th_draw_stages_run", CTX, ("DrawStages", None, None, "fragment", FBLOCK, R), VIEW_PASS, OUT)]
    t = drawn(recorder, render=programs["fragment"], view=False)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_flow_deposit", CTX, D, OUT)]


def test_local_pairs_on_both_passes(recorder, programs):
    pair = (programs["vertex"], programs["fragment"])
    t = drawn(recorder, flow=pair, render=[None, programs["fragment"]], prologue=True, widths=(1, 3))
    t.draw()
    assert recorder.calls == widths(1, 3) + [("th_draw_stages_run", CTX, ("DrawStages", "draw", VBLOCK, "fragment", FBLOCK, None), FLOW_PASS, OUT)] + \
        PROLOGUE_0 + [("th_draw_stages_run", CTX, ("DrawStages", None, None, "fragment", FBLOCK, R), VIEW_PASS, OUT)]
    t = drawn(recorder, flow=[None, programs["fragment"]], render=pair, view=False, buffers=2, prologue=True)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_stages_run", CTX, ("DrawStages", None, None, "fragment", FBLOCK, D), FLOW_PASS, OUT)]
    t = drawn(recorder, flow=pair, render=pair, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_stages_run", CTX, ("DrawStages", "draw", VBLOCK, "fragment", FBLOCK, None), FLOW_PASS, OUT),
                                             ("th_view_bind", CTX, 0),
                                             ("th_draw_stages_run", CTX, ("DrawStages", "draw", VBLOCK, "fragment", FBLOCK, None), VIEW_PASS, OUT)]


def test_the_pass_helpers_keep_their_signatures(recorder, programs):
    """tests and tools call them: _draw_program(program, which, uniforms), _draw_stages(vertex, fragment, which, uniforms)"""
    t = drawn(recorder)
    u = t.draw_program_uniforms()
    assert t._draw_program(programs["vertex"], VIEW_PASS, u) == 0
    assert t._draw_stages(None, programs["fragment"], FLOW_PASS, u) == 0
    assert recorder.calls == [("th_draw_program_run", CTX, "draw", ("FlowUniforms", VBLOCK), 16, VIEW_PASS, OUT),
                              ("th_draw_stages_run", CTX, ("DrawStages", None, None, "fragment", FBLOCK, D), FLOW_PASS, OUT)]
    with pytest.raises(TypeError):
        t._draw_program(programs["fragment"], FLOW_PASS, u)
    assert t.particles.deposit_flow(t.viewSize, t.timer.time, t.state["speedLimit"]) == 0
    assert recorder.calls[2:] == [("th_flow_deposit", CTX, D, OUT)]


# ---- a row band, the exchange issued by the library -------------------------------------------------------------------------------
def test_band_builtin_draw_runs_the_prologue_first(recorder):
    t = drawn(recorder, band=True)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_view_bind", CTX, -1), ("th_draw_sharded", CTX, D, R, OUT)]
    t = drawn(recorder, band=True, prologue=True, widths=(1, 1))
    t.draw()
    assert recorder.calls == widths(1, 1) + PROLOGUE_0 + [("th_draw_sharded", CTX, D, R, OUT)]
    t = drawn(recorder, band=True, prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + PROLOGUE_2 + [("th_draw_sharded", CTX, D, R, OUT)]


def test_band_builtin_draw_without_a_view(recorder):
    t = drawn(recorder, band=True, view=False, prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_sharded", CTX, D, None, OUT)]


def test_band_flow_program_goes_through_the_librarys_program_exchange(recorder, programs):
    t = drawn(recorder, band=True, flow=programs["vertex"], prologue=True, buffers=2)
    t.draw()
    assert recorder.calls == widths(5, 1) + PROLOGUE_2 + \
        [("th_draw_program_sharded", CTX, "draw", ("FlowUniforms", VBLOCK), 16, D, None, None, 0, R, OUT, OUT)]
    t = drawn(recorder, band=True, flow=programs["vertex"], view=False, prologue=True)
    t.draw()
    assert recorder.calls == widths(5, 1) + [("th_draw_program_sharded", CTX, "draw", ("FlowUniforms", VBLOCK), 16, D, None, None, 0, None, OUT, OUT)]
    t = drawn(recorder, band=True, flow=programs["bare"], render=programs["vertex"], widths=(3, 3))
    t.draw()
    assert recorder.calls == widths(3, 3) + [("th_view_bind", CTX, -1),
                                             ("th_draw_program_sharded", CTX, "draw", None, 0, D, "draw", ("FlowUniforms", VBLOCK), 16, R, OUT, OUT)]


def test_band_render_program_without_a_view_is_the_builtin_flow_pass(recorder, programs):
    for render in (programs["vertex"], programs["fragment"]):
        t = drawn(recorder, band=True, render=render, view=False)
        t.draw()
        assert recorder.calls == widths(5, 1) + [("th_draw_sharded", CTX, D, None, OUT)]
        assert (t.fragments, t.view_fragments) == (0, 0)


def test_band_fragment_stage_is_refused_before_anything_draws(recorder, programs):
    """the library-issued exchange carries no fragment stage: NotImplementedError names the route that does, and no call that
    draws or exchanges was made - only the widths and, with a view, the prologue, which come first on every sharded route"""
    t = drawn(recorder, band=True, render=programs["fragment"], prologue=True)
    with pytest.raises(NotImplementedError) as e:
        t.draw()
    assert "fragment stage" in str(e.value) and "th_draw_stages_emit" in str(e.value)
    assert recorder.calls == widths(5, 1) + PROLOGUE_0
    t = drawn(recorder, band=True, flow=(programs["vertex"], programs["fragment"]), render=programs["vertex"], view=False, prologue=True)
    with pytest.raises(NotImplementedError) as e:
        t.draw()
    assert "fragment stage" in str(e.value)
    assert recorder.calls == widths(5, 1)
