"""Draw programs (include/tendrils_hip.h "draw programs"), the part that needs no GPU: th_draw_program_compile builds a caller's
vertex stage for gfx950 through hiprtc on any machine, behind a prelude of its own - the three compile entry points do not take
each other's sources - and nothing about it brings a second HIP runtime into the process."""
import ctypes as C
import os

import pytest

from test_program_build import DRIFT
from test_screen_program_build import COPY, ONLY_TH_MAIN, ONLY_TH_SCREEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the library's own flow stage, written out as a program (tendrils_amd/csrc/th_raster.hpp: dep_fetch, dep_vertex_colors)
FLOW = """struct FlowUniforms { float viewSize[2]; float time; float speedLimit; };
__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    const FlowUniforms &u = th_uniforms<FlowUniforms>(v);
    const float4 s = v.state;
    if (!(s.x != -1000000.0f || s.y != -1000000.0f)) return th_discard_vertex();
    th_vertex o;
    o.position = make_float2(s.x * u.viewSize[0], s.y * u.viewSize[1]);
    o.color = make_float4(s.z, s.w, u.time, __builtin_fminf(__builtin_sqrtf(s.z * s.z + s.w * s.w) / u.speedLimit, 1.0f));
    return o;
}
"""

# the user's line 3 lacks its semicolon
BROKEN = """__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    th_vertex o = th_discard_vertex()
    return o;
}
"""

# this kind's entry point and nothing else (no type of any prelude: what fails elsewhere is the missing entry point, not the text)
ONLY_TH_VERTEX_MAIN = ONLY_TH_MAIN.replace("th_main", "th_vertex_main")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_with(lib, entry, source, name=b"test_draw"):
    handle = C.c_void_p()
    status = getattr(lib, entry)(source.encode(), name, C.byref(handle))
    return status, handle


def test_compile_needs_no_gpu_and_no_second_runtime(lib):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_draw_program_compile", FLOW)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value
    assert lib.th_program_log() == b""
    assert len(_capi._mapped("libhiprtc")) == 1, _capi._mapped("libhiprtc")
    assert len(_capi._mapped("libamdhip64")) == 1, _capi._mapped("libamdhip64")
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_a_syntax_error_names_the_users_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_draw_program_compile", BROKEN, b"broken_draw")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "broken_draw:3:" in log and "error" in log, log
    assert b"broken_draw" in lib.th_last_error()


@pytest.mark.parametrize("source", [ONLY_TH_MAIN, ONLY_TH_SCREEN], ids=["th_main", "th_screen"])
def test_another_kinds_source_is_no_draw_program(lib, source):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_draw_program_compile", source)
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_vertex_main" in lib.th_program_log().decode()


def test_the_other_compile_entry_points_keep_their_own_preludes(lib):
    from tendrils_amd import _capi
    for entry, good, wants in (("th_program_compile", DRIFT, "th_main"), ("th_screen_program_compile", COPY, "th_screen")):
        status, handle = compile_with(lib, entry, good)
        assert status == _capi.TH_OK and lib.th_program_log() == b"", lib.th_program_log()
        lib.th_program_destroy(handle)
        status, handle = compile_with(lib, entry, ONLY_TH_VERTEX_MAIN)
        assert status == _capi.TH_ERR_INVALID and not handle.value
        assert wants in lib.th_program_log().decode()


def test_the_python_host_raises_with_the_compilers_output(lib):
    import tendrils_amd as ta
    from tendrils_amd.particles import DrawProgram
    with pytest.raises(ta.TendrilsHipError) as e:
        DrawProgram.from_source(BROKEN, name="broken_draw")
    assert e.value.status == 1 and "broken_draw:3:" in str(e.value)

    class TooLarge(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 1025)]
    with pytest.raises(ValueError):
        DrawProgram.from_source(FLOW, TooLarge)
    prog = ta.DrawProgram.from_source(FLOW, name="flow")
    assert prog.kind == "draw" and prog.handle
    prog.dispose()
    assert prog.handle is None
    prog.dispose()


def test_running_without_a_gpu_is_a_loud_error(lib):
    """as tests/test_program_build.py: no fall-back of any kind"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import tendrils_amd as ta
    from tendrils_amd import _capi
    from tendrils_amd.particles import DrawProgram
    prog = DrawProgram.from_source(FLOW, name="flow")
    with pytest.raises(ta.TendrilsHipError):          # no context can exist: the entry point says so, it does not compute
        _capi.call("th_draw_program_run", None, prog.handle, None, 0, _capi.TH_PASS_FLOW, None)
    prog.dispose()
