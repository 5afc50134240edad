"""Screen programs (include/tendrils_hip.h "screen programs"), the part that needs no GPU: th_screen_program_compile builds a
caller's full-screen pass for gfx950 through hiprtc on any machine, behind a prelude of its own - the two entry points do not
take each other's programs - and nothing about it brings a second HIP runtime into the process."""
import ctypes as C
import os

import pytest

from test_program_build import DRIFT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COPY = """__device__ float4 th_screen(const th_screen_pass &s)
{
    return th_tex(s, 0, s.uv.x, s.uv.y);
}
"""

# the user's line 3 lacks its semicolon
BROKEN = """__device__ float4 th_screen(const th_screen_pass &s)
{
    float4 c = th_texel(s, 0, s.x, s.y)
    return c;
}
"""

# the other kind's entry point and nothing else (no type of either prelude: what fails is the missing entry point, not the text)
ONLY_TH_MAIN = """__device__ float4 th_main(float4 v)
{
    return v;
}
"""
ONLY_TH_SCREEN = ONLY_TH_MAIN.replace("th_main", "th_screen")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_screen(lib, source, name=b"test_screen"):
    handle = C.c_void_p()
    status = lib.th_screen_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def compile_state(lib, source, name=b"test_program"):
    handle = C.c_void_p()
    status = lib.th_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def test_compile_needs_no_gpu_and_no_second_runtime(lib):
    from tendrils_amd import _capi
    status, handle = compile_screen(lib, COPY)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value
    assert lib.th_program_log() == b""
    assert len(_capi._mapped("libhiprtc")) == 1, _capi._mapped("libhiprtc")
    assert len(_capi._mapped("libamdhip64")) == 1, _capi._mapped("libamdhip64")
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_a_syntax_error_names_the_users_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_screen(lib, BROKEN, b"broken_screen")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "broken_screen:3:" in log and "error" in log, log
    assert b"broken_screen" in lib.th_last_error()


def test_a_state_program_is_no_screen_program(lib):
    from tendrils_amd import _capi
    status, handle = compile_screen(lib, ONLY_TH_MAIN)
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_screen" in lib.th_program_log().decode()


def test_th_program_compile_keeps_its_own_prelude(lib):
    from tendrils_amd import _capi
    status, handle = compile_state(lib, DRIFT)
    assert status == _capi.TH_OK and lib.th_program_log() == b"", lib.th_program_log()
    lib.th_program_destroy(handle)
    status, handle = compile_state(lib, ONLY_TH_SCREEN)
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_main" in lib.th_program_log().decode()


def test_the_python_host_raises_with_the_compilers_output(lib):
    import tendrils_amd as ta
    from tendrils_amd.particles import ScreenProgram
    with pytest.raises(ta.TendrilsHipError) as e:
        ScreenProgram.from_source(BROKEN, name="broken_screen")
    assert e.value.status == 1 and "broken_screen:3:" in str(e.value)

    class TooLarge(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 1025)]
    with pytest.raises(ValueError):
        ScreenProgram.from_source(COPY, TooLarge)
    prog = ScreenProgram.from_source(COPY, name="copy")
    assert prog.kind == "screen" and prog.handle
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
    from tendrils_amd.particles import ScreenProgram
    prog = ScreenProgram.from_source(COPY, name="copy")
    with pytest.raises(ta.TendrilsHipError):          # no context can exist: the entry point says so, it does not compute
        _capi.call("th_screen_run", None, prog.handle, None, 0, None, 0, _capi.SCREEN_TARGET_VIEW, 0, 1)
    prog.dispose()
