"""User programs (include/tendrils_hip.h "user programs"), the part that needs no GPU: th_program_compile builds a caller's
pass for gfx950 through hiprtc on any machine, its diagnostics carry the caller's own line numbers, and nothing about it
brings a second HIP runtime into the process."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIFT = """struct Drift { float k; };
__device__ float4 th_main(const th_pass &p)
{
    const Drift &u = th_uniforms<Drift>(p);
    float4 s = p.self;
    s.x = s.x + s.z * u.k;
    s.y = s.y + s.w * u.k;
    return s;
}
"""

# the user's line 3 lacks its semicolon
BROKEN = """__device__ float4 th_main(const th_pass &p)
{
    float4 s = p.self
    return s;
}
"""

NO_MAIN = """__device__ float4 not_the_entry(const th_pass &p)
{
    return p.self;
}
"""


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_program(lib, source, name=b"test_program"):
    handle = C.c_void_p()
    status = lib.th_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def test_compile_needs_no_gpu_and_no_second_runtime(lib):
    from tendrils_amd import _capi
    status, handle = compile_program(lib, DRIFT)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value
    assert lib.th_program_log() == b""
    # hiprtc came in at run time (the copy the process holds, else by soname): still ONE HIP runtime in the process
    assert len(_capi._mapped("libhiprtc")) == 1, _capi._mapped("libhiprtc")
    assert len(_capi._mapped("libamdhip64")) == 1, _capi._mapped("libamdhip64")
    assert lib.th_program_destroy(handle) == _capi.TH_OK
    assert lib.th_program_destroy(None) == _capi.TH_OK


def test_a_syntax_error_names_the_users_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_program(lib, BROKEN, b"broken_pass")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "broken_pass:3:" in log and "error" in log, log
    assert b"broken_pass" in lib.th_last_error()
    # the log belongs to the last compile of the thread: a good one empties it
    status, handle = compile_program(lib, DRIFT)
    assert status == _capi.TH_OK and lib.th_program_log() == b""
    lib.th_program_destroy(handle)


def test_a_source_without_th_main_does_not_compile(lib):
    from tendrils_amd import _capi
    status, handle = compile_program(lib, NO_MAIN)
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_main" in lib.th_program_log().decode()


def test_the_python_host_raises_with_the_compilers_output(lib):
    import tendrils_amd as ta
    from tendrils_amd.particles import Program
    with pytest.raises(ta.TendrilsHipError) as e:
        Program.from_source(BROKEN, name="broken_pass")
    assert e.value.status == 1 and "broken_pass:3:" in str(e.value)

    class TooLarge(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 1025)]
    with pytest.raises(ValueError):
        Program.from_source(DRIFT, TooLarge)
    prog = Program.from_source(DRIFT, name="drift")
    assert prog.kind == "user" and prog.handle
    prog.dispose()
    assert prog.handle is None
    prog.dispose()


def test_running_without_a_gpu_is_a_loud_error(lib):
    """as tests/test_capi_exports.py::test_no_gpu_is_a_loud_error: no fall-back of any kind"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import tendrils_amd as ta
    from tendrils_amd import _capi
    from tendrils_amd.particles import Program
    from tendrils_amd.tendrils import View

    class Drift(C.Structure):
        _fields_ = [("k", C.c_float)]
    prog = Program.from_source(DRIFT, Drift, name="drift")
    t = ta.Tendrils(View(8, 8), dict(logicShader=prog))
    t.resize()
    with pytest.raises(ta.TendrilsHipError):
        t.setup(8)
    block = Drift(k=1.0)
    with pytest.raises(ta.TendrilsHipError):          # no context can exist: the entry point says so, it does not compute
        _capi.call("th_program_run", None, prog.handle, C.byref(block), C.sizeof(block), _capi.TH_SOURCE_NONE, _capi.TH_TARGET_RING)
    prog.dispose()
