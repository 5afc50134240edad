"""Step programs (include/tendrils_hip.h "step programs"), the part that needs no GPU: th_step_program_compile builds a
caller's integrator for gfx950 through hiprtc on any machine, its diagnostics carry the caller's own line numbers, and the one
restriction of the kind - no th_particles - is a compile error on the caller's own line."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIFT = """struct Drift { float unused; };
__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self;
    p.x = p.x + p.z * s.dt;
    p.y = p.y + p.w * s.dt;
    return p;
}
"""

# the caller's line 3 lacks its semicolon
BROKEN = """__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self
    return p;
}
"""

NO_MAIN = """__device__ float4 not_the_entry(const th_step_pass &s)
{
    return s.self;
}
"""

# the caller's line 4 reads another texel of the ring: what a step program cannot do
NEIGHBOUR = """__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self;
    const float4 q = th_particles(s, s.x + 1, s.y);
    p.x = q.x;
    return p;
}
"""

# a state program: the other kind's entry point and pass type
STATE = """__device__ float4 th_main(const th_pass &p)
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


def compile_step(lib, source, name=b"test_step"):
    handle = C.c_void_p()
    status = lib.th_step_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def test_a_step_program_compiles_without_a_device(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, DRIFT)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value
    assert lib.th_program_log() == b""
    assert len(_capi._mapped("libhiprtc")) == 1, _capi._mapped("libhiprtc")
    assert len(_capi._mapped("libamdhip64")) == 1, _capi._mapped("libamdhip64")
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_a_source_without_th_step_main_does_not_compile(lib):
    from tendrils_amd import _capi
    for source in (NO_MAIN, STATE):
        status, handle = compile_step(lib, source)
        assert status == _capi.TH_ERR_INVALID and not handle.value
    status, handle = compile_step(lib, NO_MAIN)
    assert "th_step_main" in lib.th_program_log().decode()


def test_th_particles_does_not_exist_for_a_step_program(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, NEIGHBOUR, b"neighbour_step")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    line = [l for l in log.splitlines() if "neighbour_step:4:" in l and "error" in l]
    assert line and "th_particles" in line[0], log
    assert b"neighbour_step" in lib.th_last_error()
    # ... and the same accessor is what a state program has: the restriction is the kind's, not the compiler's
    handle = C.c_void_p()
    source = NEIGHBOUR.replace("th_step_main", "th_main").replace("th_step_pass", "th_pass")
    assert lib.th_program_compile(source.encode(), b"neighbour_state", C.byref(handle)) == _capi.TH_OK, lib.th_program_log()
    lib.th_program_destroy(handle)


def test_a_syntax_error_names_the_callers_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, BROKEN, b"broken_step")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "broken_step:3:" in log and "error" in log, log
    assert b"broken_step" in lib.th_last_error()
    status, handle = compile_step(lib, DRIFT)                # the log belongs to the last compile of the thread
    assert status == _capi.TH_OK and lib.th_program_log() == b""
    lib.th_program_destroy(handle)


def test_the_python_host_raises_with_the_compilers_output(lib):
    import tendrils_amd as ta
    with pytest.raises(ta.TendrilsHipError) as e:
        ta.StepProgram.from_source(BROKEN, name="broken_step")
    assert e.value.status == 1 and "broken_step:3:" in str(e.value)
    with pytest.raises(ta.TendrilsHipError) as e:
        ta.StepProgram.from_source(NEIGHBOUR, name="neighbour_step")
    assert "th_particles" in str(e.value)

    class TooLarge(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 1025)]
    with pytest.raises(ValueError):
        ta.StepProgram.from_source(DRIFT, TooLarge)
    prog = ta.StepProgram.from_source(DRIFT, name="drift")
    assert isinstance(prog, ta.Program) and prog.kind == "step" and prog.handle
    prog.dispose()
    assert prog.handle is None
    prog.dispose()
