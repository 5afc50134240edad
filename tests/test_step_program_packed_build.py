"""Step programs on the packed ring (th_step_prelude.inc: th_step_packed_kernel), the part that needs no GPU: a step program
compiles for gfx950 without a device against a prelude that carries a second entry point with the first one's signature - the
launch record is still the 232 bytes both static_asserts pin -; the drift program still compiles to an empty log; and the
kind's one restriction is still an error on the caller's own line, behind the codec text now in front of the prelude."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIFT = """__device__ float4 th_step_main(const th_step_pass &s)
{
    float4 p = s.self;
    p.x = p.x + p.z * s.dt;
    p.y = p.y + p.w * s.dt;
    return p;
}
"""

# the packed entry as a program's source sees it: declared, with th_step_kernel's signature, over the same record
PACKED_ENTRY = """static_assert(__is_same(decltype(&th_step_packed_kernel), decltype(&th_step_kernel)), "one signature, two entry points");
static_assert(sizeof(th_step_args) == 232, "the record a step program is launched with");
__device__ float4 th_step_main(const th_step_pass &s)
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


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_step(lib, source, name=b"test_step_packed"):
    handle = C.c_void_p()
    status = lib.th_step_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def test_a_source_that_names_the_packed_entry_compiles_without_a_device(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, PACKED_ENTRY)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK
    assert lib.th_abi_version() == 14                        # no entry point was added for it


def test_the_drift_program_still_compiles_to_an_empty_log(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, DRIFT)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_th_particles_still_fails_on_the_callers_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, NEIGHBOUR, b"neighbour_packed")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    line = [l for l in log.splitlines() if "neighbour_packed:4:" in l and "error" in l]
    assert line and "th_particles" in line[0], log
