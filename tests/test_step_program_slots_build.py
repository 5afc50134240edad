"""Step programs over tile-sorted slots (include/tendrils_hip.h: th_step_program_view_size; th_step_prelude.inc: th_step_args::perm),
the part that needs no GPU: the library exports the new entry and the Python binding declares it; a step program still compiles
for gfx950 against the grown launch record without a device - the prelude's own static_assert on the record holds, and the
library's (th_stepprog.hip) held when it was built -; and the kind's one restriction is still an error on the caller's own line."""
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

# the launch record as a program sees it: the slot order's permutation is part of it, the record is 232 bytes
RECORD = """static_assert(sizeof(th_step_args) == 232, "the record a step program is launched with");
static_assert(sizeof(((th_step_args *)0)->perm) == sizeof(const unsigned *), "perm: slot -> texel");
__device__ float4 th_step_main(const th_step_pass &s)
{
    return make_float4((float)s.x, (float)s.y, (float)s.index, s.args->perm ? 1.0f : 0.0f);
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


def compile_step(lib, source, name=b"test_step"):
    handle = C.c_void_p()
    status = lib.th_step_program_compile(source.encode(), name, C.byref(handle))
    return status, handle


def test_the_library_exports_the_key_and_the_binding_declares_it(lib):
    from tendrils_amd import _capi
    assert "th_step_program_view_size" in _capi.PROTOTYPES
    fn = lib.th_step_program_view_size                       # (AttributeError: not exported)
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 2
    # no context: refused like every entry point, nothing dereferenced
    assert fn(None, None) == _capi.TH_ERR_INVALID and b"null context" in lib.th_last_error()
    with open(os.path.join(ROOT, "include", "tendrils_hip.h")) as f:
        assert "th_status th_step_program_view_size(th_context *ctx, const float viewSize[2]);" in f.read()
    assert lib.th_abi_version() == 14


def test_a_step_program_compiles_against_the_grown_record_without_a_device(lib):
    from tendrils_amd import _capi
    for source in (DRIFT, RECORD):
        status, handle = compile_step(lib, source)
        assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
        assert handle.value and lib.th_program_log() == b""
        assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_th_particles_still_fails_on_the_callers_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_step(lib, NEIGHBOUR, b"neighbour_slots")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    line = [l for l in log.splitlines() if "neighbour_slots:4:" in l and "error" in l]
    assert line and "th_particles" in line[0], log
