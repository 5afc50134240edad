"""Measure programs (include/tendrils_hip.h "measure programs"), the part that needs no GPU: both libraries export the four
entry points, th_measure_program_compile builds a caller's sample function for gfx950 through hiprtc on any machine for 1 .. 8
channels, its diagnostics carry the caller's own line numbers, th_particles does not exist for this kind, and the prelude holds
the two kernels it says it holds - without an atomic or an assembly statement anywhere in its code."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["th_measure_async", "th_measure_global", "th_measure_program_compile", "th_measure_run"]

LIVE = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    s.v[0] = (m.self.x != -1000000.0f || m.self.y != -1000000.0f) ? 1.0f : 0.0f;
    return s;
}
"""

# what the two sides share, as the caller's compiler sees it
LAYOUT = """static_assert(sizeof(th_measure_args) == 64, "record");
static_assert(sizeof(th_program_uniform_block) == 1024 && alignof(th_program_uniform_block) == 16, "block");
static_assert(sizeof(th_measure_partial) == 144, "partial");
static_assert(__builtin_offsetof(th_measure_partial, taken) == 0 && __builtin_offsetof(th_measure_partial, particles) == 8, "counts");
static_assert(__builtin_offsetof(th_measure_partial, sum) == 16 && __builtin_offsetof(th_measure_partial, min) == 80, "sums, minima");
static_assert(__builtin_offsetof(th_measure_partial, max) == 112, "maxima");
static_assert(sizeof(th_sample) == 4 * TH_MEASURE_CHANNELS + 4, "sample");
static_assert(TH_MEASURE_CHANNELS == 3, "channels");
__device__ th_sample th_measure_main(const th_measure_pass &m) { return th_no_sample(); }
"""

# the caller's line 4 reads another texel of the ring: what a measure program cannot do
NEIGHBOUR = """__device__ th_sample th_measure_main(const th_measure_pass &m)
{
    th_sample s = th_sample_zero();
    const float4 q = th_particles(m, m.x + 1, m.y);
    s.v[0] = q.x;
    return s;
}
"""


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_measure(lib, source, channels=1, name=b"test_measure"):
    handle = C.c_void_p()
    status = lib.th_measure_program_compile(source.encode(), name, channels, C.byref(handle))
    return status, handle


def test_both_libraries_export_the_calls_and_the_binding_declares_them(lib):
    from tendrils_amd import _capi
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", CSRC, "release"], stdout=subprocess.DEVNULL)
    for path in (TESTING, RELEASE):
        have = exported(path)
        assert [c for c in CALLS if c in have] == CALLS, path
    assert [c for c in CALLS if c in _capi.PROTOTYPES] == CALLS
    assert [c for c in CALLS if c in header_symbols(testing=False)] == CALLS
    assert lib.th_abi_version() == 14
    text = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    assert "#define TH_ABI_VERSION 14\n" in text
    for c in CALLS:
        assert hasattr(lib, c)


def test_the_result_type_is_144_bytes_on_both_sides(lib):
    from tendrils_amd import _capi
    R = _capi.MeasureResult
    assert C.sizeof(R) == 144
    assert (R.taken.offset, R.particles.offset, R.sum.offset, R.min.offset, R.max.offset) == (0, 8, 16, 80, 112)
    text = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    decl = re.search(r"typedef struct th_measure_result \{(.*?)\} th_measure_result;", text, flags=re.S)
    assert decl and re.sub(r"\s+", " ", decl.group(1)).strip() == "uint64_t taken, particles; double sum[8]; float min[8], max[8];"


def test_the_layouts_the_two_sides_share_compile_with_an_empty_log(lib):
    from tendrils_amd import _capi
    status, handle = compile_measure(lib, LAYOUT, 3, b"layout")
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


@pytest.mark.parametrize("channels", [1, 8])
def test_a_measure_program_compiles_without_a_device(lib, channels):
    from tendrils_amd import _capi
    status, handle = compile_measure(lib, LIVE, channels)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert len(_capi._mapped("libhiprtc")) == 1, _capi._mapped("libhiprtc")
    assert lib.th_program_destroy(handle) == _capi.TH_OK


@pytest.mark.parametrize("channels", [0, 9, -1])
def test_channels_outside_1_to_8_are_refused(lib, channels):
    from tendrils_amd import _capi
    status, handle = compile_measure(lib, LIVE, channels)
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert b"channels" in lib.th_last_error() and str(channels).encode() in lib.th_last_error()


def test_th_particles_does_not_exist_for_a_measure_program(lib):
    from tendrils_amd import _capi
    status, handle = compile_measure(lib, NEIGHBOUR, 1, b"neighbour_measure")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    line = [l for l in log.splitlines() if "neighbour_measure:4:" in l and "error" in l]
    assert line and "th_particles" in line[0], log
    assert b"neighbour_measure" in lib.th_last_error()


def test_the_prelude_holds_two_kernels_and_neither_atomics_nor_assembly():
    text = open(os.path.join(CSRC, "th_measure_prelude.inc")).read()
    code = re.sub(r"//[^\n]*", "", text)
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    kernels = re.findall(r'extern\s+"C"\s+__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', code)
    assert sorted(kernels) == ["th_measure_kernel", "th_measure_packed_kernel"]
    assert code.count("__global__") == 2
    assert "atomic" not in code.lower() and "asm" not in code.lower()
    assert '#include "' not in code and "#include <" not in code          # no project header, nothing beyond hiprtc's own
    # ... and the fold, which does not depend on the caller's source, is the library's own kernel in the unit beside it
    unit = open(os.path.join(CSRC, "th_measure.hip")).read()
    unit_code = re.sub(r"//[^\n]*", "", unit)
    assert re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", unit_code) == ["measure_fold_kernel"]
    assert "atomic" not in unit_code.lower() and "asm" not in unit_code.lower()


def test_the_python_host_compiles_and_refuses(lib):
    import tendrils_amd as ta
    prog = ta.MeasureProgram.from_source(LIVE, channels=2, name="live")
    assert isinstance(prog, ta.Program) and prog.kind == "measure" and prog.handle and prog.channels == 2
    prog.dispose()
    assert prog.handle is None
    with pytest.raises(ta.TendrilsHipError) as e:
        ta.MeasureProgram.from_source(NEIGHBOUR, name="neighbour_measure")
    assert "th_particles" in str(e.value) and "neighbour_measure:4:" in str(e.value)
    with pytest.raises(ta.TendrilsHipError):
        ta.MeasureProgram.from_source(LIVE, channels=9)

    class TooLarge(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 1025)]
    with pytest.raises(ValueError):
        ta.MeasureProgram.from_source(LIVE, TooLarge)
