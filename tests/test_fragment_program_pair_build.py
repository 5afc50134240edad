"""Both passes' fragment stages over one rasterisation (th_draw_stages_pair), the part that needs no GPU: both libraries export
the call and the binding declares it, the ABI version stays; every fragment program's module holds two more entry points,
th_fragment_pair_kernel and th_fragment_pair_bins_kernel, over records of their own - the existing record, then the half - and the
four older records keep their sizes; the new prelude file declares exactly those two kernels; the programs of the other tests
still build through hiprtc with an empty log."""
import ctypes as C
import os
import re

import pytest

from test_fragment_program_build import IDENTITY, VIGNETTE, compile_with, exported, lib  # noqa: F401  (lib: the fixture)
from test_fragment_program_line_build import FALLOFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIR_KERNELS = ("th_fragment_pair_kernel", "th_fragment_pair_bins_kernel")

# the module as a program's source sees it: the two new entry points over records of their own, the old records as they were
ENTRY_POINTS = """static_assert(__is_same(decltype(&th_fragment_pair_kernel), void (*)(const th_fragment_pair_args, const th_program_uniform_block)), "a record of its own");
static_assert(__is_same(decltype(&th_fragment_pair_bins_kernel), void (*)(const th_fragment_pair_bins_args, const th_program_uniform_block)), "a record of its own");
static_assert(sizeof(th_fragment_pair_args) == 72 && __builtin_offsetof(th_fragment_pair_args, half) == 64, "the first record in front, the half behind");
static_assert(sizeof(th_fragment_pair_bins_args) == 120 && __builtin_offsetof(th_fragment_pair_bins_args, half) == 112, "the bins' record in front, the half behind");
static_assert(__is_same(decltype(th_fragment_pair_args::f), th_fragment_args) && __is_same(decltype(th_fragment_pair_bins_args::b), th_fragment_bins_args), "the existing records");
static_assert(__is_same(decltype(th_fragment_pair_args::half), unsigned) && __is_same(decltype(th_fragment_pair_bins_args::half), unsigned), "the half");
static_assert(sizeof(th_fragment_args) == 64 && sizeof(th_fragment_line_args) == 72 && sizeof(th_fragment_bins_args) == 112 && sizeof(th_fragment_line_bins_args) == 120, "the other records keep their sizes");
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    return f.color;
}
"""


def test_both_libraries_export_the_call_and_the_binding_declares_it(lib):  # noqa: F811
    from tendrils_amd import _capi
    release = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
    for path in (_capi.LIB_PATH, release):
        assert "th_draw_stages_pair" in exported(path), "%s does not export th_draw_stages_pair" % path
    assert "th_draw_stages_pair" in _capi.PROTOTYPES and hasattr(lib, "th_draw_stages_pair")
    restype, argtypes = _capi.PROTOTYPES["th_draw_stages_pair"]
    assert restype is C.c_int32 and len(argtypes) == 5
    assert argtypes[1] is argtypes[2] and argtypes[1]._type_ is _capi.DrawStages
    assert argtypes[3]._type_ is C.c_uint64 and argtypes[4]._type_ is C.c_int32
    assert lib.th_abi_version() == 14
    header = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    assert re.search(r"th_status\s+th_draw_stages_pair\(th_context \*ctx, const th_draw_stages \*flow, const th_draw_stages \*view,\s*"
                     r"uint64_t \*fragments, int32_t \*rasterisations\);", header)


def test_the_module_declares_the_two_pair_entry_points(lib):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", ENTRY_POINTS, b"pair_entry_points")
    assert status == _capi.TH_OK, lib.th_program_log()
    assert lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_the_new_prelude_file_declares_exactly_the_two_kernels():
    prelude = open(os.path.join(ROOT, "tendrils_amd", "csrc", "th_fragment_pair_prelude.inc")).read()
    declared = re.findall(r'extern "C" __global__ __launch_bounds__\(256\) void (\w+)\(', prelude)
    assert sorted(declared) == sorted(PAIR_KERNELS), declared
    assert len(re.findall(r"__global__", prelude)) == 2
    assert "sizeof(th_fragment_pair_args) == 72" in prelude and "sizeof(th_fragment_pair_bins_args) == 120" in prelude
    for word in ("__shared__", "atomic", "asm"):              # no LDS, no atomics, no inline assembly in the kernels' text
        code = "\n".join(line.split("//")[0] for line in prelude.splitlines())
        assert word not in code, word


@pytest.mark.parametrize("source", [IDENTITY, VIGNETTE, FALLOFF], ids=["identity", "vignette", "falloff"])
def test_the_programs_compile_with_no_device(lib, source):  # noqa: F811
    from tendrils_amd import _capi
    assert hasattr(lib, "th_draw_stages_pair")             # (the library whose modules hold the two pair kernels)
    status, handle = compile_with(lib, "th_fragment_program_compile", source)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK
