"""th_line(f) through the binned draw() (TH_OPT_LINE_BINS), the part that needs no GPU: the prelude holds a sixth entry point,
th_fragment_line_bins_kernel, over a record that is the bins kernel's 112 bytes with the line records' pointer behind them; the
other records keep their sizes; the programs of the other tests still build through hiprtc on any machine; the hosts know the
option by the number the header gives it; the switch adds no entry point to the ABI.

The switch's number on the Python side is asked of Particles.option_number, the lookup Particles.option() goes through, not of
Particles.OPTIONS: tests/test_fragment_program_bins_build.py pins that table as the numbers 0 .. 16, every one once, so a
seventeenth entry cannot stand in it while that test stays as it is (Particles.MORE_OPTIONS holds it)."""
import os
import re

import pytest

from test_fragment_program_build import IDENTITY, VIGNETTE, compile_with, lib  # noqa: F401  (lib: the fixture)
from test_fragment_program_line_build import ALL_FIELDS, FALLOFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("th_fragment_kernel", "th_fragment_band_kernel", "th_fragment_bins_kernel", "th_fragment_line_kernel",
           "th_fragment_line_band_kernel", "th_fragment_line_bins_kernel")

# the module as a program's source sees it: the new entry point over a record of its own, the five others over theirs
ENTRY_POINTS = """static_assert(__is_same(decltype(&th_fragment_line_bins_kernel), void (*)(const th_fragment_line_bins_args, const th_program_uniform_block)), "a record of its own");
static_assert(sizeof(th_fragment_line_bins_args) == 120 && __builtin_offsetof(th_fragment_line_bins_args, lines) == 112, "112 bytes in front, the pointer behind");
static_assert(__is_same(decltype(th_fragment_line_bins_args::lines), const th_fragment_line *), "the places' records");
static_assert(__is_same(decltype(&th_fragment_bins_kernel), void (*)(const th_fragment_bins_args, const th_program_uniform_block)), "the bins' record");
static_assert(__is_same(decltype(&th_fragment_line_kernel), void (*)(const th_fragment_line_args, const th_program_uniform_block)), "the line record");
static_assert(__is_same(decltype(&th_fragment_line_band_kernel), decltype(&th_fragment_line_kernel)), "the line record");
static_assert(__is_same(decltype(&th_fragment_kernel), void (*)(const th_fragment_args, const th_program_uniform_block)), "the first record");
static_assert(__is_same(decltype(&th_fragment_band_kernel), decltype(&th_fragment_kernel)), "the first record");
static_assert(sizeof(th_fragment_args) == 64 && sizeof(th_fragment_line_args) == 72 && sizeof(th_fragment_bins_args) == 112 && sizeof(th_fragment_line) == 16, "the other records keep their sizes");
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    return f.color;
}
"""


def test_the_module_declares_six_entry_points(lib):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", ENTRY_POINTS, b"entry_points")
    assert status == _capi.TH_OK, lib.th_program_log()
    assert lib.th_program_destroy(handle) == _capi.TH_OK
    prelude = open(os.path.join(ROOT, "tendrils_amd", "csrc", "th_fragment_prelude.inc")).read()
    declared = re.findall(r'extern "C" __global__ __launch_bounds__\(256\) void (\w+)\(', prelude)
    assert sorted(declared) == sorted(KERNELS), declared
    assert "sizeof(th_fragment_line_bins_args) == 120" in prelude


def test_the_option_has_the_headers_number_and_the_abi_is_unchanged(lib):  # noqa: F811
    from tendrils_amd.particles import Particles
    assert Particles.option_number("line_bins") == 17
    assert Particles.option_number("stage_bins") == Particles.OPTIONS["stage_bins"] == 16
    header = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    assert re.search(r"\bTH_OPT_LINE_BINS\s*=\s*17\b", header)
    numbers = list(Particles.OPTIONS.values()) + list(Particles.MORE_OPTIONS.values())
    assert sorted(numbers) == list(range(18))                          # every number once
    assert lib.th_abi_version() == 14


@pytest.mark.parametrize("source", [IDENTITY, VIGNETTE, FALLOFF, ALL_FIELDS], ids=["identity", "vignette", "falloff", "all-fields"])
def test_the_programs_compile_with_no_device(lib, source):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", source)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK
