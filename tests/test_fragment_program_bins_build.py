"""Fragment programs through the bins (TH_OPT_STAGE_BINS), the part that needs no GPU: the prelude with its third entry point,
th_fragment_bins_kernel, still builds the tests' programs through hiprtc on any machine; the Python host knows the option by the
number the header gives it; the ABI version is what it was - the switch adds no entry point."""
import ctypes as C
import os
import re

import pytest

from test_fragment_program_build import IDENTITY, VIGNETTE, compile_with, lib  # noqa: F401  (lib: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("source", [IDENTITY, VIGNETTE], ids=["identity", "vignette"])
def test_the_programs_still_compile_with_no_device(lib, source):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", source)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_the_option_has_the_headers_number_and_the_abi_is_unchanged(lib):  # noqa: F811
    from tendrils_amd.particles import Particles
    assert Particles.OPTIONS["stage_bins"] == 16
    header = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    assert re.search(r"\bTH_OPT_STAGE_BINS\s*=\s*16\b", header)
    assert sorted(Particles.OPTIONS.values()) == list(range(17))      # every number once
    assert lib.th_abi_version() == 14


def test_the_prelude_holds_the_three_entry_points(lib):  # noqa: F811
    """the text hiprtc receives defines the bins kernel beside the two it had; its record restates the bins' constants"""
    prelude = open(os.path.join(ROOT, "tendrils_amd", "csrc", "th_fragment_prelude.inc")).read()
    for kernel in ("th_fragment_kernel", "th_fragment_band_kernel", "th_fragment_bins_kernel"):
        assert re.search(r'extern "C" __global__ __launch_bounds__\(256\) void %s\(' % kernel, prelude), kernel
    assert "sizeof(th_fragment_args) == 64" in prelude and "sizeof(th_fragment_bins_args) == 112" in prelude
