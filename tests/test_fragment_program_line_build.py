"""The fragment's line (th_line(f), include/tendrils_hip.h "fragment programs"), the part that needs no GPU: a fragment program
that reads th_line builds for gfx950 through hiprtc on any machine, the module holds the two entry points that take the line
records beside the three it had, the programs of the other tests build as before, and the other kinds' programs have no such
accessor: a source of theirs that names it fails on the caller's own line."""
import os
import re

import pytest

from test_draw_program_build import FLOW
from test_fragment_program_build import IDENTITY, VIGNETTE, compile_with, lib  # noqa: F401  (lib: the fixture)
from test_screen_program_build import COPY
from test_step_program_build import DRIFT as STEP_DRIFT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's @todo ("SDF from line, to weaken force further away", src/flow/index.frag) as a program: alpha falls off with
# the fragment's distance from its line
FALLOFF = """struct Falloff { float halfWidth; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    float4 o = f.color;
    o.w = o.w * fmaxf(1.0f - fabsf(th_line(f).across) / th_uniforms<Falloff>(f).halfWidth, 0.0f);
    return o;
}
"""

# every field, each through its own type
ALL_FIELDS = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const th_fragment_line &l = th_line(f);
    static_assert(__is_same(decltype(l.line), unsigned) && __is_same(decltype(l.along), float), "index and parameter");
    return make_float4(l.along, l.across, l.length, (float)l.line);
}
"""

# the module as a program's source sees it: the two line entry points declared with one signature over a record that is the
# existing 64-byte record with the records' pointer behind it; the three other entry points over their own records
ENTRY_POINTS = """static_assert(__is_same(decltype(&th_fragment_line_kernel), decltype(&th_fragment_line_band_kernel)), "one signature, two entry points");
static_assert(__is_same(decltype(&th_fragment_line_kernel), void (*)(const th_fragment_line_args, const th_program_uniform_block)), "a record of their own");
static_assert(__is_same(decltype(&th_fragment_kernel), void (*)(const th_fragment_args, const th_program_uniform_block)), "the existing record");
static_assert(__is_same(decltype(&th_fragment_band_kernel), decltype(&th_fragment_kernel)), "the existing record");
static_assert(sizeof(th_fragment_args) == 64 && sizeof(th_fragment_line_args) == 72 && __builtin_offsetof(th_fragment_line_args, lines) == 64, "64 bytes in front, the pointer behind");
static_assert(sizeof(th_fragment_line) == 16 && sizeof(th_fragment_bins_args) == 112, "one record a fragment");
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    return f.color;
}
"""


@pytest.mark.parametrize("source", [FALLOFF, ALL_FIELDS], ids=["falloff", "all-fields"])
def test_a_program_that_reads_the_line_compiles_with_no_device(lib, source):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", source, b"reads_line")
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_the_module_holds_the_two_line_entry_points(lib):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", ENTRY_POINTS, b"entry_points")
    assert status == _capi.TH_OK, lib.th_program_log()
    assert lib.th_program_destroy(handle) == _capi.TH_OK
    prelude = open(os.path.join(ROOT, "tendrils_amd", "csrc", "th_fragment_prelude.inc")).read()
    for kernel in ("th_fragment_kernel", "th_fragment_band_kernel", "th_fragment_bins_kernel", "th_fragment_line_kernel", "th_fragment_line_band_kernel"):
        assert re.search(r'extern "C" __global__ __launch_bounds__\(256\) void %s\(' % kernel, prelude), kernel
    assert lib.th_abi_version() == 14


@pytest.mark.parametrize("source", [IDENTITY, VIGNETTE], ids=["identity", "vignette"])
def test_the_programs_without_it_still_compile(lib, source):  # noqa: F811
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", source)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert lib.th_program_destroy(handle) == _capi.TH_OK


@pytest.mark.parametrize("entry,good,at", [("th_draw_program_compile", FLOW, "const FlowUniforms &u"),
                                           ("th_step_program_compile", STEP_DRIFT, "float4 p = s.self;"),
                                           ("th_screen_program_compile", COPY, "return th_tex")], ids=["draw", "step", "screen"])
def test_the_other_kinds_have_no_such_accessor(lib, entry, good, at):  # noqa: F811
    """a working program of the kind with one more line in its body, which names th_line: the error is on that line"""
    from tendrils_amd import _capi
    assert at in good
    lines = good.split("\n")
    where = next(k for k, text in enumerate(lines) if at in text)
    bad = "\n".join(lines[:where] + ["    const float away = th_line(%s).across;" % ("v" if "draw" in entry else "s")] + lines[where:])
    status, handle = compile_with(lib, entry, good, b"plain")
    assert status == _capi.TH_OK, lib.th_program_log()
    assert lib.th_program_destroy(handle) == _capi.TH_OK
    status, handle = compile_with(lib, entry, bad, b"names_line")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "names_line:%d:" % (where + 1) in log and "th_line" in log and "error" in log, log
