"""What the no-GPU tests of the built-in passes over the ring share (tests/test_density_build.py, test_select_build.py,
test_histogram_build.py, test_follow_build.py): the library fixture, a unit's code without its comments, the assertions every one
of them makes in the same words - and the three tests that are the same for all four, written here once and imported by each
module, which names its unit in UNITS below."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tendrils_hip.h")
# test module -> its unit, and the word no program kind may hold
UNITS = dict(test_density_build=("th_density.hip", "density"), test_select_build=("th_select.hip", "select"),
             test_histogram_build=("th_histogram.hip", "hist"), test_follow_build=("th_follow.hip", "follow"))
# the device code the units share: the slot loader, the sums and the texel rank; the texel set's kernels beside the scan
SHARED = ("th_ring.hpp", "th_sort.hip")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def stripped(name):
    text = open(os.path.join(CSRC, name)).read()
    code = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"/\*.*?\*/", "", code, flags=re.S)


def kernels(code):
    return re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)


def makefile_list(name):
    return re.search(r"^%s\s*:=(.*)$" % name, open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()


def assert_exported_and_bound(lib, calls):
    """both libraries export `calls`, and the header, the libraries' symbol tables and the ctypes binding agree"""
    from tendrils_amd import _capi
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", CSRC, "release"], stdout=subprocess.DEVNULL)
    for path in (TESTING, RELEASE):
        have = exported(path)
        assert [c for c in calls if c in have] == calls, path
    assert [c for c in calls if c in header_symbols(testing=False)] == calls
    assert exported(RELEASE) == header_symbols(testing=False)
    assert sorted(_capi.PROTOTYPES) == header_symbols(testing=True)
    for c in calls:
        assert hasattr(lib, c) and _capi.PROTOTYPES[c][0] is C.c_int32


def assert_c_layout(tmp_path, asserts):
    """the header's declarations as a C compiler lays them out: every (condition, message) holds"""
    source = tmp_path / "layout.c"
    source.write_text('#include <stddef.h>\n#include "tendrils_hip.h"\n' + "".join('_Static_assert(%s, "%s");\n' % a for a in asserts))
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def assert_fixed_integer_code(code, atomics):
    """no assembly statement, no run-time compilation, no switch read from the environment; the atomics are among `atomics`, and
    nothing of a float type goes near one"""
    assert "asm" not in code.lower() and "hiprtc" not in code.lower() and "getenv" not in code
    assert set(re.findall(r"\batomic\w+", code)) <= set(atomics)
    for call_ in re.findall(r"atomic\w+\s*\(([^;]*);", code):
        assert "float" not in call_ and "double" not in call_, call_


def unit_of(request):
    assert request.module.__name__ in UNITS, "name the unit of %s in builtin_pass.UNITS" % request.module.__name__
    return UNITS[request.module.__name__]


# ---- the tests every one of the four modules imports: the same assertions, about the importing module's unit -------------------
def test_the_abi_version_is_still_14(lib):
    assert lib.th_abi_version() == 14
    assert "#define TH_ABI_VERSION 14\n" in open(HEADER).read()


def test_the_unit_is_in_core(request):
    unit, _ = unit_of(request)
    assert unit in makefile_list("CORE")       # (CORE is what both the testing and the release library link)
    assert {"th_ring.hpp", "th_select_match.hpp"} <= set(makefile_list("HDRS"))


def test_no_prelude_and_no_program_kind_came_with_it(request):
    _, word = unit_of(request)
    preludes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_prelude.inc")))
    assert preludes == ["th_draw_prelude.inc", "th_fragment_pair_prelude.inc", "th_fragment_prelude.inc", "th_measure_prelude.inc",
                        "th_program_prelude.inc", "th_screen_prelude.inc", "th_step_prelude.inc"]
    assert word not in open(os.path.join(CSRC, "th_program_kinds.hpp")).read().lower()
