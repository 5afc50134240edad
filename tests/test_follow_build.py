"""Follow (include/tendrils_hip.h "follow"; tendrils_amd/csrc/th_follow.hip), the part that needs no GPU: both libraries export
th_follow_set, th_follow_sample, th_follow_read and th_follow_query, the header, the libraries' symbol tables and the ctypes
binding agree, the ABI version stays 14, th_follow_info has the size and offsets the header states on both sides, the limits their
values, the unit is linked into both libraries, holds no assembly statement, no run-time compilation and no switch read from the
environment, its only atomic is the integer OR of the mark kernel - and the pass is a built-in one: no prelude and no program
kind came with it."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["th_follow_query", "th_follow_read", "th_follow_sample", "th_follow_set"]
INFO_OFFSETS = dict(particles=0, followed=8, depth=16, samples=24, held=32, locates=40)
CONSTANTS = dict(TH_FOLLOW_MAX_PARTICLES=1 << 20, TH_FOLLOW_MAX_DEPTH=1 << 16, TH_FOLLOW_MAX_ENTRIES=1 << 24)
KERNELS = {"follow_clear_kernel", "follow_mark_kernel", "follow_count_kernel", "follow_fill_kernel", "follow_locate_kernel", "follow_gather_kernel"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def stripped(name="th_follow.hip"):
    text = open(os.path.join(CSRC, name)).read()
    code = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"/\*.*?\*/", "", code, flags=re.S)


def test_both_libraries_export_the_calls_and_header_nm_and_binding_agree(lib):
    from tendrils_amd import _capi
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", CSRC, "release"], stdout=subprocess.DEVNULL)
    for path in (TESTING, RELEASE):
        have = exported(path)
        assert [c for c in CALLS if c in have] == CALLS, path
    assert [c for c in CALLS if c in header_symbols(testing=False)] == CALLS
    assert exported(RELEASE) == header_symbols(testing=False)
    assert sorted(_capi.PROTOTYPES) == header_symbols(testing=True)
    for c in CALLS:
        assert hasattr(lib, c)
        assert _capi.PROTOTYPES[c][0] is C.c_int32 and _capi.PROTOTYPES[c][1][0] is C.c_void_p
    info = C.POINTER(_capi.FollowInfo)
    assert _capi.PROTOTYPES["th_follow_set"][1][1:] == [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32]
    assert _capi.PROTOTYPES["th_follow_sample"][1][1:] == [C.c_int32, C.c_double]
    assert _capi.PROTOTYPES["th_follow_read"][1][1:] == [C.c_uint64, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_double), info]
    assert _capi.PROTOTYPES["th_follow_query"][1][1:] == [info, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


def test_the_abi_version_is_still_14(lib):
    assert lib.th_abi_version() == 14
    assert "#define TH_ABI_VERSION 14\n" in open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()


def test_the_info_block_is_48_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    I = _capi.FollowInfo
    assert C.sizeof(I) == 48
    assert {k: getattr(I, k).offset for k, _ in I._fields_} == INFO_OFFSETS
    assert all(t is C.c_uint64 for _, t in I._fields_)
    # ... and as a C compiler lays the header's declaration out, with the limits' values
    lines = ['#include <stddef.h>\n#include "tendrils_hip.h"\n', "_Static_assert(sizeof(th_follow_info) == 48, \"size\");\n"]
    lines += ["_Static_assert(offsetof(th_follow_info, %s) == %d, \"info.%s\");\n" % (k, v, k) for k, v in INFO_OFFSETS.items()]
    lines += ["_Static_assert(%s == %d, \"%s\");\n" % (k, v, k) for k, v in CONSTANTS.items()]
    # the history at its limit is 256 MiB: 16 bytes a particle and sample
    lines += ["_Static_assert((unsigned long long)TH_FOLLOW_MAX_ENTRIES * 16ull == 256ull << 20, \"256 MiB\");\n"]
    source = tmp_path / "follow_layout.c"
    source.write_text("".join(lines))
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    for name, value in CONSTANTS.items():
        assert getattr(_capi, name[3:]) == value, name


def test_the_unit_is_in_core():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    core = re.search(r"^CORE\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "th_follow.hip" in core            # (CORE is what both the testing and the release library link)


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped()
    assert "asm" not in code.lower()
    assert "hiprtc" not in code.lower()
    assert "getenv" not in code                # (no switch between development arms is left in the product)
    kernels = re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)
    assert set(kernels) == KERNELS and len(kernels) == len(KERNELS)
    assert len(re.findall(r"__launch_bounds__\(256\)", code)) == len(KERNELS)
    # one atomic: the mark kernel's OR into a 64-bit word of the mask, of an integer shifted into place
    assert re.findall(r"\batomic\w+", code) == ["atomicOr"]
    call_, = re.findall(r"atomicOr\s*\(([^;]*);", code)
    assert "float" not in call_ and "double" not in call_ and "1ull <<" in call_ and "&mask[" in call_
    assert "unsigned long long *mask)" in code
    # no wave-wide operation: a lane past the end may leave
    assert not re.search(r"__(ballot|shfl\w*|syncthreads|any|all)\b", code)
    # the slot loader is select's
    assert '#include "th_select_match.hpp"' in code and "struct Slot" not in code and "Slot<PACKED>::load" in code


def test_select_and_the_histogram_are_as_they_were():
    for unit, kernels in (("th_select.hip", {"select_clear_kernel", "select_mark_kernel", "select_count_kernel", "select_total_kernel", "select_gather_kernel"}),
                          ("th_histogram.hip", {"hist_clear_kernel", "hist_tally_kernel"})):
        code = stripped(unit)
        assert set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)) == kernels, unit
        assert "follow" not in code.lower(), unit
    # following uses scratch of its own: select's device addresses stay valid until the next select
    assert "select_" not in stripped().replace("th_select_match.hpp", "")


def test_no_prelude_and_no_program_kind_came_with_it():
    preludes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_prelude.inc")))
    assert preludes == ["th_draw_prelude.inc", "th_fragment_pair_prelude.inc", "th_fragment_prelude.inc", "th_measure_prelude.inc",
                        "th_program_prelude.inc", "th_screen_prelude.inc", "th_step_prelude.inc"]
    assert "follow" not in open(os.path.join(CSRC, "th_program_kinds.hpp")).read().lower()
