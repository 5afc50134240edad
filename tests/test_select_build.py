"""Select (include/tendrils_hip.h "select"; tendrils_amd/csrc/th_select.hip), the part that needs no GPU: both libraries export
th_select and th_select_async, the header, the libraries' symbol tables and the ctypes binding agree, the ABI version stays 14,
the three structures have the sizes and offsets the header states on both sides, the flags are 1, 2, 4, the unit is linked into
both libraries, holds no assembly statement and no run-time compilation, its atomics are integer ORs and adds - and the pass is a
built-in one: no prelude and no program kind came with it."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["th_select", "th_select_async"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def stripped():
    text = open(os.path.join(CSRC, "th_select.hip")).read()
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
        res, args = _capi.PROTOTYPES[c]
        assert res is C.c_int32 and len(args) == 6 and args[1] == C.POINTER(_capi.SelectUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_select"][1][3:] == [C.POINTER(_capi.Selected), C.c_uint64, C.POINTER(_capi.SelectInfo)]
    assert _capi.PROTOTYPES["th_select_async"][1][3:] == [C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


def test_the_abi_version_is_still_14(lib):
    assert lib.th_abi_version() == 14
    assert "#define TH_ABI_VERSION 14\n" in open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()


def test_the_structures_are_40_32_and_32_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    from tendrils_amd.particles import SELECTED
    U, R, I = _capi.SelectUniforms, _capi.Selected, _capi.SelectInfo
    assert (C.sizeof(U), C.sizeof(R), C.sizeof(I)) == (40, 32, 32)
    assert (U.box.offset, U.speed2.offset, U.stride.offset, U.phase.offset, U.flags.offset, U.reserved.offset) == (0, 16, 24, 28, 32, 36)
    assert (R.state.offset, R.index.offset, R.x.offset, R.y.offset, R.reserved.offset) == (0, 16, 20, 24, 28)
    assert (I.particles.offset, I.live.offset, I.matched.offset, I.written.offset) == (0, 8, 16, 24)
    # (the numpy view of a record the host reads the records through)
    assert SELECTED.itemsize == 32 and [SELECTED.fields[k][1] for k in ("state", "index", "x", "y", "reserved")] == [0, 16, 20, 24, 28]
    # ... and as a C compiler lays the header's declarations out
    source = tmp_path / "select_layout.c"
    source.write_text('#include <stddef.h>\n#include "tendrils_hip.h"\n'
                      "_Static_assert(sizeof(th_select_uniforms) == 40 && sizeof(th_selected) == 32 && sizeof(th_select_info) == 32, \"sizes\");\n"
                      "_Static_assert(offsetof(th_select_uniforms, box) == 0 && offsetof(th_select_uniforms, speed2) == 16 && "
                      "offsetof(th_select_uniforms, stride) == 24 && offsetof(th_select_uniforms, phase) == 28 && "
                      "offsetof(th_select_uniforms, flags) == 32 && offsetof(th_select_uniforms, reserved) == 36, \"uniform fields\");\n"
                      "_Static_assert(offsetof(th_selected, state) == 0 && offsetof(th_selected, index) == 16 && offsetof(th_selected, x) == 20 && "
                      "offsetof(th_selected, y) == 24 && offsetof(th_selected, reserved) == 28, \"record fields\");\n"
                      "_Static_assert(offsetof(th_select_info, particles) == 0 && offsetof(th_select_info, live) == 8 && "
                      "offsetof(th_select_info, matched) == 16 && offsetof(th_select_info, written) == 24, \"info fields\");\n"
                      "_Static_assert(TH_SELECT_BOX == 1u && TH_SELECT_SPEED == 2u && TH_SELECT_INERT == 4u, \"flags\");\n")
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_flags_are_1_2_4():
    from tendrils_amd import _capi
    assert (_capi.SELECT_BOX, _capi.SELECT_SPEED, _capi.SELECT_INERT) == (1, 2, 4)
    header = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    for name, value in (("BOX", 1), ("SPEED", 2), ("INERT", 4)):
        assert re.search(r"^#define TH_SELECT_%s\s+%du\b" % (name, value), header, flags=re.M), name


def test_the_unit_is_in_core():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    core = re.search(r"^CORE\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "th_select.hip" in core            # (CORE is what both the testing and the release library link)


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped()
    assert "asm" not in code.lower()
    assert "hiprtc" not in code.lower()
    kernels = re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)
    assert {"select_mark_kernel", "select_gather_kernel"} <= set(kernels)
    atomics = set(re.findall(r"\batomic\w+", code))
    assert atomics and atomics <= {"atomicOr", "atomicAdd"}
    for call_ in re.findall(r"atomic\w+\s*\(([^;]*);", code):
        assert "float" not in call_ and "double" not in call_, call_
    # the shared scan is used as it is
    assert "launch_exclusive_scan_u32" in code and "__ballot" in code


def test_no_prelude_and_no_program_kind_came_with_it():
    preludes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_prelude.inc")))
    assert preludes == ["th_draw_prelude.inc", "th_fragment_pair_prelude.inc", "th_fragment_prelude.inc", "th_measure_prelude.inc",
                        "th_program_prelude.inc", "th_screen_prelude.inc", "th_step_prelude.inc"]
    assert "select" not in open(os.path.join(CSRC, "th_program_kinds.hpp")).read().lower()
