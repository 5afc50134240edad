"""The histogram (include/tendrils_hip.h "histogram"; tendrils_amd/csrc/th_histogram.hip), the part that needs no GPU: both
libraries export th_histogram and th_histogram_async, the header, the libraries' symbol tables and the ctypes binding agree, the
ABI version stays 14, the two structures have the sizes and offsets the header states on both sides, the constants their values,
the unit is linked into both libraries, holds no assembly statement and no run-time compilation, its atomics are integer adds,
it evaluates select's predicate through the header select does - and the pass is a built-in one: no prelude and no program
kind came with it."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["th_histogram", "th_histogram_async"]
CONSTANTS = dict(TH_HIST_X=0, TH_HIST_Y=1, TH_HIST_VX=2, TH_HIST_VY=3, TH_HIST_SPEED2=4, TH_HIST_SPEED=5, TH_HIST_LINEAR=0, TH_HIST_KEY=1)
UNIFORM_OFFSETS = dict(select=0, channel=40, mode=44, bins=48, lo=52, hi=56, key_prefix=60, key_shift=64, reserved=68)
INFO_OFFSETS = dict(particles=0, live=8, matched=16, below=24, above=32, nan=40)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def stripped(name="th_histogram.hip"):
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
        res, args = _capi.PROTOTYPES[c]
        assert res is C.c_int32 and len(args) == 5 and args[1] == C.POINTER(_capi.HistogramUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_histogram"][1][3:] == [C.POINTER(C.c_uint32), C.POINTER(_capi.HistogramInfo)]
    assert _capi.PROTOTYPES["th_histogram_async"][1][3:] == [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


def test_the_abi_version_is_still_14(lib):
    assert lib.th_abi_version() == 14
    assert "#define TH_ABI_VERSION 14\n" in open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()


def test_the_structures_are_72_and_48_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    U, I = _capi.HistogramUniforms, _capi.HistogramInfo
    assert (C.sizeof(U), C.sizeof(I)) == (72, 48)
    assert {k: getattr(U, k).offset for k, _ in U._fields_} == UNIFORM_OFFSETS
    assert {k: getattr(I, k).offset for k, _ in I._fields_} == INFO_OFFSETS
    assert dict(U._fields_)["select"] is _capi.SelectUniforms and C.sizeof(_capi.SelectUniforms) == 40
    # ... and as a C compiler lays the header's declarations out, with the constants' values
    lines = ['#include <stddef.h>\n#include "tendrils_hip.h"\n',
             "_Static_assert(sizeof(th_histogram_uniforms) == 72 && sizeof(th_histogram_info) == 48, \"sizes\");\n"]
    lines += ["_Static_assert(offsetof(th_histogram_uniforms, %s) == %d, \"uniforms.%s\");\n" % (k, v, k) for k, v in UNIFORM_OFFSETS.items()]
    lines += ["_Static_assert(offsetof(th_histogram_info, %s) == %d, \"info.%s\");\n" % (k, v, k) for k, v in INFO_OFFSETS.items()]
    lines += ["_Static_assert(%s == %d, \"%s\");\n" % (k, v, k) for k, v in CONSTANTS.items()]
    source = tmp_path / "histogram_layout.c"
    source.write_text("".join(lines))
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_constants_have_the_headers_values():
    from tendrils_amd import _capi
    from tendrils_amd.particles import HIST_CHANNELS, QUANTILE_PASSES
    header = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s\s+%d\b" % (name, value), header, flags=re.M), name
        assert getattr(_capi, name[3:]) == value, name
    assert HIST_CHANNELS == dict(x=0, y=1, vx=2, vy=3, speed2=4, speed=5)
    # the radix select's three passes: 11, 11 and 10 bits of the key from the top, shifts 21, 10 and 0
    assert QUANTILE_PASSES == ((2048, 21), (2048, 10), (1024, 0))
    assert sum(bins.bit_length() - 1 for bins, _ in QUANTILE_PASSES) == 32


def test_the_key_of_a_float_orders_like_the_float_and_inverts():
    import numpy as np
    from tendrils_amd.particles import float_key, key_float
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.5, np.inf], np.float32)
    k = float_key(v).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert (key_float(float_key(v)).view(np.uint32) == v.view(np.uint32)).all()


def test_the_unit_is_in_core():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    core = re.search(r"^CORE\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "th_histogram.hip" in core         # (CORE is what both the testing and the release library link)
    assert "th_select_match.hpp" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1).split()


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped()
    assert "asm" not in code.lower()
    assert "hiprtc" not in code.lower()
    assert "getenv" not in code                # (no switch between development arms is left in the product)
    kernels = re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)
    assert set(kernels) == {"hist_clear_kernel", "hist_tally_kernel"}
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicAdd"}
    calls = re.findall(r"atomicAdd\s*\(([^;]*);", code)
    assert len(calls) >= 4
    for call_ in calls:
        assert "float" not in call_ and "double" not in call_, call_
    # every word an atomic adds to, and everything added, is declared an integer
    assert "extern __shared__ uint32_t lds[]" in code and "uint32_t *tally = lds, *hist = lds + " in code
    assert "uint32_t *counts;" in code and "unsigned long long *info;" in code
    assert not re.search(r"\b(float|double)\s*\*", code)


def test_select_and_the_histogram_evaluate_one_predicate():
    shared = stripped("th_select_match.hpp")
    assert len(re.findall(r"\bbool\s+select_match\s*\(", shared)) == 1 and "struct Slot<true>" in shared
    for unit in ("th_select.hip", "th_histogram.hip"):
        code = stripped(unit)
        assert '#include "th_select_match.hpp"' in code and "select_match(" in code and "select_checks(" in code, unit
        assert not re.search(r"\bbool\s+select_match\s*\(", code) and "struct Slot" not in code, unit


def test_no_prelude_and_no_program_kind_came_with_it():
    preludes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_prelude.inc")))
    assert preludes == ["th_draw_prelude.inc", "th_fragment_pair_prelude.inc", "th_fragment_prelude.inc", "th_measure_prelude.inc",
                        "th_program_prelude.inc", "th_screen_prelude.inc", "th_step_prelude.inc"]
    assert "hist" not in open(os.path.join(CSRC, "th_program_kinds.hpp")).read().lower()
