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

from builtin_pass import (CSRC, HEADER, assert_c_layout, assert_exported_and_bound, assert_fixed_integer_code, kernels, lib, stripped,      # noqa: F401
                          test_no_prelude_and_no_program_kind_came_with_it, test_the_abi_version_is_still_14, test_the_unit_is_in_core)

CALLS = ["th_histogram", "th_histogram_async"]
CONSTANTS = dict(TH_HIST_X=0, TH_HIST_Y=1, TH_HIST_VX=2, TH_HIST_VY=3, TH_HIST_SPEED2=4, TH_HIST_SPEED=5, TH_HIST_LINEAR=0, TH_HIST_KEY=1)
UNIFORM_OFFSETS = dict(select=0, channel=40, mode=44, bins=48, lo=52, hi=56, key_prefix=60, key_shift=64, reserved=68)
INFO_OFFSETS = dict(particles=0, live=8, matched=16, below=24, above=32, nan=40)


def test_both_libraries_export_the_calls_and_header_nm_and_binding_agree(lib):
    from tendrils_amd import _capi
    assert_exported_and_bound(lib, CALLS)
    for c in CALLS:
        args = _capi.PROTOTYPES[c][1]
        assert len(args) == 5 and args[1] == C.POINTER(_capi.HistogramUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_histogram"][1][3:] == [C.POINTER(C.c_uint32), C.POINTER(_capi.HistogramInfo)]
    assert _capi.PROTOTYPES["th_histogram_async"][1][3:] == [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


def test_the_structures_are_72_and_48_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    U, I = _capi.HistogramUniforms, _capi.HistogramInfo
    assert (C.sizeof(U), C.sizeof(I)) == (72, 48)
    assert {k: getattr(U, k).offset for k, _ in U._fields_} == UNIFORM_OFFSETS
    assert {k: getattr(I, k).offset for k, _ in I._fields_} == INFO_OFFSETS
    assert dict(U._fields_)["select"] is _capi.SelectUniforms and C.sizeof(_capi.SelectUniforms) == 40
    # ... and as a C compiler lays the header's declarations out, with the constants' values
    assert_c_layout(tmp_path, [("sizeof(th_histogram_uniforms) == 72 && sizeof(th_histogram_info) == 48", "sizes")]
                    + [("offsetof(th_histogram_uniforms, %s) == %d" % (k, v), "uniforms." + k) for k, v in UNIFORM_OFFSETS.items()]
                    + [("offsetof(th_histogram_info, %s) == %d" % (k, v), "info." + k) for k, v in INFO_OFFSETS.items()]
                    + [("%s == %d" % (k, v), k) for k, v in CONSTANTS.items()])


def test_the_constants_have_the_headers_values():
    from tendrils_amd import _capi
    from tendrils_amd.particles import HIST_CHANNELS, QUANTILE_PASSES
    header = open(HEADER).read()
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


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped("th_histogram.hip")
    assert_fixed_integer_code(code, {"atomicAdd"})        # (getenv: no switch between development arms is left in the product)
    assert set(kernels(code)) == {"hist_clear_kernel", "hist_tally_kernel"}
    # the bin's add in LDS and the flush of the bins; the five counters' adds are the shared fold's (tests/test_select_build.py)
    assert re.findall(r"atomicAdd\s*\(([^;]*);", code) == ["&hist[bin], 1u)", "&p.counts[i], n)"]
    assert "fold_counters<kLive, kMatched, kBelow, kAbove, kNan>(tally, p.info, {live, matched, below, above, nan})" in code
    # every word an atomic adds to, and everything added, is declared an integer
    assert "extern __shared__ uint32_t lds[]" in code and "uint32_t *tally = lds, *hist = lds + " in code
    assert "uint32_t *counts;" in code and "unsigned long long *info;" in code
    assert not re.search(r"\b(float|double)\s*\*", code)


ONCE = {r"\bbool\s+select_match\s*\(": "th_select_match.hpp", r"struct\s+Slot<true>": "th_ring.hpp", r"\bT\s+wave_sum\s*\(T\b": "th_ring.hpp",
        r"\bwave_sum\s*\([^()]*\)\s*\{": "th_ring.hpp", r"__popcll\(word & \(bit - 1ull\)\)": "th_ring.hpp"}


def test_select_and_the_histogram_evaluate_one_predicate():
    """... on one Slot, and the passes share one wave_sum (a template that serves both widths: no other definition of the name
    anywhere) and one popcount rank: each is defined exactly once across csrc/, in the shared header, and no unit defines its own"""
    sources = {os.path.basename(p): stripped(os.path.basename(p)) for ext in ("hip", "hpp", "inc") for p in glob.glob(os.path.join(CSRC, "*." + ext))}
    for pattern, home in ONCE.items():
        assert {name: len(re.findall(pattern, code)) for name, code in sources.items() if re.search(pattern, code)} == {home: 1}, pattern
    for unit in ("th_select.hip", "th_histogram.hip"):
        code = sources[unit]
        assert '#include "th_select_match.hpp"' in code and "select_match(" in code and "select_checks(" in code, unit
    assert '#include "th_ring.hpp"' in sources["th_select_match.hpp"]
