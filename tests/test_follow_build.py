"""Follow (include/tendrils_hip.h "follow"; tendrils_amd/csrc/th_follow.hip), the part that needs no GPU: both libraries export
th_follow_set, th_follow_sample, th_follow_read and th_follow_query, the header, the libraries' symbol tables and the ctypes
binding agree, the ABI version stays 14, th_follow_info has the size and offsets the header states on both sides, the limits their
values, the unit is linked into both libraries, holds no assembly statement, no run-time compilation and no switch read from the
environment, its only atomic is the integer OR of the mark kernel - and the pass is a built-in one: no prelude and no program
kind came with it."""
import ctypes as C
import re

from builtin_pass import (assert_c_layout, assert_exported_and_bound, assert_fixed_integer_code, kernels, lib, stripped,      # noqa: F401
                          test_no_prelude_and_no_program_kind_came_with_it, test_the_abi_version_is_still_14, test_the_unit_is_in_core)

CALLS = ["th_follow_query", "th_follow_read", "th_follow_sample", "th_follow_set"]
INFO_OFFSETS = dict(particles=0, followed=8, depth=16, samples=24, held=32, locates=40)
CONSTANTS = dict(TH_FOLLOW_MAX_PARTICLES=1 << 20, TH_FOLLOW_MAX_DEPTH=1 << 16, TH_FOLLOW_MAX_ENTRIES=1 << 24)
KERNELS = {"follow_mark_kernel", "follow_fill_kernel", "follow_locate_kernel", "follow_gather_kernel"}


def test_both_libraries_export_the_calls_and_header_nm_and_binding_agree(lib):
    from tendrils_amd import _capi
    assert_exported_and_bound(lib, CALLS)
    for c in CALLS:
        assert _capi.PROTOTYPES[c][1][0] is C.c_void_p
    info = C.POINTER(_capi.FollowInfo)
    assert _capi.PROTOTYPES["th_follow_set"][1][1:] == [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32]
    assert _capi.PROTOTYPES["th_follow_sample"][1][1:] == [C.c_int32, C.c_double]
    assert _capi.PROTOTYPES["th_follow_read"][1][1:] == [C.c_uint64, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_double), info]
    assert _capi.PROTOTYPES["th_follow_query"][1][1:] == [info, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


def test_the_info_block_is_48_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    I = _capi.FollowInfo
    assert C.sizeof(I) == 48
    assert {k: getattr(I, k).offset for k, _ in I._fields_} == INFO_OFFSETS
    assert all(t is C.c_uint64 for _, t in I._fields_)
    # ... and as a C compiler lays the header's declaration out, with the limits' values
    # (the history at its limit is 256 MiB: 16 bytes a particle and sample)
    assert_c_layout(tmp_path, [("sizeof(th_follow_info) == 48", "size")]
                    + [("offsetof(th_follow_info, %s) == %d" % (k, v), "info." + k) for k, v in INFO_OFFSETS.items()]
                    + [("%s == %d" % (k, v), k) for k, v in CONSTANTS.items()]
                    + [("(unsigned long long)TH_FOLLOW_MAX_ENTRIES * 16ull == 256ull << 20", "256 MiB")])
    for name, value in CONSTANTS.items():
        assert getattr(_capi, name[3:]) == value, name


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped("th_follow.hip")
    assert_fixed_integer_code(code, {"atomicOr"})         # (getenv: no switch between development arms is left in the product)
    assert set(kernels(code)) == KERNELS and len(kernels(code)) == len(KERNELS)
    assert len(re.findall(r"__launch_bounds__\(256\)", code)) == len(KERNELS)
    # one atomic: the mark kernel's OR into a 64-bit word of the mask, of an integer shifted into place
    assert re.findall(r"\batomic\w+", code) == ["atomicOr"]
    call_, = re.findall(r"atomicOr\s*\(([^;]*);", code)
    assert "float" not in call_ and "double" not in call_ and "1ull <<" in call_ and "&mask[" in call_
    assert "unsigned long long *mask)" in code
    # no wave-wide operation: a lane past the end may leave
    assert not re.search(r"__(ballot|shfl\w*|syncthreads|any|all)\b", code)
    # the slot loader and the rank are the shared ones; the set is cleared and ranked by the launchers beside the scan
    assert '#include "th_ring.hpp"' in code and "struct Slot" not in code and "Slot<PACKED>::load" in code and "texel_rank(set, t)" in code
    assert "launch_texel_set_clear(" in code and "launch_texel_set_rank(" in code and "__popcll" not in code


def test_select_and_the_histogram_are_as_they_were():
    for unit, names in (("th_select.hip", {"select_clear_kernel", "select_mark_kernel", "select_total_kernel", "select_gather_kernel"}),
                        ("th_histogram.hip", {"hist_clear_kernel", "hist_tally_kernel"})):
        code = stripped(unit)
        assert set(kernels(code)) == names, unit
        assert "follow" not in code.lower(), unit
    # following uses scratch of its own - a TexelSet beside select's, two members of the context: select's device addresses stay
    # valid until the next select
    context = stripped("th_ctx.hpp")
    assert len(re.findall(r"\bthi::TexelSet\s+\w+;", context)) == 2 and "thi::TexelSet select_set;" in context and "thi::TexelSet follow_texels;" in context
    assert "select_" not in stripped("th_follow.hip") and "follow_" not in stripped("th_select.hip")
