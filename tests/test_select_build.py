"""Select (include/tendrils_hip.h "select"; tendrils_amd/csrc/th_select.hip), the part that needs no GPU: both libraries export
th_select and th_select_async, the header, the libraries' symbol tables and the ctypes binding agree, the ABI version stays 14,
the three structures have the sizes and offsets the header states on both sides, the flags are 1, 2, 4, the unit is linked into
both libraries, holds no assembly statement and no run-time compilation, its one atomic is an integer OR and the shared device
code's (th_ring.hpp, the texel set's kernels in th_sort.hip) integer adds - and the pass is a built-in one: no prelude and no
program kind came with it."""
import ctypes as C
import re

from builtin_pass import (HEADER, SHARED, assert_c_layout, assert_exported_and_bound, assert_fixed_integer_code, kernels, lib, stripped,      # noqa: F401
                          test_no_prelude_and_no_program_kind_came_with_it, test_the_abi_version_is_still_14, test_the_unit_is_in_core)

CALLS = ["th_select", "th_select_async"]


def test_both_libraries_export_the_calls_and_header_nm_and_binding_agree(lib):
    from tendrils_amd import _capi
    assert_exported_and_bound(lib, CALLS)
    for c in CALLS:
        args = _capi.PROTOTYPES[c][1]
        assert len(args) == 6 and args[1] == C.POINTER(_capi.SelectUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_select"][1][3:] == [C.POINTER(_capi.Selected), C.c_uint64, C.POINTER(_capi.SelectInfo)]
    assert _capi.PROTOTYPES["th_select_async"][1][3:] == [C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]


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
    assert_c_layout(tmp_path, [
        ("sizeof(th_select_uniforms) == 40 && sizeof(th_selected) == 32 && sizeof(th_select_info) == 32", "sizes"),
        ("offsetof(th_select_uniforms, box) == 0 && offsetof(th_select_uniforms, speed2) == 16 && offsetof(th_select_uniforms, stride) == 24 && "
         "offsetof(th_select_uniforms, phase) == 28 && offsetof(th_select_uniforms, flags) == 32 && offsetof(th_select_uniforms, reserved) == 36", "uniform fields"),
        ("offsetof(th_selected, state) == 0 && offsetof(th_selected, index) == 16 && offsetof(th_selected, x) == 20 && "
         "offsetof(th_selected, y) == 24 && offsetof(th_selected, reserved) == 28", "record fields"),
        ("offsetof(th_select_info, particles) == 0 && offsetof(th_select_info, live) == 8 && offsetof(th_select_info, matched) == 16 && "
         "offsetof(th_select_info, written) == 24", "info fields"),
        ("TH_SELECT_BOX == 1u && TH_SELECT_SPEED == 2u && TH_SELECT_INERT == 4u", "flags")])


def test_the_flags_are_1_2_4():
    from tendrils_amd import _capi
    assert (_capi.SELECT_BOX, _capi.SELECT_SPEED, _capi.SELECT_INERT) == (1, 2, 4)
    header = open(HEADER).read()
    for name, value in (("BOX", 1), ("SPEED", 2), ("INERT", 4)):
        assert re.search(r"^#define TH_SELECT_%s\s+%du\b" % (name, value), header, flags=re.M), name


def test_the_unit_holds_no_assembly_no_runtime_compilation_and_only_integer_atomics():
    code = stripped("th_select.hip")
    assert_fixed_integer_code(code, {"atomicOr"})
    assert set(kernels(code)) == {"select_clear_kernel", "select_mark_kernel", "select_total_kernel", "select_gather_kernel"}
    assert re.findall(r"\batomic\w+", code) == ["atomicOr"]            # (the live count's add is the shared fold's)
    # the texel set is ranked by the shared launcher - the scan as it is -, the texel-order fast path's ballot is the mask word
    assert "launch_texel_set_rank" in code and "fold_counters<kLive>(part, p.info, {live_n})" in code and "__ballot" in code
    assert "launch_exclusive_scan_u32(counts, block_sums, nwords, s)" in stripped("th_sort.hip")


def test_the_shared_device_code_is_fixed_integer_code_too():
    ring, sort = (stripped(name) for name in SHARED)
    assert_fixed_integer_code(ring, {"atomicAdd"})
    assert_fixed_integer_code(sort, {"atomicAdd"})
    assert re.findall(r"atomicAdd\s*\(([^;]*);", ring) == ["&info[to], (unsigned long long)n)"] and not kernels(ring)
    assert "texel_set_count_kernel" in kernels(sort) and "hipMemsetAsync(mask, 0, (size_t)nwords * sizeof *mask, s)" in sort
