"""The density map (include/tendrils_hip.h "density map"; tendrils_amd/csrc/th_density.hip), the part that needs no GPU: both
libraries export th_density and th_density_async, the header, the libraries' symbol tables and the ctypes binding agree, the ABI
version stays 14, the two structures have the sizes the header states on both sides, the unit holds no assembly statement, and
the pass is a built-in one - no prelude came with it."""
import ctypes as C

from builtin_pass import (assert_c_layout, assert_exported_and_bound, assert_fixed_integer_code, kernels, lib, stripped,      # noqa: F401
                          test_no_prelude_and_no_program_kind_came_with_it, test_the_abi_version_is_still_14, test_the_unit_is_in_core)

CALLS = ["th_density", "th_density_async"]


def test_both_libraries_export_the_calls_and_header_nm_and_binding_agree(lib):
    from tendrils_amd import _capi
    assert_exported_and_bound(lib, CALLS)
    for c in CALLS:
        args = _capi.PROTOTYPES[c][1]
        assert len(args) == 4 and args[1] == C.POINTER(_capi.DensityUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_density"][1][3] == C.POINTER(_capi.DensityInfo)
    assert _capi.PROTOTYPES["th_density_async"][1][3] == C.POINTER(C.c_void_p)


def test_the_structures_are_24_and_40_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    U, I = _capi.DensityUniforms, _capi.DensityInfo
    assert C.sizeof(U) == 24 and C.sizeof(I) == 40
    assert (U.viewSize.offset, U.w.offset, U.h.offset, U.dest.offset, U.slot.offset) == (0, 8, 12, 16, 20)
    assert [I.particles.offset, I.live.offset, I.inside.offset, I.outside.offset, I.nonfinite_velocity.offset] == [0, 8, 16, 24, 32]
    # ... and as a C compiler lays the header's declarations out
    assert_c_layout(tmp_path, [
        ("sizeof(th_density_uniforms) == 24", "uniforms"), ("sizeof(th_density_info) == 40", "info"),
        ("offsetof(th_density_uniforms, w) == 8 && offsetof(th_density_uniforms, dest) == 16 && offsetof(th_density_uniforms, slot) == 20", "uniform fields"),
        ("offsetof(th_density_info, nonfinite_velocity) == 32", "info fields"), ("TH_VIEW_TEXTURE == 0 && TH_VIEW_SPAWN_IMAGE == 2", "destinations")])
    assert (_capi.VIEW_TEXTURE, _capi.VIEW_SPAWN_IMAGE) == (0, 2)


def test_the_unit_holds_no_assembly_and_no_float_atomic():
    code = stripped("th_density.hip")
    assert kernels(code) == ["density_clear_kernel", "density_tally_kernel", "density_convert_kernel"]
    # every atomic of the unit adds, or takes the minimum / maximum of, an integer: nothing of a float type goes near one
    assert_fixed_integer_code(code, {"atomicAdd", "atomicMin", "atomicMax"})
    # the slot loader, the butterflies and the counters' fold are the shared ones (tests/test_select_build.py checks them)
    assert '#include "th_ring.hpp"' in code and "struct Slot" not in code and "__shfl" not in code
    assert "fold_counters<kLive, kOutside, kNonfinite>(tally, p.info, {live, outside, nonfinite})" in code
