"""The density map (include/tendrils_hip.h "density map"; tendrils_amd/csrc/th_density.hip), the part that needs no GPU: both
libraries export th_density and th_density_async, the header, the libraries' symbol tables and the ctypes binding agree, the ABI
version stays 14, the two structures have the sizes the header states on both sides, the unit holds no assembly statement, and
the pass is a built-in one - no prelude came with it."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from test_release_build import CSRC, RELEASE, TESTING, exported, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["th_density", "th_density_async"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


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
        assert res is C.c_int32 and len(args) == 4 and args[1] == C.POINTER(_capi.DensityUniforms) and args[2] is C.c_int32
    assert _capi.PROTOTYPES["th_density"][1][3] == C.POINTER(_capi.DensityInfo)
    assert _capi.PROTOTYPES["th_density_async"][1][3] == C.POINTER(C.c_void_p)


def test_the_abi_version_is_still_14(lib):
    assert lib.th_abi_version() == 14
    assert "#define TH_ABI_VERSION 14\n" in open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()


def test_the_structures_are_24_and_40_bytes_on_both_sides(tmp_path):
    from tendrils_amd import _capi
    U, I = _capi.DensityUniforms, _capi.DensityInfo
    assert C.sizeof(U) == 24 and C.sizeof(I) == 40
    assert (U.viewSize.offset, U.w.offset, U.h.offset, U.dest.offset, U.slot.offset) == (0, 8, 12, 16, 20)
    assert [I.particles.offset, I.live.offset, I.inside.offset, I.outside.offset, I.nonfinite_velocity.offset] == [0, 8, 16, 24, 32]
    # ... and as a C compiler lays the header's declarations out
    source = tmp_path / "density_layout.c"
    source.write_text('#include <stddef.h>\n#include "tendrils_hip.h"\n'
                      "_Static_assert(sizeof(th_density_uniforms) == 24, \"uniforms\");\n"
                      "_Static_assert(sizeof(th_density_info) == 40, \"info\");\n"
                      "_Static_assert(offsetof(th_density_uniforms, w) == 8 && offsetof(th_density_uniforms, dest) == 16 && "
                      "offsetof(th_density_uniforms, slot) == 20, \"uniform fields\");\n"
                      "_Static_assert(offsetof(th_density_info, nonfinite_velocity) == 32, \"info fields\");\n"
                      "_Static_assert(TH_VIEW_TEXTURE == 0 && TH_VIEW_SPAWN_IMAGE == 2, \"destinations\");\n")
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert (_capi.VIEW_TEXTURE, _capi.VIEW_SPAWN_IMAGE) == (0, 2)


def test_the_unit_holds_no_assembly_and_no_float_atomic():
    text = open(os.path.join(CSRC, "th_density.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    assert "asm" not in code.lower()
    kernels = re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", code)
    assert kernels == ["density_clear_kernel", "density_tally_kernel", "density_convert_kernel"]
    assert "hiprtc" not in code
    # every atomic of the unit adds, or takes the minimum / maximum of, an integer: nothing of a float type goes near one
    for call_ in re.findall(r"atomic\w+\s*\(([^;]*);", code):
        assert "float" not in call_ and "double" not in call_, call_
    assert set(re.findall(r"\batomic\w+", code)) <= {"atomicAdd", "atomicMin", "atomicMax"}


def test_no_prelude_and_no_program_kind_came_with_it():
    preludes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_prelude.inc")))
    assert preludes == ["th_draw_prelude.inc", "th_fragment_pair_prelude.inc", "th_fragment_prelude.inc", "th_measure_prelude.inc",
                        "th_program_prelude.inc", "th_screen_prelude.inc", "th_step_prelude.inc"]
    assert "density" not in open(os.path.join(CSRC, "th_program_kinds.hpp")).read().lower()
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    core = re.search(r"^CORE\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "th_density.hip" in core            # (CORE is what both the testing and the release library link)
