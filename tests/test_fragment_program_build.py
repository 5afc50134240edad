"""Fragment programs (include/tendrils_hip.h "fragment programs"), the part that needs no GPU: the library and the release library
export the three calls and the binding declares them, th_fragment_program_compile builds a caller's fragment stage for gfx950
through hiprtc on any machine behind a prelude of its own, a source that lacks th_fragment_main or names an accessor the stage
does not have fails on the caller's own line, and the other kinds compile as before."""
import ctypes as C
import os
import subprocess

import pytest

from test_draw_program_build import FLOW
from test_program_build import DRIFT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("th_fragment_program_compile", "th_draw_stages_run", "th_draw_stages_emit")

IDENTITY = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    return f.color;
}
"""

# a vignette, a stripe by window texel, a tint from the colour map at the window position, alpha shaped by a uniform: x, y,
# coord, viewRes, color, pass, the uniform block and a th_colormap tap, in + - *, fminf / fmaxf and selects only (with
# contraction off numpy restates it exactly: tests/test_gpu_fragment_program.py)
VIGNETTE = """struct FragUniforms { float tint[4]; float invRes[2]; float edge; float gain; };
__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    const FragUniforms &u = th_uniforms<FragUniforms>(f);
    const float cx = f.coord.x - 0.5f * f.viewRes.x, cy = f.coord.y - 0.5f * f.viewRes.y;
    const float fall = fmaxf(1.0f - (cx * cx + cy * cy) * u.edge, 0.25f);
    const float4 m = th_colormap(f, f.coord.x * u.invRes[0], f.coord.y * u.invRes[1]);
    const float stripe = ((f.x + 3u * f.y) & 1u) ? u.gain : 1.0f;
    const float k = fall * stripe;
    float4 o;
    o.x = f.color.x * k + m.x * u.tint[0];
    o.y = f.color.y * k + m.y * u.tint[1];
    o.z = f.pass == TH_PASS_VIEW ? f.color.z * k + m.z * u.tint[2] : f.color.z;
    o.w = fminf(f.color.w * u.tint[3] + m.w * 0.125f, 1.0f);
    return o;
}
"""

# the entry point is missing (the function has another name)
NO_MAIN = """__device__ float4 fragment(const th_fragment_pass &f)
{
    return f.color;
}
"""

# line 4 reads the particles: a fragment stage has no such accessor
NAMES_PARTICLES = """__device__ float4 th_fragment_main(const th_fragment_pass &f)
{
    float4 o = f.color;
    o.x = th_particles(f, 0.5f, 0.5f).x;
    return o;
}
"""


class FragUniforms(C.Structure):
    _fields_ = [("tint", C.c_float * 4), ("invRes", C.c_float * 2), ("edge", C.c_float), ("gain", C.c_float)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def compile_with(lib, entry, source, name=b"test_fragment"):
    handle = C.c_void_p()
    status = getattr(lib, entry)(source.encode(), name, C.byref(handle))
    return status, handle


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_calls_and_the_binding_declares_them(lib):
    from tendrils_amd import _capi
    release = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
    if not os.path.exists(release):
        import __graft_entry__ as g
        g.build()
    for path in (_capi.LIB_PATH, release):
        names = exported(path)
        for call in CALLS:
            assert call in names, "%s does not export %s" % (path, call)
    for call in CALLS:
        assert call in _capi.PROTOTYPES and hasattr(lib, call)
    assert C.sizeof(_capi.DrawStages) == 56           # three pointers, each slot's size behind its block, on 8-byte boundaries
    assert lib.th_abi_version() == 14


@pytest.mark.parametrize("source", [IDENTITY, VIGNETTE], ids=["identity", "vignette"])
def test_a_fragment_program_compiles_with_no_device(lib, source):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", source)
    assert status == _capi.TH_OK, (lib.th_last_error(), lib.th_program_log())
    assert handle.value and lib.th_program_log() == b""
    assert len(_capi._mapped("libhiprtc")) == 1 and len(_capi._mapped("libamdhip64")) == 1
    assert lib.th_program_destroy(handle) == _capi.TH_OK


def test_a_source_without_the_entry_point_does_not_compile(lib):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", NO_MAIN, b"no_main")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_fragment_main" in lib.th_program_log().decode()
    assert b"no_main" in lib.th_last_error()


def test_naming_th_particles_fails_on_the_callers_own_line(lib):
    from tendrils_amd import _capi
    status, handle = compile_with(lib, "th_fragment_program_compile", NAMES_PARTICLES, b"reads_particles")
    assert status == _capi.TH_ERR_INVALID and not handle.value
    log = lib.th_program_log().decode()
    assert "reads_particles:4:" in log and "th_particles" in log and "error" in log, log


def test_the_other_kinds_still_compile_and_keep_their_own_preludes(lib):
    from tendrils_amd import _capi
    for entry, good in (("th_draw_program_compile", FLOW), ("th_program_compile", DRIFT)):
        status, handle = compile_with(lib, entry, good)
        assert status == _capi.TH_OK and lib.th_program_log() == b"", lib.th_program_log()
        assert lib.th_program_destroy(handle) == _capi.TH_OK
        status, handle = compile_with(lib, entry, IDENTITY)           # a fragment stage is no program of theirs
        assert status == _capi.TH_ERR_INVALID and not handle.value
        assert "test_fragment:1:" in lib.th_program_log().decode() and "th_fragment_pass" in lib.th_program_log().decode()
    status, handle = compile_with(lib, "th_fragment_program_compile", FLOW)      # ... nor a vertex stage a fragment program
    assert status == _capi.TH_ERR_INVALID and not handle.value
    assert "th_vertex" in lib.th_program_log().decode()


def test_the_python_host_compiles_and_raises_with_the_compilers_output(lib):
    import tendrils_amd as ta
    from tendrils_amd.particles import DrawProgram, FragmentProgram, shader_stages
    with pytest.raises(ta.TendrilsHipError) as e:
        FragmentProgram.from_source(NAMES_PARTICLES, name="reads_particles")
    assert e.value.status == 1 and "reads_particles:4:" in str(e.value)
    frag = ta.FragmentProgram.from_source(VIGNETTE, FragUniforms, "vignette")
    vert = DrawProgram.from_source(FLOW, name="flow")
    assert frag.kind == "fragment" and frag.handle
    block = frag.pack(dict(tint=[1, 2, 3, 4], gain=0.5, unknown=7))
    assert list(block.tint) == [1, 2, 3, 4] and block.gain == 0.5 and block.edge == 0
    # what flowShader / renderShader accept
    assert shader_stages(None) == (None, None) and shader_stages(vert) == (vert, None) and shader_stages(frag) == (None, frag)
    assert shader_stages((vert, frag)) == (vert, frag) and shader_stages([None, frag]) == (None, frag) and shader_stages((None, None)) == (None, None)
    for bad in ((frag, vert), (vert, frag, None), (vert, vert), "flow"):
        with pytest.raises(TypeError):
            shader_stages(bad)
    frag.dispose()
    with pytest.raises(TypeError):
        shader_stages((vert, frag))                 # a disposed program is no stage
    vert.dispose()
