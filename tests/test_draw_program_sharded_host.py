"""Draw programs on row-band shards, the part that needs no GPU: the two entry points (th_draw_program_emit,
th_draw_program_sharded) are bound with the signatures include/tendrils_hip.h declares and exported by the library - the
release library too -, and the sharded route of the Python host packs a program's uniforms from the same function as the
unsharded draw()."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendrils_amd", "csrc")
RELEASE = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
NEW = ("th_draw_program_emit", "th_draw_program_sharded")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from tendrils_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi.load()


def header_parameters(name):
    """the parameter list of `th_status name(...)` in the header, one C declaration per parameter"""
    text = open(os.path.join(ROOT, "include", "tendrils_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.findall(r"\bth_status\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert len(found) == 1, (name, found)
    return [" ".join(p.split()) for p in found[0].split(",")]


def ctype_of(parameter):
    """the ctypes type tendrils_amd/_capi.py binds a C parameter with"""
    from tendrils_amd import _capi
    kind = parameter.rsplit(" ", 1)[0] + (" *" * parameter.rsplit(" ", 1)[1].count("*"))
    kind = " ".join(kind.replace("*", " * ").split())
    return {"th_context *": C.c_void_p, "th_program *": C.c_void_p, "const void *": C.c_void_p, "uint32_t": C.c_uint32, "int32_t": C.c_int32,
            "uint64_t *": C.POINTER(C.c_uint64), "void * *": C.POINTER(C.c_void_p),
            "const th_deposit_uniforms *": C.POINTER(_capi.DepositUniforms), "const th_render_uniforms *": C.POINTER(_capi.RenderUniforms)}[kind]


def test_the_binding_declares_both_calls_as_the_header_does():
    from tendrils_amd import _capi
    assert [len(header_parameters(n)) for n in NEW] == [8, 11]
    for name in NEW:
        result, arguments = _capi.PROTOTYPES[name]
        assert result is C.c_int32
        assert arguments == [ctype_of(p) for p in header_parameters(name)], name


def test_the_library_exports_both_calls(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == list(_prototype(name))


def _prototype(name):
    from tendrils_amd import _capi
    return _capi.PROTOTYPES[name][1]


def test_the_release_library_exports_both_calls(lib):
    """built as tests/test_release_build.py builds it"""
    subprocess.check_call(["make", "-j3", "-C", CSRC, "release"], stdout=subprocess.DEVNULL)
    out = subprocess.run(["nm", "-D", "--defined-only", RELEASE], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (th_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NEW) <= exported


def test_the_sharded_route_packs_uniforms_with_the_unsharded_function():
    """one function makes the dict a program's block is packed from - Tendrils.draw_program_uniforms - and both routes call it:
    Tendrils.draw for the unsharded passes, sharding.draw_sharded_programs for a band's.  Likewise th_deposit_uniforms: nothing in
    tendrils.py or sharding.py constructs one but a deposit_uniforms() - Tendrils.deposit_uniforms hands the frame's scalars to
    particles.deposit_uniforms, which Particles.deposit_flow and export_lines (they take scalars) build theirs with too"""
    from tendrils_amd import particles, sharding, tendrils
    from tendrils_amd.tendrils import Tendrils
    local, sharded = inspect.getsource(Tendrils.draw), inspect.getsource(sharding.draw_sharded_programs)
    assert "self.draw_program_uniforms()" in local and "tendrils.draw_program_uniforms()" in sharded
    for source in (local, sharded):                # ... and neither builds a dict of its own
        assert "dict(" not in source and ".update(" not in source
    assert "draw_sharded_programs" in local
    for route in (sharding.draw_sharded, sharding.draw_sharded_native):
        assert "draw_sharded_programs" in inspect.getsource(route)
    builder = inspect.getsource(particles.deposit_uniforms)
    assert "DepositUniforms(" in builder and "deposit_uniforms(" in inspect.getsource(Tendrils.deposit_uniforms)
    for module in (tendrils, sharding):
        assert "DepositUniforms(" not in inspect.getsource(module), module.__name__
    assert "DepositUniforms(" not in inspect.getsource(particles).replace(builder, "")


class _Stub:
    """as much of a Tendrils as draw_program_uniforms reads"""
    def __init__(self, shape, band):
        self.state = dict(speedLimit=0.01, flowDecay=0.5)
        self.timer = type("T", (), dict(time=12.5))()
        self.viewSize, self.viewRes = [1.0, 0.5], [96, 54]
        self.particles = type("P", (), dict(shape=list(shape), geomShape=[shape[0], 2 * shape[1]]))()
        self.colorMap = type("M", (), dict(shape=[4, 3]))()
        self.uniforms = dict(render=dict(zoom=2.0, flowDecay=0.25))
        self._band = band


def test_a_band_hands_its_programs_the_whole_textures_shape():
    from tendrils_amd.tendrils import Tendrils
    whole = Tendrils.draw_program_uniforms(_Stub((100, 100), (0, 100, 100)))
    band = Tendrils.draw_program_uniforms(_Stub((100, 33), (34, 33, 100)))
    unsharded = Tendrils.draw_program_uniforms(_Stub((100, 100), (0, None, 0)))
    assert whole == band == unsharded
    assert band["dataRes"] == [100, 100] and band["geomRes"] == [100, 200]
    assert band["zoom"] == 2.0 and band["flowDecay"] == 0.25 and band["time"] == 12.5 and band["colorMapRes"] == [4, 3]
