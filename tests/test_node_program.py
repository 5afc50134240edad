"""User programs through the Node host (tendrils_amd/js/particles.js over the addon of th_napi_program.cc): a
{ source, uniforms: ArrayBuffer } program compiles without a GPU, and on the GPU the drift pass and a spawnData pass equal the
Python host's results bit for bit."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT, bits_equal, hashed_state

NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
ADDON = os.path.join(ROOT, "tendrils_amd", "lib", "tendrils_program.node")

DRIFT = """struct Drift { float k; };
__device__ float4 th_main(const th_pass &p)
{
    const Drift &u = th_uniforms<Drift>(p);
    float4 s = p.self;
    s.x = s.x + s.z * u.k;
    s.y = s.y + s.w * u.k;
    return s;
}
"""

DATA = """__device__ float4 th_main(const th_pass &p)
{
    return th_data(p, 1.0f - p.self.x, 1.0f - p.self.y);
}
"""


def node(script, *args):
    return subprocess.run([NODE, "-e", script, *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_addon_compiles_without_a_gpu_and_reports_the_users_line():
    if not os.path.exists(ADDON):
        import __graft_entry__ as g
        g.build()
    r = node("""
    const a = require('./tendrils_amd/lib/tendrils_program.node');
    const out = { keys: Object.getOwnPropertyNames(a).sort(), none: a.SOURCE_NONE };
    const h = a.programCompile(process.argv[1], 'drift');
    out.log = a.programLog();
    a.programDestroy(h); a.programDestroy(h);
    try { a.programCompile('__device__ float4 th_main(const th_pass &p)\\n{\\n  return p.self\\n}\\n', 'broken_pass'); }
    catch (e) { out.error = String(e); }
    console.log(JSON.stringify(out));
    """, DRIFT)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["keys"] == ["SOURCE_NONE", "programCompile", "programDestroy", "programLog", "programQuery", "programRun"]
    assert out["none"] == -5 and out["log"] == "" and "broken_pass:3:" in out["error"]


SCRIPT = """
const fs = require('fs'), path = require('path');
const { Particles, disposeProgram } = require('./tendrils_amd/js/particles');
const dir = process.argv[1], spec = JSON.parse(fs.readFileSync(path.join(dir, 'spec.json'), 'utf8'));
const f32 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const save = (name, arr) => fs.writeFileSync(path.join(dir, name), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
const p = new Particles(null, { shape: spec.shape });
p.setup(3);
p.uploadTexels(f32('state.bin'), 0);
p.uploadTexels(f32('texture.bin'), 1);
// the drift pass: the caller packs its own block
const drift = { source: spec.drift, name: 'drift', uniforms: new Float32Array([spec.k]).buffer };
p.logic = drift;
p.step();                                          // rotates: buffers[0] = drift(state)
save('drift.bin', p.read(0));
const order = p.buffers.map((b) => b.id);
const info = p.programQuery(drift);
// the spawnData pass: a buffer named before the rotation
const data = { source: spec.data, name: 'data' };
p.uploadTexels(f32('state.bin'), 0);
p.logic = data;
p.step({ spawnData: p.buffers[1] });
save('data.bin', p.read(0));
let threw = '';
try { p.logic = { source: spec.drift, uniforms: new ArrayBuffer(1025) }; p.step(); } catch (e) { threw = String(e); }
disposeProgram(drift); disposeProgram(data);
p.dispose();
console.log(JSON.stringify({ order, info, threw }));
"""


@pytest.mark.gpu
def test_drift_and_spawn_data_equal_the_python_host(tmp_path):
    from tendrils_amd import _capi
    from tendrils_amd.particles import Particles, Program

    class DriftU(C.Structure):
        _fields_ = [("k", C.c_float)]
    w, h, k = 50, 30, 0.75
    st = np.ascontiguousarray(hashed_state(50, 31, inert_mod=17)[:h])
    st[..., :2] = st[..., :2] * np.float32(0.75) + np.float32(0.5)         # uv values on both sides of the edges
    texture = np.ascontiguousarray(hashed_state(50, 32)[:h])
    # the Python host
    drift, data = Program.from_source(DRIFT, DriftU, name="drift"), Program.from_source(DATA, name="data")
    p = Particles(None, dict(shape=[w, h]))
    p.setup(3)
    p.upload_texels(st, 0)
    p.upload_texels(texture, 1)
    p.logic = drift
    p.step(dict(k=k))
    want_drift, want_order = p.read(0), [b.id for b in p.buffers]
    p.upload_texels(st, 0)
    p.logic = data
    p.step(dict(spawnData=p.buffers[1]))
    want_data = p.read(0)
    p.dispose(), drift.dispose(), data.dispose()
    assert (want_drift != st).any() and (want_data != st).any()
    # the Node host
    st.tofile(tmp_path / "state.bin")
    texture.tofile(tmp_path / "texture.bin")
    (tmp_path / "spec.json").write_text(json.dumps(dict(shape=[w, h], k=k, drift=DRIFT, data=DATA)))
    r = node(SCRIPT, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["order"] == want_order
    assert out["info"]["scratchBytes"] == 0 and out["info"]["vgprs"] > 0
    assert "1025" in out["threw"]
    assert bits_equal(np.fromfile(tmp_path / "drift.bin", np.float32).reshape(h, w, 4), want_drift).all()
    assert bits_equal(np.fromfile(tmp_path / "data.bin", np.float32).reshape(h, w, 4), want_data).all()
