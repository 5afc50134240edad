"""The colour-map blend through the Node host (tendrils_amd/js/blend.js over the addon of th_napi_blend.cc): the addon loads
without a GPU and exports what it says, the AudioTexture maps equal the reference's, and on the GPU the demo's two frames -
the first draw() before any step(), the second after one - equal the captures blend_first_frame_24x16 and blend_demo_24x16
bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, bits_equal, load

NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
ADDON = os.path.join(ROOT, "tendrils_amd", "lib", "tendrils_blend.node")


def node(script, *args):
    return subprocess.run([NODE, "-e", script, *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_addon_loads_without_a_gpu_and_the_audio_maps_are_the_references():
    if not os.path.exists(ADDON):
        import __graft_entry__ as g
        g.build()
    fx = load(os.path.join(GOLDEN, "blend_demo_24x16.npz"))
    r = node("""
    const a = require('./tendrils_amd/lib/tendrils_blend.node');
    const { AudioTexture, Blend } = require('./tendrils_amd/js/blend');
    const spec = JSON.parse(process.argv[1]);
    const mic = new AudioTexture(null, 8).frequencies(Uint8Array.from(spec.raw0));
    const held = Array.from(mic.texels);
    mic.apply();
    const track = new AudioTexture(null, Float32Array.from(spec.raw1)).waveform().apply();
    const blend = new Blend(null, { views: [mic.texture], alphas: [1] });
    let threw = '';
    try { blend.draw({}); } catch (e) { threw = String(e); }
    console.log(JSON.stringify({ keys: Object.getOwnPropertyNames(a).sort(), mic: Array.from(mic.texels), track: Array.from(track.texels),
                                 held, shape: track.shape, resolution: blend.resolution, threw }));
    """, json.dumps(dict(raw0=fx["raw0"].tolist(), raw1=fx["raw1"].tolist())))
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["keys"] == ["MAX_BLEND_VIEWS", "MAX_TEXTURES", "TEX_L32F", "TEX_RGBA32F", "TEX_RGBA8", "VIEW_FRAMES", "VIEW_SPAWN_IMAGE",
                           "VIEW_TEXTURE", "colormapBlend", "colormapDownload", "colormapResize", "colormapShape", "textureUpload"]
    assert bits_equal(np.array(out["mic"], np.float32), fx["tex0"]).all()
    assert bits_equal(np.array(out["track"], np.float32), fx["tex1"]).all()
    assert not any(out["held"]) and out["shape"] == [16, 1] and out["resolution"] == [1, 1]
    assert "TypeError" in out["threw"]


SCRIPT = """
const fs = require('fs'), path = require('path');
const { Tendrils } = require('./tendrils_amd/js');
const { OpticalFlow } = require('./tendrils_amd/js/optical-flow');
const { AudioTexture, Blend, ColorMap } = require('./tendrils_amd/js/blend');
const dir = process.argv[1], spec = JSON.parse(fs.readFileSync(path.join(dir, 'spec.json'), 'utf8'));
const save = (name, arr) => fs.writeFileSync(path.join(dir, name), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
const t = new Tendrils({ drawingBufferWidth: 16, drawingBufferHeight: 9 });
t.resize();
t.setup(8);
const mic = new AudioTexture(null, 8), track = new AudioTexture(null, 16);
const opticalFlow = new OpticalFlow(t);
opticalFlow.resize([12, 10]);
opticalFlow.setPixels(Uint8Array.from(spec.video));
const blend = new Blend(null, { views: [mic.texture, track.texture, opticalFlow.buffers[0]], alphas: [0.1, 0.3, 0.8] });
const map = new ColorMap(t);
const shapes = [map.shape];
map.shape = [24, 16];
shapes.push(map.shape);
const blending = [];
for (let frame = 0; frame < 2; ++frame) {
  mic.frequencies(Uint8Array.from(spec.raw0)).apply();
  track.waveform(Uint8Array.from(spec.raw1)).apply();
  blending.push(t.blending);
  blend.draw(map);
  save(`frame${frame}.bin`, map.read());
  t.timer.tick();
  t.step();
}
opticalFlow.step();                                // the frame's identity follows the rotation
blend.draw(map, undefined, true, false);
save('override.bin', map.read());
let threw = '';
try { new Blend(null, { views: new Array(9).fill(mic), alphas: new Array(9).fill(0.1) }).draw(map); } catch (e) { threw = String(e); }
t.dispose();
console.log(JSON.stringify({ shapes, blending, resolution: blend.resolution, threw }));
"""


@pytest.mark.gpu
def test_the_demos_two_frames_equal_the_captures(tmp_path):
    first = load(os.path.join(GOLDEN, "blend_first_frame_24x16.npz"))
    demo = load(os.path.join(GOLDEN, "blend_demo_24x16.npz"))
    (tmp_path / "spec.json").write_text(json.dumps(dict(raw0=demo["raw0"].tolist(), raw1=demo["raw1"].tolist(),
                                                        video=demo["tex2"].reshape(-1).tolist())))
    r = node(SCRIPT, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["shapes"] == [[1, 1], [24, 16]] and out["blending"] == [False, True] and out["resolution"] == [24, 16]
    assert "views" in out["threw"]

    def frame(name):
        return np.fromfile(tmp_path / name, np.float32).reshape(16, 24, 4)
    assert bits_equal(frame("frame0.bin"), first["out"]).all()
    assert bits_equal(frame("frame1.bin"), demo["out"]).all()
    assert bits_equal(frame("override.bin"), first["out"]).all()
