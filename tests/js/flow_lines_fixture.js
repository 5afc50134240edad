'use strict';
// Draws flow lines through the Node host (tendrils_amd/js/flow-line.js) for tests/test_gpu_flow_line.py.
// Usage: node flow_lines_fixture.js <job.json> <initial flow .npy (f32 [h, w, 4])> <out: raw f32>
const fs = require('fs');
const path = require('path');

const root = path.join(__dirname, '..', '..');
const T = require(path.join(root, 'tendrils_amd', 'js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const npy = fs.readFileSync(process.argv[3]);
const hlen = npy.readUInt16LE(8);
const base = new Float32Array(npy.buffer.slice(npy.byteOffset + 10 + hlen, npy.byteOffset + npy.length));

const t = new T.Tendrils({ drawingBufferWidth: job.w, drawingBufferHeight: job.h }, {});
t.resize();
t.setup(16);
t.flow.shape = [job.w, job.h];
t.flow.setPixels(base);
t.flow.bind();
const lines = new T.FlowLines();
for (const l of job.lines) {
  const fl = lines.get(l.id, { closed: l.closed });
  l.points.forEach((p, i) => fl.add(l.times[i], p));
}
const order = Object.keys(lines.active);
if (JSON.stringify(order) !== JSON.stringify(job.lines.map((l) => String(l.id)))) throw new Error('draw order ' + order);
for (const fl of Object.values(lines.active)) {
  Object.assign(fl.line.uniforms, job.uniforms);
  fl.update().draw();
}
const out = t.flow.read();
fs.writeFileSync(process.argv[4], Buffer.from(out.buffer, out.byteOffset, out.byteLength));
t.dispose && t.dispose();
