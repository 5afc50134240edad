'use strict';
// Flow lines: strokes drawn into tendrils.flow - the reference's FlowLine / FlowLines (src/flow-line/index.js, multi.js)
// over the flow-lines addon (lib/tendrils_flow_lines.node: th_flow_line_attributes, th_flow_lines).  update() builds the
// strip's attributes; draw() draws the strip as of the last update() into the flow texture bound last
// (`tendrils.flow.bind()`) or into draw(target).  FlowLines.active is a plain object, so it iterates as the reference's
// does: integer ids ascending, then other ids in insertion order.
const path = require('path');

const addon = require(path.join(__dirname, '..', 'lib', 'tendrils_flow_lines.node'));

const defaults = () => ({                        // Line's defaults (src/geom/line/index.js:15-29) + FlowLine's
  color: [1, 1, 1, 1], rad: 0.1, viewSize: [1, 1], speed: 3, speedLimit: 0.01, crestShape: 0.6
});

let bound = null;
const bind = (flow) => { bound = flow; return flow; };

const handleOf = (target) => {
  const t = target || bound;
  if (!t) throw new Error('no flow texture bound: call tendrils.flow.bind() or pass draw(target)');
  if (!t.owner || !t.owner.particles) throw new Error("the flow texture's Tendrils has no particles (call setup() first)");
  return t.owner.particles.handle;
};

const packUniforms = (u) => new Float32Array([u.speed, u.rad, u.crestShape, u.speedLimit, u.viewSize[0], u.viewSize[1]]);

// One th_flow_lines call: lines = [{points: Float32Array, times: Float64Array, closed}] in draw order
function drawLines(handle, uniforms, lines) {
  let n = 0;
  for (const l of lines) n += l.times.length;
  const points = new Float32Array(2 * n), times = new Float64Array(n);
  const offsets = new Int32Array(lines.length + 1), closed = new Int32Array(lines.length);
  let at = 0;
  lines.forEach((l, i) => {
    points.set(l.points, 2 * at); times.set(l.times, at);
    at += l.times.length; offsets[i + 1] = at; closed[i] = l.closed ? 1 : 0;
  });
  addon.flowLines(handle, packUniforms(uniforms), points, times, lines.length ? offsets : new Int32Array(0), closed);
}

class Line {
  constructor(options = {}) {
    this.uniforms = options.uniforms || defaults();
    this.path = options.path || [];
    this.closed = !!options.closed;
    this.attributes = null;
    this.drawn = null;
  }

  update(times) {
    const n = this.path.length, points = new Float32Array(2 * n), t = new Float64Array(n);
    this.path.forEach((p, i) => { points[2 * i] = p[0]; points[2 * i + 1] = p[1]; t[i] = times[i]; });
    this.attributes = addon.flowLineAttributes(points, t, this.closed);
    this.drawn = { points, times: t, closed: this.closed };
    return this;
  }
}

class FlowLine {
  constructor(options = {}) {
    this.line = new Line(options);
    this.times = options.times || [];
  }

  update() { this.line.update(this.times); return this; }

  draw(target) {
    if (this.line.path.length > 0 && this.line.drawn) drawLines(handleOf(target), this.line.uniforms, [this.line.drawn]);
    return this;
  }

  add(time, point) { this.times.push(time); this.line.path.push(point); return this; }

  insert(time, point) {
    const index = this.findIndex(time);
    this.times.splice(index, 0, time);
    this.line.path.splice(index, 0, point);
    return this;
  }

  at(index, out = {}) { out.time = this.times[index]; out.point = this.line.path[index]; return out; }

  findIndex(time) {
    const next = this.times.findIndex((other) => other > time);
    return ((next < 0) ? this.times.length : next);
  }

  trim(ago, now = Date.now()) {
    const oldest = now - ago;
    while (this.times[0] < oldest) { this.times.shift(); this.line.path.shift(); }
    return this.length;
  }

  get length() { return this.times.length; }
}

class FlowLines {
  constructor() { this.active = {}; }

  get(id, options) { return (this.active[id] || (this.active[id] = new FlowLine(options))); }

  trim(...times) {
    let remaining = 0;
    for (const id of Object.keys(this.active)) {
      if (this.active[id].trim(...times) === 0) delete this.active[id];
      else ++remaining;
    }
    return remaining;
  }

  // update() (unless update === false) and draw() of every active line in order; consecutive lines with equal uniforms
  // share one th_flow_lines call
  draw(target, update = true) {
    const handle = handleOf(target);
    let run = [], key = null, uniforms = null;
    for (const id of Object.keys(this.active)) {
      const fl = this.active[id];
      if (update) fl.update();
      if (!fl.line.path.length || !fl.line.drawn) continue;
      const k = packUniforms(fl.line.uniforms).join(',');
      if (run.length && k !== key) { drawLines(handle, uniforms, run); run = []; }
      run.push(fl.line.drawn); key = k; uniforms = fl.line.uniforms;
    }
    if (run.length) drawLines(handle, uniforms, run);
    return this;
  }
}

module.exports = { FlowLine, FlowLines, Line, bind, defaults, drawLines };
