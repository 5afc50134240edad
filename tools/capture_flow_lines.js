/*
 * Capture harness for flow lines (used by tools/capture_flow_lines.py only; never by the tests or the library).
 *
 * Appended, in a temporary copy, after the reference's compiled demo bundle whose bootstrap hands out its module loader
 * instead of starting the app: window.Tendrils is then the bundle's `require`.  The harness finds the compiled FlowLine
 * and FlowLines modules by their text and drives the reference's own classes; nothing here restates their arithmetic.
 *
 * job: {kind:'flowline', flowW, flowH, flow: b64 f32 [H*W*4] | null, uniforms: {...},
 *       lines: [{id, closed, points: [[x, y]...], times: [...]}...], trim: [ago, now] | null}
 * Lines are created through FlowLines.get(id, {closed}) in the order given; every point through FlowLine.add().  After
 * the optional FlowLines.trim(ago, now), every line of `active` (in the object's own iteration order) gets the uniforms,
 * update() and draw() into an RGBA32F framebuffer of the flow's shape, blending SRC_ALPHA / ONE_MINUS_SRC_ALPHA as
 * Tendrils.step() leaves it.  Returns the draw order, every drawn line's attribute arrays and the framebuffer.
 */
(function () {
  function findModule(req, needles) {
    var ids = Object.keys(req.m), hit = [];
    for (var i = 0; i < ids.length; ++i) {
      var src = Function.prototype.toString.call(req.m[ids[i]]), ok = true;
      for (var k = 0; k < needles.length; ++k) if (src.indexOf(needles[k]) < 0) { ok = false; break; }
      if (ok) hit.push(ids[i]);
    }
    if (hit.length !== 1) throw new Error('module lookup ' + JSON.stringify(needles) + ' matched ' + hit.length);
    return req(+hit[0]);
  }
  function b64ToBytes(s) {
    var bin = atob(s), n = bin.length, out = new Uint8Array(n);
    for (var i = 0; i < n; ++i) out[i] = bin.charCodeAt(i);
    return out;
  }
  function bytesToB64(u8) {
    var parts = [], CH = 0x8000;
    for (var i = 0; i < u8.length; i += CH)
      parts.push(String.fromCharCode.apply(null, u8.subarray(i, Math.min(i + CH, u8.length))));
    return btoa(parts.join(''));
  }
  function f32ToB64(f) { return bytesToB64(new Uint8Array(f.buffer, f.byteOffset, f.byteLength)); }

  function runFlowLine(job) {
    var req = window.Tendrils;
    if (typeof req !== 'function' || !req.m) throw new Error('the bundle did not hand out its module loader');
    var FlowLineMod = findModule(req, ['crestShape:.6', 'findIndex', 'setAttributes']);
    var FlowLinesMod = findModule(req, ['this.active={}', 'trim']);
    var FlowLines = FlowLinesMod.FlowLines || FlowLinesMod.default;
    if (!FlowLineMod.FlowLine) throw new Error('FlowLine module has no FlowLine export');

    var W = job.flowW, H = job.flowH, c = document.createElement('canvas');
    c.width = W; c.height = H;
    var gl = c.getContext('webgl', {preserveDrawingBuffer: true, antialias: false, alpha: true, premultipliedAlpha: false});
    if (!gl || !gl.getExtension('OES_texture_float')) throw new Error('no float webgl');
    gl.getExtension('WEBGL_color_buffer_float');
    var floatBlend = !!gl.getExtension('EXT_float_blend');

    var tex = gl.createTexture();
    gl.bindTexture(gl.TEXTURE_2D, tex);
    gl.texParameteri(gl.TEXTURE_2D, gl.TEXTURE_MIN_FILTER, gl.NEAREST);
    gl.texParameteri(gl.TEXTURE_2D, gl.TEXTURE_MAG_FILTER, gl.NEAREST);
    gl.texParameteri(gl.TEXTURE_2D, gl.TEXTURE_WRAP_S, gl.CLAMP_TO_EDGE);
    gl.texParameteri(gl.TEXTURE_2D, gl.TEXTURE_WRAP_T, gl.CLAMP_TO_EDGE);
    var init = job.flow ? new Float32Array(b64ToBytes(job.flow).buffer) : new Float32Array(4 * W * H);
    gl.texImage2D(gl.TEXTURE_2D, 0, gl.RGBA, W, H, 0, gl.RGBA, gl.FLOAT, init);
    var fbo = gl.createFramebuffer();
    gl.bindFramebuffer(gl.FRAMEBUFFER, fbo);
    gl.framebufferTexture2D(gl.FRAMEBUFFER, gl.COLOR_ATTACHMENT0, gl.TEXTURE_2D, tex, 0);
    if (gl.checkFramebufferStatus(gl.FRAMEBUFFER) !== gl.FRAMEBUFFER_COMPLETE) throw new Error('float framebuffer incomplete');

    var lines = new FlowLines(gl);
    for (var i = 0; i < job.lines.length; ++i) {
      var L = job.lines[i], fl = lines.get(L.id, {closed: !!L.closed});
      for (var p = 0; p < L.points.length; ++p) fl.add(L.times[p], new Float32Array(L.points[p]));
    }
    if (job.trim) lines.trim(job.trim[0], job.trim[1]);

    gl.disable(gl.DEPTH_TEST);
    gl.disable(gl.CULL_FACE);
    gl.enable(gl.BLEND);
    gl.blendFunc(gl.SRC_ALPHA, gl.ONE_MINUS_SRC_ALPHA);
    var order = [], attrs = [], names = ['position', 'normal', 'miter', 'previous', 'time', 'dt'];
    for (var id in lines.active) {
      var line = lines.active[id];
      Object.assign(line.line.uniforms, job.uniforms);
      line.update();
      gl.bindFramebuffer(gl.FRAMEBUFFER, fbo);
      gl.viewport(0, 0, W, H);
      line.draw();
      order.push(id);
      var a = {length: line.length};
      for (var k = 0; k < names.length; ++k) a[names[k]] = f32ToB64(line.line.attributes[names[k]].data);
      attrs.push(a);
    }
    gl.bindFramebuffer(gl.FRAMEBUFFER, fbo);
    var out = new Float32Array(4 * W * H);
    gl.readPixels(0, 0, W, H, gl.RGBA, gl.FLOAT, out);
    return {order: order, attrs: attrs, out: f32ToB64(out), floatBlend: floatBlend,
            samples: gl.getParameter(gl.SAMPLES), err: gl.getError()};
  }

  window.Plotly = {
    version: '2.0.0',
    toImage: function (fig) {
      var res;
      try {
        var job = fig.layout.job;
        if (job.kind === 'flowline') res = runFlowLine(job);
        else res = {error: 'unknown job kind'};
      } catch (e) {
        res = {error: String(e), stack: e && e.stack};
      }
      return Promise.resolve(JSON.stringify(res));
    }
  };
})();
