/*
 * Capture harness for the colour-map blend (used by tools/capture_blend.py only; never by the tests or the library).
 *
 * Appended, in a temporary copy, after the reference's compiled demo bundle whose bootstrap hands out its module loader
 * instead of starting the app: window.Tendrils is then the bundle's `require`.  The harness finds the compiled Blend,
 * AudioTexture and gl-fbo modules by their text and drives the reference's own objects; nothing here restates their
 * arithmetic.
 *
 * job: {kind:'blend', targetW, targetH, alphas: [...], glBlend: bool, clear: bool, prefill: b64 f32 [H*W*4] | null,
 *       textures: [{type:'audio', n, map:'frequencies'|'waveform'|'assign', data: b64 u8 [n] | b64 f32 [n] (assign)} |
 *                  {type:'rgba8', w, h, data: b64 u8 [h*w*4]} | {type:'rgba32f', w, h, data: b64 f32 [h*w*4]}...],
 *       views: [index into textures...]}
 * An audio texture is the reference's AudioTexture(gl, n) filled through its own waveform() / frequencies() / assign() and
 * apply(); the other two are gl-fbo objects (non-float / {float: true}) whose colour attachment receives the texels.  The
 * target is a float gl-fbo of the target's shape.  With glBlend the GL state is what Tendrils.step() leaves behind
 * (BLEND enabled, SRC_ALPHA / ONE_MINUS_SRC_ALPHA), else the context's initial state.  Then Blend.draw(target, undefined,
 * clear).  Returns the target read back as floats and every audio texture's float array as the reference mapped it.
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

  function runBlend(job) {
    var req = window.Tendrils;
    if (typeof req !== 'function' || !req.m) throw new Error('the bundle did not hand out its module loader');
    var BlendMod = findModule(req, ['alphas:this.alphas', 't.Blend=']);
    var AudioMod = findModule(req, ['t.AudioTexture=void 0']);
    var FBO = findModule(req, ['gl-fbo: Missing shape parameter']);
    var Blend = BlendMod.Blend || BlendMod.default, AudioTexture = AudioMod.AudioTexture || AudioMod.default;

    var W = job.targetW, H = job.targetH, c = document.createElement('canvas');
    c.width = W; c.height = H;
    var gl = c.getContext('webgl', {preserveDrawingBuffer: true, antialias: false, alpha: true, premultipliedAlpha: false});
    if (!gl || !gl.getExtension('OES_texture_float')) throw new Error('no float webgl');
    gl.getExtension('WEBGL_color_buffer_float');
    var floatBlend = !!gl.getExtension('EXT_float_blend');

    var made = [], arrays = [], shapes = [];
    for (var i = 0; i < job.textures.length; ++i) {
      var t = job.textures[i];
      if (t.type === 'audio') {
        var at = new AudioTexture(gl, t.n);
        if (t.map === 'assign') at.assign(new Float32Array(b64ToBytes(t.data).buffer));
        else at[t.map](b64ToBytes(t.data));
        at.apply();
        made.push(at.texture);
        arrays.push(f32ToB64(at.array.data));
        shapes.push(at.texture.shape.slice());
      } else {
        var f = FBO(gl, [t.w, t.h], t.type === 'rgba32f' ? {float: true} : {});
        gl.bindTexture(gl.TEXTURE_2D, f.color[0].handle);
        if (t.type === 'rgba32f')
          gl.texImage2D(gl.TEXTURE_2D, 0, gl.RGBA, t.w, t.h, 0, gl.RGBA, gl.FLOAT, new Float32Array(b64ToBytes(t.data).buffer));
        else
          gl.texImage2D(gl.TEXTURE_2D, 0, gl.RGBA, t.w, t.h, 0, gl.RGBA, gl.UNSIGNED_BYTE, b64ToBytes(t.data));
        made.push(f);
        arrays.push(null);
        shapes.push(f.shape.slice());
      }
    }
    var target = FBO(gl, [W, H], {float: true});
    if (job.prefill) {
      gl.bindTexture(gl.TEXTURE_2D, target.color[0].handle);
      gl.texImage2D(gl.TEXTURE_2D, 0, gl.RGBA, W, H, 0, gl.RGBA, gl.FLOAT, new Float32Array(b64ToBytes(job.prefill).buffer));
    }
    gl.bindFramebuffer(gl.FRAMEBUFFER, null);

    var views = [];
    for (var v = 0; v < job.views.length; ++v) views.push(made[job.views[v]]);
    var blend = new Blend(gl, {views: views, alphas: job.alphas.slice()});

    if (job.glBlend) {          // what Tendrils.step() ends with (src/index.js:267-268)
      gl.enable(gl.BLEND);
      gl.blendFunc(gl.SRC_ALPHA, gl.ONE_MINUS_SRC_ALPHA);
    }
    blend.draw(target, undefined, !!job.clear);

    target.bind();
    var out = new Float32Array(4 * W * H);
    gl.readPixels(0, 0, W, H, gl.RGBA, gl.FLOAT, out);
    return {out: f32ToB64(out), arrays: arrays, shapes: shapes, floatBlend: floatBlend, resolution: blend.resolution.slice(),
            blendEnabled: gl.isEnabled(gl.BLEND), err: gl.getError()};
  }

  window.Plotly = {
    version: '2.0.0',
    toImage: function (fig) {
      var res;
      try {
        var job = fig.layout.job;
        if (job.kind === 'blend') res = runBlend(job);
        else res = {error: 'unknown job kind'};
      } catch (e) {
        res = {error: String(e), stack: e && e.stack};
      }
      return Promise.resolve(JSON.stringify(res));
    }
  };
})();
