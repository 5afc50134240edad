'use strict';
// Mirror of the demo's colour-map blend: `Blend` (src/screen/blend/index.js) and the `AudioTexture`s it sums
// (src/audio/data-texture.js, src/audio/utils.js), over the blend addon (lib/tendrils_blend.node: th_texture_upload,
// th_colormap_resize / _blend / _download).  Every frame, before tendrils.step().draw(), the demo runs
// blend.draw(tendrils.colorMap) (src/demo.main.js:541-560, 1068-1079): here one pass over the colour map on the device, whose
// views are textures the context already holds - the optical-flow frames, the image spawner's buffer - and the audio data
// textures, a few hundred bytes uploaded per frame.  Nothing is read back.
//
//   const track = new AudioTexture(null, analyser.frequencyBinCount);
//   const map = new ColorMap(tendrils);  map.shape = [w, h];
//   const blend = new Blend(null, { views: [track.texture, track.texture, opticalFlow.buffers[0]], alphas: [0.1, 0.3, 0.8] });
//   each frame:  track.frequencies(bytes).apply();  blend.draw(map);  tendrils.step().draw();
const path = require('path');

const addon = require(path.join(__dirname, '..', 'lib', 'tendrils_blend.node'));
const { ImageBuffer, PixelSpawner } = require('./spawn/pixels');

const waveformMap = (v) => (v - 128) * (1 / 128);   // src/audio/utils.js:1-2
const frequencyMap = (v) => v * (1 / 256);          // src/audio/utils.js:4-5

// src/audio/data-texture.js: a Float32Array of n bins behind an n x 1 one-channel float texture (sampled as (L, L, L, 1)).
// assign() / waveform() / frequencies() map analyser data into `array`; apply() is texture.setPixels(array): the texture
// holds what the array held THEN.  The texels travel to the device when a blend next uses the texture.
class AudioTexture {
  constructor(gl, array) {
    this.gl = gl;
    this.array = (typeof array === 'number') ? new Float32Array(array) : Float32Array.from(array);
    if (!this.array.length) throw new Error('an AudioTexture needs at least one bin');
    this.texture = this;                           // (the reference hands `audioTexture.texture` to Blend.views: both name this object)
    this.shape = [this.array.length, 1];
    this.texels = Float32Array.from(this.array);   // makeTexture(gl, array): the texture starts from the array
    this.version = 0;
  }

  apply(array = this.array) {
    if (array.length !== this.array.length) throw new Error(`AudioTexture.apply: ${array.length} values for ${this.array.length} bins`);
    this.texels = Float32Array.from(array);
    ++this.version;
    return this;
  }

  map(fn, data = this.array) {                     // mapList: the source's elements over the array's
    const n = Math.min(data.length, this.array.length);
    for (let k = 0; k < n; ++k) this.array[k] = fn(data[k]);
    return this;
  }

  assign(data) { return this.map((v) => v, data); }
  waveform(data) { return this.map(waveformMap, data); }
  frequencies(data) { return this.map(frequencyMap, data); }
}

// tendrils.colorMap as the device holds it (src/index.js:94-96: a 1 x 1 float FBO until someone gives it a shape): the
// target of Blend.draw.  `shape = [w, h]` is the demo's colorMap.shape = shape (src/demo.main.js:504): a new shape gives a
// zero-filled map, the same shape nothing.
class ColorMap {
  constructor(tendrils) { this.tendrils = tendrils; }
  get handle() { return this.tendrils.particles.handle; }
  get shape() { return addon.colormapShape(this.handle); }
  set shape(wh) {
    const was = this.shape;
    if (was[0] === (wh[0] | 0) && was[1] === (wh[1] | 0)) return;
    addon.colormapResize(this.handle, wh[0] | 0, wh[1] | 0);
    this.tendrils.colorMap = null;                 // (the host copy setColorMap kept is not this map's any more)
  }
  read() { return addon.colormapDownload(this.handle); }     // Float32Array, w x h RGBA32F
}

// texture slot `slot` of the context holds `texture` as of its last apply(): upload when it does not
function upload(particles, slot, texture) {
  const held = (particles.textures || (particles.textures = new Array(addon.MAX_TEXTURES).fill(null)));
  if (!held[slot] || held[slot].texture !== texture || held[slot].version !== texture.version) {
    addon.textureUpload(particles.handle, slot, addon.TEX_L32F, texture.texels, texture.texels.length, 1);
    held[slot] = { texture, version: texture.version };
  }
}

// src/screen/blend/index.js: `views` summed into a target, each with its alpha of `alphas`.  A view is an AudioTexture (or
// its .texture), one of OpticalFlow.buffers (the frame texture with that identity, wherever step() has rotated it to), or the
// image spawner's buffer (a PixelSpawner, its .buffer or .buffer.color[0]).  The only target is a ColorMap.
class Blend {
  constructor(gl, options) {
    const params = Object.assign({ views: [], alphas: [], resolution: [1, 1] }, options);
    this.gl = gl;
    this.views = params.views;
    this.alphas = params.alphas;
    this.resolution = params.resolution;
    this.uniforms = {};
  }

  // Blend.draw(target, resolution = target.shape, clear = true).  The reference leaves the GL's blend state as it finds it:
  // what Tendrils.step() / spawnShader() last left enabled (SRC_ALPHA, ONE_MINUS_SRC_ALPHA), nothing before the first of
  // them - `glBlend` overrides what the target's Tendrils has tracked.
  draw(target, resolution, clear = true, glBlend) {
    if (!(target instanceof ColorMap) || !target.tendrils.particles) throw new TypeError('Blend.draw: the target is the ColorMap of a Tendrils that has been set up');
    const tendrils = target.tendrils, particles = tendrils.particles, shape = target.shape;
    if (resolution && ((resolution[0] | 0) !== shape[0] || (resolution[1] | 0) !== shape[1])) throw new RangeError(`Blend.draw: resolution ${resolution} is not the target's shape ${shape}`);
    this.resolution = shape;
    const n = this.views.length;
    if (this.alphas.length < n) throw new RangeError(`Blend.draw: ${n} views but ${this.alphas.length} alphas`);
    if (n < 1 || n > addon.MAX_BLEND_VIEWS) throw new RangeError(`Blend.draw: 1..${addon.MAX_BLEND_VIEWS} views (got ${n})`);
    const pairs = new Int32Array(2 * n), slots = [];
    this.views.forEach((v, i) => {
      let view = (v && v.texture) || v;
      if (view instanceof PixelSpawner) view = view.buffer;
      if (view instanceof AudioTexture) {
        if (slots.indexOf(view) < 0) { slots.push(view); upload(particles, slots.length - 1, view); }
        pairs[2 * i] = addon.VIEW_TEXTURE; pairs[2 * i + 1] = slots.indexOf(view);
      } else if (view && view.opticalFlow && view.opticalFlow.buffers.indexOf(view) >= 0) {
        pairs[2 * i] = addon.VIEW_FRAMES; pairs[2 * i + 1] = view.opticalFlow.buffers.indexOf(view);
      } else if (view instanceof ImageBuffer) {
        view.bindFor(particles);
        pairs[2 * i] = addon.VIEW_SPAWN_IMAGE;
      } else throw new TypeError(`Blend.draw: view ${i} is no AudioTexture, OpticalFlow frame or image buffer`);
    });
    const blending = (glBlend === undefined) ? !!tendrils.blending : !!glBlend;
    addon.colormapBlend(particles.handle, pairs, Float32Array.from(this.alphas.slice(0, n)), blending, !!clear);
    tendrils.colorMap = null;                      // (a host copy setColorMap kept is older than the device's map now)
    return this;
  }
}

module.exports = { AudioTexture, Blend, ColorMap, waveformMap, frequencyMap, default: Blend };
