"""Host mirror of the demo's colour-map blend: `Blend` (src/screen/blend/index.js) and the `AudioTexture`s it sums
(src/audio/data-texture.js, src/audio/utils.js).  Every frame, before tendrils.step().draw(), the demo runs
blend.draw(tendrils.colorMap) (src/demo.main.js:541-560, 1068-1079): one pass over the colour map on the device
(th_colormap_blend), whose views are textures the context already holds - the optical-flow frames, the image spawner's buffer
- and the audio data textures, a few hundred bytes uploaded per frame (th_texture_upload).  Nothing is read back.

    track = AudioTexture(None, analyser_bins)
    blend = Blend(None, dict(views=[track, track, optical_flow.frame(0)], alphas=[0.1, 0.3, 0.8]))
    each frame:  track.frequencies(analyser_bytes).apply();  blend.draw(tendrils.colorMap);  tendrils.step().draw()
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import call
from .particles import Density
from .spawn.pixels import ImageBuffer, PixelSpawner


def waveform_map(v):
    """src/audio/utils.js:1-2: (v - 128) * (1 / 128), in the Float32Array the reference maps into"""
    return ((np.asarray(v, np.float64) - 128.0) * (1.0 / 128.0)).astype(np.float32)


def frequency_map(v):
    """src/audio/utils.js:4-5: v * (1 / 256)"""
    return (np.asarray(v, np.float64) * (1.0 / 256.0)).astype(np.float32)


class AudioTexture:
    """src/audio/data-texture.js: a Float32Array of n bins behind an n x 1 one-channel float texture (sampled as
    (L, L, L, 1)).  assign() / waveform() / frequencies() map analyser data into `array`; apply() is texture.setPixels(array):
    the texture holds what the array held THEN.  The texels travel to the device when a blend next uses the texture."""

    def __init__(self, gl=None, array=None):
        self.gl = gl
        if isinstance(array, (int, np.integer)):
            self.array = np.zeros(int(array), np.float32)
        else:
            self.array = np.array(array, np.float32).reshape(-1)
        assert self.array.size > 0, "an AudioTexture needs at least one bin"
        self.texture = self                       # (the reference hands `audioTexture.texture` to Blend.views: both name this object)
        self.shape = [int(self.array.size), 1]
        self._texels = self.array.copy()          # makeTexture(gl, array): the texture starts from the array
        self._version = 0

    def apply(self, array=None):
        src = self.array if array is None else np.asarray(array, np.float32).reshape(-1)
        assert src.size == self.array.size, (src.size, self.array.size)
        self._texels = src.astype(np.float32, copy=True)
        self._version += 1
        return self

    def _map(self, fn, data):
        src = self.array if data is None else np.asarray(data).reshape(-1)
        n = min(src.size, self.array.size)        # mapList writes the source's elements over the array's
        self.array[:n] = fn(src[:n])
        return self

    def assign(self, data=None):
        return self._map(lambda v: np.asarray(v, np.float32), data)

    def waveform(self, data=None):
        return self._map(waveform_map, data)

    def frequencies(self, data=None):
        return self._map(frequency_map, data)

    def read(self, particles, slot):
        """the texels of `slot` as the device holds them (tests)"""
        out = np.empty(self.array.size, np.float32)
        call("th_texture_download", particles._ctx, int(slot), out.ctypes.data_as(C.c_void_p))
        return out


class FrameView:
    """One of OpticalFlow.buffers as a blend's view (`video: opticalFlow.buffers[0]`, src/demo.main.js:552): the frame texture
    with this identity, wherever OpticalFlow.step() has rotated it to since."""

    def __init__(self, optical_flow, identity):
        self.optical_flow = optical_flow
        self.identity = identity

    def index(self):
        return self.optical_flow.buffers.index(self.identity)


class Blend:
    """src/screen/blend/index.js: `views` summed into a target, each with its alpha of `alphas`.  A view is an AudioTexture
    (or its .texture), an OpticalFlow frame (optical_flow.frame(k)), or the image spawner's buffer (a PixelSpawner, its
    .buffer - an ImageBuffer - or .buffer.color[0]), or a Density (what Particles.density returned: the texture slot or the
    spawn image it filled; the audio textures of the draw then travel in the other slots).  The only target is a Tendrils' colorMap."""

    def __init__(self, gl=None, options=None, views=None, alphas=None, resolution=None):
        params = dict(views=[], alphas=[], resolution=[1, 1])
        params.update(options or {})
        self.gl = gl
        self.views = list(params["views"] if views is None else views)
        self.alphas = list(params["alphas"] if alphas is None else alphas)
        self.resolution = list(params["resolution"] if resolution is None else resolution)
        self.uniforms = {}

    def draw(self, target, resolution=None, clear=True, gl_blend=None):
        """Blend.draw(target, resolution = target.shape, clear = true).  The reference leaves the GL's blend state as it
        finds it: what Tendrils.step() / spawnShader() last left enabled (SRC_ALPHA, ONE_MINUS_SRC_ALPHA), nothing before
        the first of them - `gl_blend` overrides what the target's Tendrils has tracked."""
        from .tendrils import ColorMap
        if not isinstance(target, ColorMap) or target._o is None or target._o.particles is None:
            raise TypeError("Blend.draw: the target is the colorMap of a Tendrils that has been set up")
        tendrils = target._o
        particles = tendrils.particles
        shape = target.shape
        if resolution is not None and [int(resolution[0]), int(resolution[1])] != shape:
            raise ValueError("Blend.draw: resolution %r is not the target's shape %r" % (list(resolution), shape))
        self.resolution = shape
        n = len(self.views)
        if len(self.alphas) < n:
            raise ValueError("Blend.draw: %d views but %d alphas" % (n, len(self.alphas)))
        if not 1 <= n <= _capi.MAX_BLEND_VIEWS:
            raise ValueError("Blend.draw: 1..%d views (got %d)" % (_capi.MAX_BLEND_VIEWS, n))
        table = (_capi.BlendView * n)()
        slots = []                                # the distinct audio textures of this draw, in order of appearance
        taken = {v.slot for v in self.views if isinstance(v, Density) and v.into == "texture"}
        free = [k for k in range(_capi.MAX_TEXTURES) if k not in taken]
        for i, view in enumerate(self.views):
            found = resolve_view(particles, view, slots, free)
            if found is None:
                raise TypeError("Blend.draw: view %d (%r) is no AudioTexture, OpticalFlow frame or image buffer" % (i, view))
            table[i].source, table[i].index = found
            table[i].alpha = float(self.alphas[i])
        target.bind_shape()
        blending = tendrils.blending if gl_blend is None else bool(gl_blend)
        call("th_colormap_blend", particles._ctx, table, n, int(blending), int(bool(clear)))
        target.blended()
        return self


def resolve_view(particles, view, slots, free=range(_capi.MAX_TEXTURES)):
    """(TH_VIEW_* source, index) of one of the views a host hands to a pass over textures - an AudioTexture (or its .texture),
    an OpticalFlow frame, the image spawner's buffer (a PixelSpawner, its .buffer or .buffer.color[0]) - or None for anything
    else.  `slots`: the distinct audio textures of this pass so far, in order of appearance; the k-th of them travels in
    texture slot free[k]."""
    if isinstance(view, Density):
        return (_capi.VIEW_TEXTURE, view.slot) if view.into == "texture" else (_capi.VIEW_SPAWN_IMAGE, 0)
    view = getattr(view, "texture", view)
    if isinstance(view, PixelSpawner):
        view = view.buffer
    if isinstance(view, AudioTexture):
        if not any(view is s for s in slots):
            slots.append(view)
            _upload(particles, free[len(slots) - 1], view)
        return _capi.VIEW_TEXTURE, free[[view is s for s in slots].index(True)]
    if isinstance(view, FrameView):
        return _capi.VIEW_FRAMES, view.index()
    if isinstance(view, ImageBuffer):
        view.bind_for(particles)
        return _capi.VIEW_SPAWN_IMAGE, 0
    return None


def _upload(particles, slot, texture):
    """texture slot `slot` of the context holds `texture` as of its last apply(): upload when it does not"""
    held = particles.textures
    if held[slot] is None or held[slot][0] is not texture or held[slot][1] != texture._version:
        t = texture._texels
        call("th_texture_upload", particles._ctx, slot, _capi.TEX_L32F, t.ctypes.data_as(C.c_void_p), int(t.size), 1)
        held[slot] = (texture, texture._version)


default = Blend
