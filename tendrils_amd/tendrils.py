"""Host mirror of the reference's simulation facade `Tendrils` (src/index.js:84-457) for the
particle-update path: state uniforms, timer, flow/targets textures, step(), spawn(),
spawnShader(), resize(), and draw() = the flow pass + the view pass (the particles' lines with the
render shader's colours into an RGBA8 image of the drawing buffer: `view`, read with read_view()).
The demo's last pass - a shader of its own over the finished view (src/screen) - is screenShader() with a caller's
ScreenProgram; the reference's own blur shader is outside this build.  The constructor's flowShader / renderShader options
take a caller's DrawProgram - the vertex stage of the flow pass / the view pass of draw() -, a FragmentProgram - the fragment
stage, behind the library's vertex stage - or the reference's pair (vertex, fragment).
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import call
from .particles import (LOGIC, Follow, Particles, Program, ScreenProgram, StepProgram, deposit_uniforms, draw_program_args, draw_stages, run_pass,
                        shader_stages)
from .timer import Timer


def defaults():
    """src/index.js:28-75"""
    timer = Timer()
    timer.step = 1000 / 60
    return dict(
        state=dict(
            rootNum=2 ** 9,
            autoClearView=False, autoFade=True,
            damping=0.043, speedLimit=0.01,
            forceWeight=0.016, varyForce=-0.1,
            flowWeight=1, varyFlow=0.2,
            noiseWeight=0.002, varyNoise=0.3,
            flowDecay=0.005, flowWidth=5,
            noiseScale=2.125, varyNoiseScale=0.5,
            noiseSpeed=0.00025, varyNoiseSpeed=0.1,
            target=0, varyTarget=1,
            lineWidth=1, speedAlpha=0.000001, colorMapAlpha=0.4,
            baseColor=[1, 1, 1, 0.5], flowColor=[1, 1, 1, 0.04], fadeColor=[0.1333, 0.1333, 0.1333, 0]),
        timer=timer, numBuffers=0, logicShader=None, colorMap=None)


gl_settings = dict(preserveDrawingBuffer=True, antialias=True)     # src/index.js:77-80


def cover_aspect(size):
    """src/utils/aspect.js:4-11: scale(inverse(size), max(size))"""
    m = max(size[0], size[1])
    return [m / size[0], m / size[1]]


class View:
    """What the reference reads from its WebGL context: the drawing-buffer size."""

    def __init__(self, width, height):
        self.drawingBufferWidth = int(width)
        self.drawingBufferHeight = int(height)


class FlowTexture:
    """tendrils.flow (src/index.js:102): RGBA32F, NEAREST, CLAMP_TO_EDGE, resizable."""

    def __init__(self, owner):
        self._o = owner
        self._shape = [1, 1]

    @property
    def shape(self):
        return list(self._shape)

    @shape.setter
    def shape(self, wh):
        self._shape = [int(wh[0]), int(wh[1])]
        if self._o.particles is not None:
            call("th_flow_resize", self._o.particles._ctx, self._shape[0], self._shape[1])

    def set_pixels(self, texels):
        t = np.ascontiguousarray(texels, np.float32)
        assert t.shape == (self._shape[1], self._shape[0], 4), (t.shape, self._shape)
        call("th_flow_upload", self._o.particles._ctx, t.ctypes.data_as(_capi._fp))

    def read(self):
        out = np.empty((self._shape[1], self._shape[0], 4), np.float32)
        call("th_flow_download", self._o.particles._ctx, out.ctypes.data_as(_capi._fp))
        return out

    def clear(self):
        call("th_flow_clear", self._o.particles._ctx)

    def bind(self):
        """tendrils.flow.bind(): the target of the FlowLine / FlowLines draws that name none (tendrils_amd/flow_line.py)."""
        from . import flow_line
        return flow_line.bind(self)

    def source_index(self):
        return _capi.TH_SOURCE_FLOW


class ColorMap:
    """tendrils.colorMap (src/index.js:94-96): RGBA32F, a 1x1 zero texture until set.  The host copy `set_pixels` keeps
    (for a context made later) is dropped by whatever changes the map on the device: a Blend.draw into it, a new shape."""

    def __init__(self, owner):
        self._o = owner
        self._shape = [1, 1]
        self._pixels = None

    @property
    def shape(self):
        return list(self._shape)

    @shape.setter
    def shape(self, wh):                           # colorMap.shape = shape (src/demo.main.js:504): gl-fbo gives a new shape
        wh = [int(wh[0]), int(wh[1])]              # zeroed attachments and leaves the same shape alone
        if wh != self._shape:
            self._shape, self._pixels = wh, None
            self.bind_shape()

    def set_pixels(self, texels):
        t = np.ascontiguousarray(texels, np.float32)
        assert t.ndim == 3 and t.shape[2] == 4
        self._shape = [t.shape[1], t.shape[0]]
        self._pixels = t
        self.bind()

    def bind(self):
        if self._pixels is not None and self._o.particles is not None:
            call("th_colormap_upload", self._o.particles._ctx, self._pixels.ctypes.data_as(_capi._fp),
                 self._shape[0], self._shape[1])
        elif self._pixels is None:
            self.bind_shape()

    def bind_shape(self):
        """the device's map has this shape (a context made after the shape was set starts from a zeroed map of it)"""
        if self._o.particles is not None and self._shape != [1, 1]:
            call("th_colormap_resize", self._o.particles._ctx, self._shape[0], self._shape[1])

    def blended(self):
        """a pass on the device has written the map: the host copy is older than it"""
        self._pixels = None

    def read(self):
        """[h, w, 4] float32: the map as the device holds it"""
        out = np.empty((self._shape[1], self._shape[0], 4), np.float32)
        call("th_colormap_download", self._o.particles._ctx, out.ctypes.data_as(_capi._fp))
        return out


class TargetsTexture:
    """tendrils.targets (src/index.js:105,207): RGBA32F at the particle shape."""

    def __init__(self, owner):
        self._o = owner
        self.shape = [1, 1]

    def set_pixels(self, texels):
        t = np.ascontiguousarray(texels, np.float32)
        call("th_targets_upload", self._o.particles._ctx, t.ctypes.data_as(_capi._fp))

    def read(self):
        p = self._o.particles
        out = np.empty((p.shape[1], p.shape[0], 4), np.float32)
        call("th_targets_download", p._ctx, out.ctypes.data_as(_capi._fp))
        return out

    def clear(self):
        call("th_targets_clear", self._o.particles._ctx)

    def target_index(self):
        return _capi.TH_TARGET_TARGETS


def init_spawner(data, x=0, y=0):
    """src/spawn/init/cpu.js:3-8"""
    data[0] = data[1] = _capi.INERT
    data[2] = data[3] = 0
    return data


class ViewBuffer:
    """One of Tendrils.buffers (src/index.js:172-177: `FBO(gl, [1, 1])`, given viewRes by resize()): an off-screen RGBA8 view
    image on the device, addressed by its place in the owner's ring."""

    def __init__(self, owner):
        self._o = owner
        self.shape = [1, 1]

    def bind(self):
        self._o._bind_view(self)
        return self

    def read(self):
        """[viewRes.y, viewRes.x, 4] uint8"""
        return self._o.read_view(self)

    def dispose(self):
        self._o = None


class ScreenImage:
    """The drawing buffer itself (gl.bindFramebuffer(gl.FRAMEBUFFER, null)) as a texture a screen pass samples."""

    def __init__(self, owner):
        self._o = owner

    def bind(self):
        self._o._bind_view(None)
        return self

    def read(self):
        return self._o.read_view(None)


class Tendrils:
    def __init__(self, gl=None, options=None):
        params = {**defaults(), **(options or {})}
        self.gl = gl if gl is not None else View(1, 1)
        self.state = params["state"]
        self.particles = None
        self.flow = FlowTexture(self)
        self.targets = TargetsTexture(self)
        self.colorMap = params.get("colorMap") or ColorMap(self)
        self.renderView = bool(params.get("renderView", True))     # draw() also runs the view pass (as the reference's does)
        self.buffers = []
        self.screen = ScreenImage(self)
        self.logicShader = None
        self._logic_option = params.get("logicShader")         # new Tendrils(gl, { logicShader }): the caller's integrator
        # new Tendrils(gl, { flowShader, renderShader }) (src/index.js:70-71, 114-120): a caller's DrawProgram as the vertex stage
        # of the flow pass / the view pass of draw(); None = the library's own stage.  Assignable, as there.  Also: a
        # FragmentProgram (the fragment stage; the library's vertex stage) or the pair (vertex or None, fragment or None).
        self.flowShader = params.get("flowShader")
        self.renderShader = params.get("renderShader")
        # draw() with a fragment stage in either shader and renderView: both passes in ONE call (th_draw_stages_pair), over one
        # rasterisation of the lines where that gives the bits of the two passes run one after the other - else as those two.
        # Off (the default): a call per pass, as ever.  Assignable.  `rasterisations`: what the last such call ran, 1 or 2
        # (None: draw() has made no such call yet).
        self.pairedStages = bool(params.get("pairedStages", False))
        self.rasterisations = None
        self.uniforms = dict(render={}, update={})
        self.viewRes = [0, 0]
        self.viewSize = [0, 0]
        self.timer = params["timer"]
        self._device = int(params.get("device", 0))
        self._mode = int(params.get("mode", _capi.TH_MODE_EXACT))
        self._state_format = int(params.get("stateFormat", _capi.TH_STATE_F32))
        self._band = (int(params.get("row0", 0)), params.get("rows"), int(params.get("globalHeight", 0)))
        self.dist = params.get("dist")           # torch.distributed module of a row-band-sharded job (draw() exchanges)
        # what gl.getParameter(gl.ALIASED_LINE_WIDTH_RANGE) reports here: [1, 1] like the GL the reference was captured on
        # (flowWidth: 5 then draws width-1 lines, as it does there); up to [1, 64] for the picture of a GL that honours widths
        self.lineWidthRange = tuple(params.get("lineWidthRange", (1, 1)))
        self._bound = None                       # the bound view image: None = the screen, else one of self.buffers
        self.blending = False                    # gl.isEnabled(gl.BLEND): what step() / spawnShader() leave enabled (Blend.draw inherits it)
        self.setupBuffers(int(params.get("numBuffers", 0) or 0))      # src/index.js:109

    # -- setup ---------------------------------------------------------------------
    def setup(self, *rest):                                   # src/index.js:149-154
        self.setupParticles(*rest)
        self.reset()
        return self

    def reset(self):
        self.spawn()
        return self

    def dispose(self):
        if self.particles is not None:
            self.particles.dispose()
            self.particles = None
        return self

    # -- Tendrils.buffers: off-screen view images (src/index.js:172-184, 359-391) ----------------------------------------
    def setupBuffers(self, numBuffers=0):                      # src/index.js:172-184
        while len(self.buffers) < numBuffers:
            self.buffers.append(ViewBuffer(self))
        while len(self.buffers) > numBuffers:
            gone = self.buffers.pop()
            if self._bound is gone:
                self._bound = None                             # (the library leaves the screen bound as well)
            gone.dispose()
        if self.particles is not None:
            call("th_view_buffers", self.particles._ctx, len(self.buffers))
        return self

    def _bind_view(self, buffer=None):
        """gl.bindFramebuffer: None = the screen, else one of self.buffers"""
        self._bound = buffer
        if self.particles is not None:
            call("th_view_bind", self.particles._ctx, -1 if buffer is None else self.buffers.index(buffer))

    def drawBuffer(self, index=None):                          # src/index.js:359-367: a buffer's contents to the screen
        self._bind_view(None)
        if self.state["autoClearView"]:
            call("th_view_clear", self.particles._ctx)         # gl.clear of the bound framebuffer - the screen - alone
        return self.copyBuffer(0 if index is None else index).stepBuffers()      # (`undefined` takes copyBuffer's default)

    def copyBuffer(self, index=0):                             # src/index.js:370-383: into the current render target
        if 0 <= index < len(self.buffers):
            call("th_view_copy", self.particles._ctx, int(index))
        return self

    def stepBuffers(self):                                     # src/index.js:385-391
        if len(self.buffers) > 1:
            self.buffers.insert(0, self.buffers.pop())         # src/utils/index.js:1-7
            if self.particles is not None:
                call("th_view_step_buffers", self.particles._ctx)
        return self

    def screenShader(self, program, uniforms=None, views=(), target=None, blend=None):
        """Screen.render() with a caller's shader bound (src/screen/index.js; the demo's last pass, src/demo.main.js:1084-1102):
        `program` - a ScreenProgram - runs once per texel of `target`: None = the bound view image, tendrils.colorMap, or a
        texture slot (an int: the slot's RGBA32F / RGBA8 texture).  views: the texture units in order - one of self.buffers,
        self.screen, self.colorMap, self.flow, anything a Blend takes, or a texture slot (an int).  blend: gl.BLEND for this
        pass; None = what the passes before left (as Blend.draw)."""
        from .blend import resolve_view
        if not isinstance(program, ScreenProgram) or not program.handle:
            raise TypeError("screenShader: %r is no compiled ScreenProgram" % (program,))
        particles, views = self.particles, list(views)
        if len(views) > _capi.MAX_BLEND_VIEWS:
            raise ValueError("screenShader: at most %d views (got %d)" % (_capi.MAX_BLEND_VIEWS, len(views)))
        named = {int(v) for v in views + [target] if isinstance(v, (int, np.integer))}
        free = [k for k in range(_capi.MAX_TEXTURES) if k not in named]      # (audio textures travel in slots nobody named)
        table, slots = (_capi.ScreenUnit * max(1, len(views)))(), []
        for i, view in enumerate(views):
            if isinstance(view, (int, np.integer)):
                found = _capi.VIEW_TEXTURE, int(view)
                particles.textures[int(view)] = None           # (whatever audio texture the host thought it held)
            elif isinstance(view, ViewBuffer):
                found = _capi.VIEW_BUFFER, self.buffers.index(view)
            elif isinstance(view, ScreenImage):
                found = _capi.VIEW_SCREEN, 0
            elif isinstance(view, ColorMap):
                view.bind_shape()
                found = _capi.VIEW_COLORMAP, 0
            elif isinstance(view, FlowTexture):
                found = _capi.VIEW_FLOW, 0
            else:
                found = resolve_view(particles, view, slots, free)
            if found is None:
                raise TypeError("screenShader: view %d (%r) is nothing a screen pass samples" % (i, view))
            table[i].source, table[i].index = found
        if target is None:
            where, index = _capi.SCREEN_TARGET_VIEW, 0
        elif isinstance(target, ColorMap):
            target.bind_shape()
            where, index = _capi.SCREEN_TARGET_COLORMAP, 0
        elif isinstance(target, (int, np.integer)):
            where, index = _capi.SCREEN_TARGET_TEXTURE, int(target)
        else:
            raise TypeError("screenShader: target %r is neither None (the bound view image), the colorMap nor a texture slot" % (target,))
        block = program.pack(uniforms or {})
        blending = self.blending if blend is None else bool(blend)
        call("th_screen_run", particles._ctx, program.handle, None if block is None else C.byref(block),
             0 if block is None else C.sizeof(block), table, len(views), where, index, int(blending))
        if where == _capi.SCREEN_TARGET_COLORMAP:
            target.blended()
        elif where == _capi.SCREEN_TARGET_TEXTURE:
            particles.textures[index] = None
        return self

    def viewport(self):                                        # src/index.js:410-419: gl.viewport(0, 0, ...viewRes) - every pass
        return self                                            # here covers its whole target already

    def setupParticles(self, rootNum=None, numBuffers=2):     # src/index.js:186-210
        rootNum = self.state["rootNum"] if rootNum is None else rootNum
        self.state["rootNum"] = rootNum
        row0, rows, gh = self._band
        shape = [rootNum, rows if rows else rootNum]
        if self.particles is not None:
            self.particles.dispose()
        self.particles = Particles(self.gl, dict(
            shape=shape, geomShape=[shape[0], shape[1] * 2], logic=Program(LOGIC),
            device=self._device, mode=self._mode, stateFormat=self._state_format, row0=row0,
            globalHeight=(gh if gh else (rootNum if rows else 0))))
        self.logicShader = self._logic_option or self.particles.logic
        self.particles.setup(numBuffers)
        self.targets.shape = shape
        self.flow.shape = self.flow.shape          # (re)create on the new context
        if isinstance(self.colorMap, ColorMap):
            self.colorMap._o = self
            self.colorMap.bind()
        call("th_line_width_range", self.particles._ctx, float(self.lineWidthRange[0]), float(self.lineWidthRange[1]))
        self._bound = None                       # (a new context: its screen is bound, its ring is empty)
        if self.buffers:
            call("th_view_buffers", self.particles._ctx, len(self.buffers))
        return self

    def line_widths(self):
        """gl.lineWidth(Math.max(0, flowWidth)) before the flow pass, gl.lineWidth(Math.max(0, lineWidth)) before the view
        pass (src/index.js:302,336); a width of 0 is GL's INVALID_VALUE: the width of that pass stays what it was."""
        flow, view = max(0.0, float(self.state["flowWidth"])), max(0.0, float(self.state["lineWidth"]))
        if flow > 0:
            call("th_line_width", self.particles._ctx, _capi.TH_PASS_FLOW, flow)
        if view > 0:
            call("th_line_width", self.particles._ctx, _capi.TH_PASS_VIEW, view)

    # -- clears ---------------------------------------------------------------------
    def clear(self):
        self.clearView()
        self.clearFlow()
        return self

    def clearView(self):                                       # src/index.js:220-229: every buffer, then the screen -
        for b in self.buffers:                                 # which it leaves bound
            self._bind_view(b)
            call("th_view_clear", self.particles._ctx)
        self._bind_view(None)
        call("th_view_clear", self.particles._ctx)
        return self

    def drawFade(self):                                        # src/index.js:342-348
        if self.state["fadeColor"][3] > 0:
            self.drawFill(self.state["fadeColor"])
        return self

    def drawFill(self, color=None):                            # src/index.js:350-356
        col = (C.c_float * 4)(*[float(v) for v in (self.state["fadeColor"] if color is None else color)])
        call("th_view_fill", self.particles._ctx, col)
        return self

    def render_uniforms(self):
        """The view pass's uniforms (src/index.js:284-293 over `state`); sin(time*flowDecay) is evaluated here - as the
        shader would, in fp32 operands - because GLSL leaves its value to the implementation."""
        s = self.state
        u = _capi.RenderUniforms(time=float(self.timer.time), speedLimit=float(s["speedLimit"]), flowDecay=float(s["flowDecay"]),
                                 speedAlpha=float(s["speedAlpha"]), colorMapAlpha=float(s["colorMapAlpha"]))
        u.sinTerm = math.sin(float(np.float32(self.timer.time)) * float(np.float32(s["flowDecay"])))
        u.viewSize[0], u.viewSize[1] = float(self.viewSize[0]), float(self.viewSize[1])
        for k in range(4):
            u.baseColor[k], u.flowColor[k] = float(s["baseColor"][k]), float(s["flowColor"][k])
        return u

    def read_view(self, buffer=None):
        """The screen image - or one of self.buffers -: [viewRes.y, viewRes.x, 4] uint8 (readPixels order).  What is bound
        stays bound."""
        out = np.empty((self.viewRes[1], self.viewRes[0], 4), np.uint8)
        was = self._bound
        if was is not buffer:
            self._bind_view(buffer)
        call("th_view_download", self.particles._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        if was is not buffer:
            self._bind_view(was)
        return out

    def clearFlow(self):                                       # src/index.js:231-236
        self.flow.clear()
        return self

    def restart(self):
        self.clear()
        self.reset()
        return self

    # -- the hot path ------------------------------------------------------------------
    def step(self):                                            # src/index.js:248-272
        if not self.timer.paused:
            self.particles.logic = self.logicShader
            self.uniforms["update"].update(self.state)
            self.uniforms["update"].update(
                dt=self.timer.dt, time=self.timer.time, start=self.timer.since,
                flow=self.flow, targets=self.targets,
                viewSize=self.viewSize, viewRes=self.viewRes)
            self._key_step_program()
            self.particles.step(self.uniforms["update"])
            self.blending = True                                # src/index.js:267-268
        return self

    def _key_step_program(self):
        """a StepProgram logicShader taps the flow field through this viewSize, like the built-in integrator: its calls may
        keep the slots sorted by it (Particles.step_view_size)"""
        if self.logicShader.kind == StepProgram.SOURCE_KIND:
            sized = all(math.isfinite(v) and v > 0 for v in self.viewSize)          # ([0, 0] until the first resize(): no key)
            self.particles.step_view_size(self.viewSize if sized else None)

    def step_n(self, n):
        """n x (timer.tick(); step()) for a fixed-step, unpaused timer, as one captured-graph replay - of a StepProgram
        logicShader: as one th_step_program_run, its steps fused."""
        tm = self.timer
        if tm.paused or tm.step < 0 or tm.end >= 0 or self.logicShader.kind not in (LOGIC, StepProgram.SOURCE_KIND):
            for _ in range(n):
                tm.tick()
                self.step()
            return self
        self.particles.logic = self.logicShader
        dt = tm.step * tm.rate
        self.uniforms["update"].update(self.state)
        self.uniforms["update"].update(dt=dt, time=tm.time, start=tm.since, flow=self.flow, targets=self.targets,
                                       viewSize=self.viewSize, viewRes=self.viewRes)
        self._key_step_program()
        self.particles.step_n(self.uniforms["update"], tm.time, dt, n)
        self.blending = self.blending or n > 0
        for _ in range(n):
            tm.tick()
        return self

    def draw(self):                                            # src/index.js:278-340
        """The flow pass - particle lines into the flow texture, so that particles respond to each other's wake - and,
        with renderView, the view pass: the same lines into the RGBA8 view buffer (after the clear / fade the state
        asks for).  Each pass runs the stages of its shader - flowShader / renderShader: a fragment stage (th_draw_stages_run:
        stream-ordered, or with particles.option("stage_bins", 1) the pipeline of the pass without it - a stage that reads th_line(f) with
        particles.option("line_bins", 1) beside it), else a vertex program (th_draw_program_run), else the library's own stage; both passes with the
        library's stages draw the same lines, and one call rasterises and sorts them once (th_draw) when they draw them with
        the same width - and so does, with self.pairedStages on, a draw() with a fragment stage in either shader
        (th_draw_stages_pair: _draw_stages_pair has the conditions).  Programs get draw_program_uniforms(), packed into each program's uniform block by field name.  A
        program pass takes the pipeline the library's own pass of this context would (Particles.draw_pipeline / TH_DRAW: binned
        where the shape and the ring allow it, else stream-ordered - include/tendrils_hip.h "draw programs"); through the bins
        a tile-sorted ring stays sorted, so step(); draw() keeps it."""
        self.line_widths()
        view = self.renderView
        programs = any(stage is not None for stage in shader_stages(self.flowShader) + shader_stages(self.renderShader))
        if self._sharded():
            # a row band: the passes go through the owners' exchange - the host's, of a torch.distributed job, or the library's
            # own over the communicator the ranks joined with sharding.comm_init() (th_draw_sharded / th_draw_program_sharded;
            # what the Node host runs); every rank calls draw() together.  Every rank holds the whole view buffer: the bind, the
            # clear and the fade are the same everywhere, and come first
            from . import sharding
            if view:
                self._view_prologue()
            if programs:
                self.fragments, self.view_fragments = sharding.draw_sharded_programs(self.dist, self, view=view)
                return self
            self.fragments = sharding.draw_sharded(self.dist, self, view=view) if self.dist is not None else sharding.draw_sharded_native(self, view=view)
            self.view_fragments = self.fragments if view else 0
            return self
        if view and not programs:
            # (the clear and the fade only touch the view buffer: it does not matter that the flow pass comes after them here)
            self._view_prologue()
            d, u, n = self.deposit_uniforms(), self.render_uniforms(), C.c_uint64(0)
            call("th_draw", self.particles._ctx, C.byref(d), C.byref(u), C.byref(n))
            self.fragments = self.view_fragments = int(n.value)
            return self
        uniforms = self.draw_program_uniforms() if programs else None
        if view and self.pairedStages and (shader_stages(self.flowShader)[1] is not None or shader_stages(self.renderShader)[1] is not None):
            # (the clear and the fade only touch the view buffer, and no stage reads it: in front of both passes, as for th_draw)
            self._view_prologue()
            self.fragments, self.view_fragments = self._draw_stages_pair(uniforms)
            return self
        self.fragments = self._draw_pass(_capi.TH_PASS_FLOW, self.flowShader, uniforms)
        if view:
            self._view_prologue()
            self.view_fragments = self._draw_pass(_capi.TH_PASS_VIEW, self.renderShader, uniforms)
        return self

    def _view_prologue(self):
        """what comes in front of the view pass: the view goes to buffers[0] when there are buffers, else to the screen
        (src/index.js:318-325) - unless autoClearView comes in between: clearView() leaves the SCREEN bound (src/index.js:226),
        there as here - then the fade"""
        self._bind_view(self.buffers[0] if self.buffers else None)
        if self.state["autoClearView"]:
            self.clearView()
        if self.state["autoFade"]:
            self.drawFade()

    def _draw_pass(self, which, shader, uniforms):
        """one pass of a whole texture with the stages of `shader`; returns its fragments"""
        vertex, fragment = shader_stages(shader)
        if fragment is not None:
            return self._draw_stages(vertex, fragment, which, uniforms)
        if vertex is not None:
            return self._draw_program(vertex, which, uniforms)
        if which == _capi.TH_PASS_FLOW:
            return self.particles.deposit_flow(self.viewSize, self.timer.time, self.state["speedLimit"])
        u, n = self.render_uniforms(), C.c_uint64(0)
        call("th_view_draw", self.particles._ctx, C.byref(u), C.byref(n))
        return int(n.value)

    def _draw_program(self, program, which, uniforms):
        args, _keep = draw_program_args(program, uniforms)
        n = C.c_uint64(0)
        call("th_draw_program_run", self.particles._ctx, *args, which, C.byref(n))
        return int(n.value)

    def _draw_stages(self, vertex, fragment, which, uniforms):
        """one pass with a caller's fragment stage behind `vertex` (a DrawProgram; None: the library's vertex stage):
        th_draw_stages_run.  By default such a pass is stream-ordered under every policy and takes the ring to texel order;
        with particles.option("stage_bins", 1) (TH_STAGE_BINS) it takes the pipeline the same pass without the fragment stage
        would - through the bins the stage runs over the page store between the emit and the blends, and a tile-sorted ring
        stays sorted.  A fragment program that reads th_line(f) stays stream-ordered under that switch unless
        particles.option("line_bins", 1) (TH_LINE_BINS) is on beside it: then its line records lie beside the page store's places.
        The bits are the same either way."""
        builtin = self.render_uniforms() if which == _capi.TH_PASS_VIEW else self.deposit_uniforms()
        stages, _keep = draw_stages(vertex, fragment, uniforms, builtin)
        n = C.c_uint64(0)
        call("th_draw_stages_run", self.particles._ctx, C.byref(stages), which, C.byref(n))
        return int(n.value)

    def _draw_stages_pair(self, uniforms):
        """both passes with the stages of flowShader and renderShader in one call, th_draw_stages_pair (pairedStages): the bits of
        the two passes one after the other; ONE rasterisation when neither shader has a vertex program, both passes draw equally
        wide lines, no fragment program reads th_line(f) and renderShader's does not name th_flow - run in sequence the view
        pass's th_flow would see the field after the flow pass has blended into it, in one rasterisation every stage runs before
        anything blends.  self.rasterisations says which it was.  Returns (fragments, view_fragments)."""
        flow, _keep_flow = draw_stages(*shader_stages(self.flowShader), uniforms, self.deposit_uniforms())
        view, _keep_view = draw_stages(*shader_stages(self.renderShader), uniforms, self.render_uniforms())
        n, ran = C.c_uint64(0), C.c_int32(0)
        call("th_draw_stages_pair", self.particles._ctx, C.byref(flow), C.byref(view), C.byref(n), C.byref(ran))
        self.rasterisations = int(ran.value)
        if self.rasterisations == 1:
            return int(n.value), int(n.value)
        info = _capi.DrawInfo()                     # (two passes: the call reports the flow pass's fragments, the query the view pass's)
        call("th_draw_query", self.particles._ctx, C.byref(info))
        return int(n.value), int(info.fragments)

    def deposit_uniforms(self):
        """the library's flow stage's uniforms of this frame (th_deposit_uniforms)"""
        return deposit_uniforms(self.viewSize, self.timer.time, self.state["speedLimit"])

    def _sharded(self):
        """this context is a row-band shard: of a torch.distributed job, or a band narrower than the texture"""
        row0, rows, gh = self._band
        return self.dist is not None or bool(rows and rows != (gh or self.state["rootNum"]))

    def draw_program_uniforms(self):
        """what draw() hands a flowShader / renderShader, on one GPU and on a row band alike (src/index.js:284-293): the state,
        time, viewSize, viewRes, colorMapRes - and dataRes, geomRes (src/particles.js:149-155) of the WHOLE particle texture -
        with self.uniforms["render"] on top; each program's block is packed from it by field name"""
        p = self.particles
        height = self._band[2] or p.shape[1]
        whole = height != p.shape[1]
        uniforms = dict(self.state, time=float(self.timer.time), viewSize=self.viewSize, viewRes=self.viewRes,
                        dataRes=[p.shape[0], height] if whole else p.shape,
                        geomRes=[p.shape[0], 2 * height] if whole else p.geomShape, colorMapRes=self.colorMap.shape)
        uniforms.update(self.uniforms["render"])
        return uniforms

    def export_lines(self, view=False):
        """Trail export: the (previous -> current) line list this frame's draw() is made of (build-defined): [n, 12]
        float32 - p0.xy, p1.xy (clip space), then both vertices' flow varyings, or (view=True) their view colours."""
        if not view:
            return self.particles.export_lines(self.viewSize, self.timer.time, self.state["speedLimit"])
        u = self.render_uniforms()
        n = C.c_uint64(0)
        call("th_export_view_lines", self.particles._ctx, C.byref(u), None, 0, C.byref(n))
        out = np.empty((int(n.value), 12), np.float32)
        if n.value:
            call("th_export_view_lines", self.particles._ctx, C.byref(u), out.ctypes.data_as(_capi._fp), n.value, C.byref(n))
        return out

    def resize(self):                                          # src/index.js:393-408
        self.viewRes[0] = self.gl.drawingBufferWidth
        self.viewRes[1] = self.gl.drawingBufferHeight
        self.viewSize[:] = cover_aspect(self.viewRes)
        for b in self.buffers:                                 # src/index.js:404 (the images follow the flow texture's shape)
            b.shape = list(self.viewRes)
        self.flow.shape = self.viewRes
        return self

    # -- respawn --------------------------------------------------------------------------
    def spawn(self, spawner=init_spawner):                     # src/index.js:425-429
        if spawner is init_spawner:
            # Particles.spawn(initSpawner) fills every ring buffer with inert texels; do it on device
            for k in range(len(self.particles.buffers)):
                call("th_spawn_init", self.particles._ctx, k)
        else:
            self.particles.spawn(spawner)
        return self

    def spawnShader(self, shader, update=None, *rest):         # src/index.js:432-457
        self.timer.tick()                                       # every GPU spawn advances time
        self.particles.logic = shader
        base = dict(self.state, time=self.timer.time, viewSize=self.viewSize, viewRes=self.viewRes)
        self.particles.step(Particles.applyUpdate(base, update), *rest)
        self.particles.logic = self.logicShader
        self.blending = True                                    # src/index.js:453-454
        return self

    def measure(self, program, uniforms=None):
        """A MeasureProgram's reduction over the particles' current state (Particles.measure of buffers[0]): its uniform block
        is filled from tendrils.state, time, viewSize and viewRes under `uniforms`, as spawnShader fills a pass's.  Read-only:
        no tick, no step - the next draw() is the one it would have been."""
        base = dict(self.state, time=self.timer.time, viewSize=self.viewSize, viewRes=self.viewRes)
        return self.particles.measure(program, Particles.applyUpdate(base, uniforms))

    def density(self, shape=None, slot=0, into="texture"):
        """The particles' count and summed velocity on a grid over the view (Particles.density of buffers[0]) under the view size
        step() hands the integrator; shape: (w, h) of the grid, the flow's by default - a cell is then the flow texel the
        particle taps.  Read-only, as measure()."""
        w, h = self.flow.shape if shape is None else shape
        return self.particles.density(w, h, self.viewSize, slot=slot, into=into)

    def select(self, **kw):
        """The particles that match a box, a band of speeds, a thinning (Particles.select, its arguments; buffers[0] by
        default): a Selection, its records in texel order.  Read-only, as measure()."""
        return self.particles.select(**kw)

    def histogram(self, channel, bins, range, **kw):
        """How a scalar of the state is distributed over the matching particles (Particles.histogram, its arguments;
        buffers[0] by default): a Histogram.  Read-only, as select()."""
        return self.particles.histogram(channel, bins, range, **kw)

    def quantiles(self, channel, q, **kw):
        """Exact order statistics of a scalar of the state over the matching particles (Particles.quantiles, its arguments):
        the median speed, the 95th percentile to normalise a ramp to.  Read-only, as select()."""
        return self.particles.quantiles(channel, q, **kw)

    def follow(self, indices, depth=64):
        """Follow the particles at texels `indices` - a Selection's .index, say - from sample to sample in a history on the
        device (Particles.follow): a TimedFollow, whose sample() takes its time from tendrils.timer unless told one.  Nothing samples
        by itself - step(); follow.sample(); draw() - and sampling is read-only, as select()."""
        return TimedFollow(self.particles, indices, depth, self.timer)


class TimedFollow(Follow):
    """What Tendrils.follow returns: a Follow whose sample() takes `time` from the tendrils' timer when it is given none"""

    def __init__(self, particles, indices, depth, timer):
        self.timer = timer
        super().__init__(particles, indices, depth)

    def sample(self, time=None, buffer=0):
        super().sample(self.timer.time if time is None else time, buffer)


default = Tendrils
