"""Host mirror of the reference's GPGPU core `Particles` (src/particles.js:43-196).

Same constructor options, fields and methods; the FBO ring, the full-screen logic
pass and the spawn upload are backed by the HIP library through the C ABI
(_capi.py).  `logic` is an opaque program object naming the kernel a pass runs
(the reference swaps shader objects: src/index.js:250,435,451).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import call


def defaults():
    """src/particles.js:30-41"""
    return dict(shape=[64, 64], geomShape=None,
                logic=None, logicVert=None, logicFrag=None,
                render=None, renderVert=None, renderFrag=None)


class Program:
    """Stand-in for a compiled gl-shader object: names a kernel family - or, from_source(), holds a pass the caller wrote."""

    COMPILE, SOURCE_KIND = "th_program_compile", "user"       # what from_source() compiles with, and into which kind

    def __init__(self, kind, **fixed):
        self.kind = kind          # 'logic' | 'spawn-init' | 'spawn-ball' | 'spawn-sample' | 'spawn-direct' | 'user'
        self.fixed = fixed        # compile-time constants of that shader (e.g. samples, apply)
        self.uniforms = {}
        self.handle = None        # 'user': the compiled th_program
        self.uniforms_struct = None

    @classmethod
    def from_source(cls, source, uniforms_struct=None, name="user_program"):
        """A user program (include/tendrils_hip.h "user programs"): HIP source defining
        `__device__ float4 th_main(const th_pass &p)`, compiled here, once, for gfx950 - no GPU needed.  uniforms_struct: the
        ctypes.Structure that mirrors the struct the source reads through th_uniforms<T>(p) (at most 1024 bytes); a pass
        fills it by field name from its uniforms.  A source that does not compile raises TendrilsHipError with the
        compiler's output (the caller's own line numbers, under `name`)."""
        if uniforms_struct is not None and C.sizeof(uniforms_struct) > 1024:
            raise ValueError("a uniform block holds at most 1024 bytes (%d)" % C.sizeof(uniforms_struct))
        lib = _capi.load()
        handle = C.c_void_p()
        status = getattr(lib, cls.COMPILE)(source.encode(), name.encode(), C.byref(handle))
        if status != _capi.TH_OK:
            raise _capi.TendrilsHipError(status, lib.th_last_error().decode(errors="replace") + "\n" +
                                         lib.th_program_log().decode(errors="replace"))
        prog = cls(cls.SOURCE_KIND, name=name)
        prog.handle, prog.uniforms_struct = handle, uniforms_struct
        return prog

    def pack(self, uniforms):
        """the uniform block of one pass: every field of uniforms_struct the dict names (gl.uniform*: the others stay zero)"""
        if self.uniforms_struct is None:
            return None
        block = self.uniforms_struct()
        for field in self.uniforms_struct._fields_:
            name, ctype = field[0], field[1]
            if name not in uniforms:
                continue
            value = uniforms[name]
            if issubclass(ctype, C.Array):
                array = getattr(block, name)
                for k, v in enumerate(np.asarray(value).reshape(-1)[:len(array)]):
                    array[k] = v.item()
            else:
                setattr(block, name, value.item() if isinstance(value, np.generic) else value)
        return block

    def query(self, particles):
        """registers, LDS, scratch (non-zero: the program spills) and code bytes of the kernel as `particles` loaded it"""
        info = _capi.ProgramInfo()
        call("th_program_query", particles._ctx, self.handle, C.byref(info))
        return {k: getattr(info, k) for k, _ in _capi.ProgramInfo._fields_ if k != "reserved"}

    def bind(self):
        return self

    def dispose(self):
        if self.handle:
            call("th_program_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass


class ScreenProgram(Program):
    """A screen program (include/tendrils_hip.h "screen programs"): from_source() takes HIP source defining
    `__device__ float4 th_screen(const th_screen_pass &s)` - the shader of one Screen.render() - and is otherwise
    Program.from_source: compiled once, for gfx950, no GPU needed; TendrilsHipError with the compiler's output; pack(),
    query() and dispose() as there.  Tendrils.screenShader() runs it."""
    COMPILE, SOURCE_KIND = "th_screen_program_compile", "screen"


class DrawProgram(Program):
    """A draw program (include/tendrils_hip.h "draw programs"): from_source() takes HIP source defining
    `__device__ th_vertex th_vertex_main(const th_vertex_pass &v)` - the vertex shader of one pass of draw() - and is otherwise
    Program.from_source: compiled once, for gfx950, no GPU needed; TendrilsHipError with the compiler's output; pack(),
    query() and dispose() as there.  Tendrils runs it as its flowShader / renderShader, through the draw() pipeline the
    library's own pass would take (Particles.draw_pipeline): the binned one leaves a tile-sorted ring in its slot order."""
    COMPILE, SOURCE_KIND = "th_draw_program_compile", "draw"


class FragmentProgram(Program):
    """A fragment program (include/tendrils_hip.h "fragment programs"): from_source() takes HIP source defining
    `__device__ float4 th_fragment_main(const th_fragment_pass &f)` - the fragment shader of one pass of draw(), called once per
    fragment with its window texel and the interpolated varying; what it returns is blended - and is otherwise
    Program.from_source: compiled once, for gfx950, no GPU needed; TendrilsHipError with the compiler's output; pack(), query()
    and dispose() as there.  Tendrils runs it as the second of a flowShader / renderShader pair (or alone: with the library's
    vertex stage); such a pass is stream-ordered unless Particles.option("stage_bins", 1) sends it through the bins.  A source
    that names th_line reads the fragment's line (th_line(f): line, along, across, length): nothing to pass here - the library
    sees it when it compiles, writes the records such a pass needs, and keeps the pass stream-ordered - unless
    Particles.option("line_bins", 1) is on beside "stage_bins": then such a pass goes through the bins too."""
    COMPILE, SOURCE_KIND = "th_fragment_program_compile", "fragment"


def shader_stages(shader):
    """(vertex, fragment) of a flowShader / renderShader: None, a DrawProgram (the vertex stage), a FragmentProgram (the fragment
    stage, with the library's vertex stage) or the reference's pair [vert, frag] (src/index.js:70-71), either of which may be None"""
    if shader is None:
        return None, None
    if isinstance(shader, FragmentProgram):
        return None, shader
    if isinstance(shader, (tuple, list)):
        if len(shader) != 2:
            raise TypeError("draw: a shader pair is (vertex, fragment): %r" % (shader,))
        vertex, fragment = shader
    else:
        vertex, fragment = shader, None
    if vertex is not None and (not isinstance(vertex, DrawProgram) or not vertex.handle):
        raise TypeError("draw: %r is no compiled DrawProgram" % (vertex,))
    if fragment is not None and (not isinstance(fragment, FragmentProgram) or not fragment.handle):
        raise TypeError("draw: %r is no compiled FragmentProgram" % (fragment,))
    return vertex, fragment


def program_block(program, uniforms):
    """(the program's handle, its uniform block packed by field name from `uniforms` - None: it has none -, the block's size):
    how every draw call hands a program over; the caller keeps the block alive across the call"""
    block = program.pack(uniforms)
    return program.handle, block, (0 if block is None else C.sizeof(block))


def draw_program_args(program, uniforms):
    """((program, uniforms, uniform_bytes) as th_draw_program_run / _emit / _sharded take a DrawProgram, its block - to be kept
    alive across the call)"""
    if not isinstance(program, DrawProgram) or not program.handle:
        raise TypeError("draw: %r is no compiled DrawProgram" % (program,))
    handle, block, size = program_block(program, uniforms)
    return (handle, None if block is None else C.byref(block), size), block


def draw_stages(vertex, fragment, uniforms, builtin):
    """(th_draw_stages, what it points to - to be kept alive across the call) of one pass: each program's block packed by field
    name from `uniforms`; `builtin`: the library's vertex-stage uniforms (a ctypes structure), read when vertex is None"""
    stages, keep = _capi.DrawStages(), [builtin]
    for slot, program in (("vertex", vertex), ("fragment", fragment)):
        if program is None:
            continue
        handle, block, size = program_block(program, uniforms)
        keep.append(block)
        setattr(stages, slot, handle)
        if block is not None:
            setattr(stages, slot + "_uniforms", C.cast(C.pointer(block), C.c_void_p))
            setattr(stages, slot + "_uniform_bytes", size)
    if vertex is None:
        stages.builtin = C.cast(C.pointer(builtin), C.c_void_p)
    return stages, keep


def deposit_uniforms(view_size, time, speed_limit):
    """th_deposit_uniforms: what the library's flow stage takes of a frame - the one place that builds them"""
    u = _capi.DepositUniforms(time=float(time), speedLimit=float(speed_limit))
    u.viewSize[0], u.viewSize[1] = float(view_size[0]), float(view_size[1])
    return u


class StepProgram(Program):
    """A step program (include/tendrils_hip.h "step programs"): from_source() takes HIP source defining
    `__device__ float4 th_step_main(const th_step_pass &s)` - one step of one particle's integrator, which reads nothing of the
    ring but its own texel (there is no th_particles) - and is otherwise Program.from_source: compiled once, for gfx950, no GPU
    needed; TendrilsHipError with the compiler's output; pack(), query() and dispose() as there.  Tendrils runs it as its
    logicShader: step() one step of it, step_n() n steps fused in one launch, with the same bits and the same ring order."""
    COMPILE, SOURCE_KIND = "th_step_program_compile", "step"


class MeasureProgram(Program):
    """A measure program (include/tendrils_hip.h "measure programs"): from_source() takes HIP source defining
    `__device__ th_sample th_measure_main(const th_measure_pass &m)` - what one particle contributes to up to `channels`
    (1 .. 8) numbers, or th_no_sample() - and is otherwise Program.from_source: compiled once, for gfx950, no GPU needed;
    TendrilsHipError with the compiler's output; pack(), query() and dispose() as there.  Particles.measure() reduces it over a
    ring buffer - per channel the sum, the minimum and the maximum, and the count of samples taken - and reads nothing back but
    the 144-byte result; nothing of the context changes."""
    COMPILE, SOURCE_KIND = "th_measure_program_compile", "measure"

    @classmethod
    def from_source(cls, source, uniforms_struct=None, channels=1, name="measure_program"):
        if uniforms_struct is not None and C.sizeof(uniforms_struct) > 1024:
            raise ValueError("a uniform block holds at most 1024 bytes (%d)" % C.sizeof(uniforms_struct))
        lib = _capi.load()
        handle = C.c_void_p()
        status = lib.th_measure_program_compile(source.encode(), name.encode(), int(channels), C.byref(handle))
        if status != _capi.TH_OK:
            raise _capi.TendrilsHipError(status, lib.th_last_error().decode(errors="replace") + "\n" +
                                         lib.th_program_log().decode(errors="replace"))
        prog = cls(cls.SOURCE_KIND, name=name, channels=int(channels))
        prog.handle, prog.uniforms_struct = handle, uniforms_struct
        return prog

    @property
    def channels(self):
        return self.fixed["channels"]


class Measure:
    """What Particles.measure returns: taken (samples), particles (texels measured), and per channel sum (float64), min, max
    (float32) - numpy arrays of the program's `channels`"""

    def __init__(self, result, channels):
        self.taken, self.particles = int(result.taken), int(result.particles)
        self.sum = np.array(result.sum[:channels], np.float64)
        self.min = np.array(result.min[:channels], np.float32)
        self.max = np.array(result.max[:channels], np.float32)
        self.raw = bytes(result)

    def __repr__(self):
        return "Measure(taken=%d, particles=%d, sum=%r, min=%r, max=%r)" % (self.taken, self.particles, self.sum, self.min, self.max)


class Density:
    """What Particles.density returns: particles, live, inside, outside, nonfinite_velocity (th_density_info), and where the
    image lies - read() downloads its h x w x 4 float texels (count, summed velocity x, y, occupied)"""

    def __init__(self, particles, info, w, h, into, slot):
        for k, _ in _capi.DensityInfo._fields_:
            setattr(self, k, int(getattr(info, k)))
        self.shape, self.into, self.slot = (int(w), int(h)), into, int(slot)
        self._p = particles

    def read(self):
        out = np.empty((self.shape[1], self.shape[0], 4), np.float32)
        if self.into == "texture":
            call("th_texture_download", self._p._ctx, self.slot, out.ctypes.data_as(C.c_void_p))
        else:
            call("th_spawn_image_download", self._p._ctx, out.ctypes.data_as(_capi._fp))
        return out

    def __repr__(self):
        return "Density(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k, _ in _capi.DensityInfo._fields_)


SELECTED = np.dtype([("state", np.float32, 4), ("index", np.uint32), ("x", np.uint32), ("y", np.uint32), ("reserved", np.uint32)])
assert SELECTED.itemsize == C.sizeof(_capi.Selected)


class Selection:
    """What Particles.select returns: the matching particles in increasing texel - index, x, y (uint32 arrays, in the whole
    texture) and state ([written, 4] float32, as decoded) - and particles, live, matched, written (th_select_info)"""

    def __init__(self, info, records):
        for k, _ in _capi.SelectInfo._fields_:
            setattr(self, k, int(getattr(info, k)))
        records = records[:self.written]
        self.index, self.x, self.y = (np.ascontiguousarray(records[k]) for k in ("index", "x", "y"))
        self.state = np.ascontiguousarray(records["state"]).reshape(-1, 4)

    def __len__(self):
        return self.written

    def __repr__(self):
        return "Selection(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k, _ in _capi.SelectInfo._fields_)


HIST_CHANNELS = dict(x=_capi.HIST_X, y=_capi.HIST_Y, vx=_capi.HIST_VX, vy=_capi.HIST_VY, speed2=_capi.HIST_SPEED2, speed=_capi.HIST_SPEED)
QUANTILE_PASSES = ((2048, 21), (2048, 10), (1024, 0))      # (bins, key_shift): 11, 11 and 10 bits of the key, from the top


class Histogram:
    """What Particles.histogram returns: counts (uint32, one per bin), edges (bins + 1 float64 values, for plotting only: the
    library bins in float32 by its own expression), and below, above, nan, matched, live, particles (th_histogram_info):
    below + counts.sum() + above + nan == matched"""

    def __init__(self, info, counts, lo, hi):
        for k, _ in _capi.HistogramInfo._fields_:
            setattr(self, k, int(getattr(info, k)))
        self.counts = counts
        self.edges = np.linspace(float(lo), float(hi), len(counts) + 1)

    def __repr__(self):
        return "Histogram(bins=%d, %s)" % (len(self.counts), ", ".join("%s=%d" % (k, getattr(self, k)) for k, _ in _capi.HistogramInfo._fields_))


def float_key(values):
    """the monotone integer key of float32 values (th_histogram's TH_HIST_KEY): its order is the floats', -0.0 just below +0.0"""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(key):
    """... and the float32 a key stands for"""
    key = np.asarray(key, np.uint32)
    return np.where(key >> 31, key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


class FollowCounts:
    """th_follow_info as plain integers: particles, followed, depth, samples, held, locates"""

    def __init__(self, info):
        for k, _ in _capi.FollowInfo._fields_:
            setattr(self, k, int(getattr(info, k)))

    def __repr__(self):
        return "FollowCounts(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k, _ in _capi.FollowInfo._fields_)


class Follow:
    """What Particles.follow returns: a set of particles - `index`, their texels in the whole texture, strictly increasing - whose
    states sample() appends to a history of `depth` samples kept on the device, and paths() reads back.  Nothing samples by
    itself: step_n(20); sample() records the state after the 20th step.  One set per Particles: a later follow() that succeeds
    replaces this one, and stop() ends it; from then on this object's sample(), read(), paths() and info raise RuntimeError -
    the context's history is another set's, of another size - and its stop() does nothing."""

    def __init__(self, particles, indices, depth):
        self._p = particles
        self.index = np.ascontiguousarray(np.asarray(indices, np.uint32).reshape(-1))
        self.depth = int(depth)
        if not len(self.index):
            raise ValueError("follow: an empty set (stop() ends following)")
        call("th_follow_set", particles._ctx, self.index.ctypes.data_as(C.POINTER(C.c_uint32)), len(self.index), self.depth)
        particles._following = self                 # (a refused set raised above: the set of before is still the followed one)

    def __len__(self):
        return len(self.index)

    @property
    def followed(self):
        """this object's set is the one its Particles follows"""
        return self._p._following is self

    def _current(self, what):
        if not self.followed:
            raise RuntimeError("follow: %s of a set that is no longer followed (replaced by a later follow(), or stopped)" % what)

    def sample(self, time=0.0, buffer=0):
        """the set's states in ring buffer `buffer`, as decoded, into the next row of the history (th_follow_sample: enqueued
        only); `time` is kept beside it on the host"""
        self._current("sample()")
        call("th_follow_sample", self._p._ctx, buffer.index if isinstance(buffer, StateBuffer) else int(buffer), float(time))

    def _counts(self, what):
        """th_follow_info of the context, once it is sure to be of THIS set (th_follow_query: nothing is launched)"""
        self._current(what)
        info = _capi.FollowInfo()
        call("th_follow_query", self._p._ctx, C.byref(info), None, None)
        if int(info.followed) != len(self.index):   # (th_follow_set called beside this object: a row is not len(self) states wide)
            raise RuntimeError("follow: %s of a set of %d, the context follows %d" % (what, len(self.index), int(info.followed)))
        return FollowCounts(info)

    @property
    def info(self):
        """particles, followed, depth, samples, held, locates (th_follow_info)"""
        return self._counts("info")

    def read(self, first, count):
        """samples [first, first + count), oldest first (th_follow_read): ([count, n, 4] float32, [count] float64)"""
        self._counts("read()")                      # (the buffer below is sized by this set: the context's must be the same)
        n, count = len(self.index), max(int(count), 0)
        states, times, info = np.zeros((count, n, 4), np.float32), np.zeros(count, np.float64), _capi.FollowInfo()
        call("th_follow_read", self._p._ctx, int(first), count, states.ctypes.data_as(C.POINTER(C.c_float)) if count else None,
             times.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
        return states, times

    def paths(self, last=None):
        """(states, times) of the last `last` samples held (None: all that are held): states a [n, k, 4] float32 view - particle
        r of the set, sample by sample, oldest first - and times their k times"""
        info = self.info
        k = info.held if last is None else min(max(int(last), 0), info.held)
        states, times = self.read(info.samples - k, k)
        return states.transpose(1, 0, 2), times

    def stop(self):
        """ends following and releases the history (th_follow_set with n = 0); nothing when this set is followed no longer"""
        if self.followed:
            call("th_follow_set", self._p._ctx, None, 0, 1)
            self._p._following = None


LOGIC = "logic"


class StateBuffer:
    """Stand-in for one gl-fbo of the ring: identity survives ring rotation."""

    def __init__(self, particles, ident):
        self._p = particles
        self.id = ident
        self.shape = list(particles.shape)

    @property
    def index(self):
        return self._p.buffers.index(self)

    def read(self):
        return self._p.read(self)

    def set_pixels(self, pixels, offset=(0, 0)):
        self._p._upload(self.index, pixels, offset)

    def source_index(self):          # as PixelSpawner.buffer / spawnData
        return self.index

    def dispose(self):
        pass


def _as_float(v):
    return float(v)


class Particles:
    def __init__(self, gl=None, options=None):
        params = {**defaults(), **(options or {})}
        self.gl = gl
        self.shape = list(params["shape"])
        self.geomShape = list(params["geomShape"] or self.shape)
        logic = params["logic"] or Program(LOGIC)
        self.logic = logic
        self.render = params["render"]
        self.buffers = []
        # src/particles.js:77-78: host staging, ndarray shape [w, h, 4]
        self.pixels = np.zeros((self.shape[0], self.shape[1], 4), np.float32)
        self._device = int(params.get("device", 0))
        self._mode = int(params.get("mode", _capi.TH_MODE_EXACT))
        self._row0 = int(params.get("row0", 0))
        self._global_height = int(params.get("globalHeight", 0))
        self._next_id = 0
        self._following = None                      # the Follow whose set the context follows (Particles.follow), or None
        # best-sample spawning from the particle texture on a row-band shard (PixelSpawner): "auto" - through
        # th_spawn_sample_sharded when the context holds the job's communicator, else the gathered path; True / False force one
        self.sharded_spawn = "auto"
        cfg = _capi.Config(device=self._device, width=self.shape[0], height=self.shape[1],
                           global_height=self._global_height, row0=self._row0, num_buffers=0,
                           mode=self._mode, state_format=int(params.get("stateFormat", 0)))
        self._ctx = C.c_void_p()
        call("th_create", C.byref(cfg), C.byref(self._ctx))
        self.textures = [None] * _capi.MAX_TEXTURES      # who last uploaded into each texture slot of the context (blend.py)

    # -- lifecycle -----------------------------------------------------------------
    def setup(self, numBuffers=1):                  # src/particles.js:81-92
        call("th_setup", self._ctx, int(numBuffers))
        while len(self.buffers) < numBuffers:
            self.buffers.append(StateBuffer(self, self._next_id))
            self._next_id += 1
        while len(self.buffers) > numBuffers:
            self.buffers.pop().dispose()

    def dispose(self):
        if self._ctx:
            call("th_destroy", self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    # -- spawn upload ------------------------------------------------------------------
    def spawn(self, map_fn, pixels=None, offset=(0, 0)):      # src/particles.js:94-117
        pixels = self.pixels if pixels is None else pixels
        w, h = pixels.shape[0], pixels.shape[1]
        data = np.zeros(4, np.float32)
        for x in range(w):
            for y in range(h):
                data[:] = 0
                map_fn(data, x, y)
                pixels[x, y, :] = data
        for k in range(len(self.buffers)):
            self._upload(k, pixels, offset)

    def _upload(self, index, pixels, offset=(0, 0)):
        """pixels: ndarray-convention [w, h, 4] (pixels[x, y]) as in the reference's setPixels."""
        px = np.ascontiguousarray(np.transpose(np.asarray(pixels, np.float32), (1, 0, 2)))
        h, w = px.shape[:2]
        call("th_upload_state", self._ctx, int(index), px.ctypes.data_as(_capi._fp),
             int(offset[0]), int(offset[1]), w, h)

    def upload_texels(self, texels, buffer=-1):
        """texels: [h, w, 4] row-major RGBA32F (readPixels order); buffer -1 = every ring buffer."""
        t = np.ascontiguousarray(texels, np.float32)
        assert t.shape == (self.shape[1], self.shape[0], 4)
        call("th_upload_state", self._ctx, int(buffer), t.ctypes.data_as(_capi._fp), 0, 0,
             self.shape[0], self.shape[1])

    def read(self, buffer=0):
        """readPixels(FLOAT) of a ring buffer -> [h, w, 4]."""
        index = buffer.index if isinstance(buffer, StateBuffer) else int(buffer)
        out = np.empty((self.shape[1], self.shape[0], 4), np.float32)
        call("th_download_state", self._ctx, index, out.ctypes.data_as(_capi._fp), 0, 0,
             self.shape[0], self.shape[1])
        return out

    # -- passes ------------------------------------------------------------------------
    def _target_index(self, buffer):
        if buffer is None:
            return _capi.TH_TARGET_RING
        if isinstance(buffer, StateBuffer):
            return buffer.index
        return buffer.target_index()        # Tendrils.targets texture object

    def step(self, update=None, buffer=None):        # src/particles.js:123-145
        target = self._target_index(buffer)
        uniforms = Particles.applyUpdate(
            dict(self.logic.uniforms, dataRes=self.shape, geomRes=self.geomShape), update)
        self.logic.uniforms = uniforms
        run_pass(self, self.logic, uniforms, target)
        if buffer is None:
            # utils.step(this.buffers): pop -> unshift  (src/utils/index.js:1-7); the C side did the same
            self.buffers.insert(0, self.buffers.pop())

    def step_n(self, update, time0, dt_ms, n):
        """n consecutive logic passes with a fixed-step timer (time_k = time0 + (k+1)*dt_ms, accumulated in
        double like src/timer.js:28-31), replayed from a captured hipGraph.  Extension: the reference
        issues these one draw call at a time.  With a StepProgram as `logic`: the same n steps of the caller's
        integrator in one th_step_program_run, fused where the ring allows (the same bits either way)."""
        uniforms = Particles.applyUpdate(
            dict(self.logic.uniforms, dataRes=self.shape, geomRes=self.geomShape), update)
        self.logic.uniforms = uniforms
        if self.logic.kind == StepProgram.SOURCE_KIND:
            # the times th_step_n computes (th_step.hip): t += dt_ms in double from time0, each value cast to fp32
            times, t = np.empty(max(int(n), 0), np.float32), float(time0)
            for k in range(times.size):
                t += float(dt_ms)
                times[k] = t
            run_step_program(self, self.logic, uniforms, times, np.float32(dt_ms), int(n))
        elif self.logic.kind != LOGIC:
            raise ValueError("step_n runs the logic program only")
        else:
            s = logic_uniforms(uniforms)
            call("th_step_n", self._ctx, C.byref(s), C.c_double(time0), C.c_double(dt_ms), int(n))
        for _ in range(int(n) % max(len(self.buffers), 1)):
            self.buffers.insert(0, self.buffers.pop())

    def step_view_size(self, view_size):
        """The key a StepProgram's calls sort the slots under (th_step_program_view_size): the view size the program's
        particles tap the flow field through, as the built-in integrator does - pos * viewSize.  None: no key (the default);
        a call then steps over whatever slot order it finds and lays out none of its own.  No key changes a result."""
        if view_size is None:
            call("th_step_program_view_size", self._ctx, None)
        else:
            call("th_step_program_view_size", self._ctx, (C.c_float * 2)(float(view_size[0]), float(view_size[1])))

    def draw(self, update=None, mode=None):          # src/particles.js:147-158 - no display here
        return None

    def updateLogic(self, logicFrag):
        self.logic = logicFrag if isinstance(logicFrag, Program) else Program(LOGIC)

    def updateRender(self, *a):
        pass

    def sync(self):
        call("th_sync", self._ctx)

    def draw_pipeline(self, which):
        """Which of the library's two draw() pipelines runs (build-defined, the results are the same): "auto", "stream"
        (texel order, stream-ordered stable sort) or "bins" (any slot order, per-bin ordering)."""
        call("th_draw_pipeline", self._ctx, {"auto": -1, "stream": 0, "bins": 1}[which])

    OPTIONS = dict(bucket=0, resort_steps=1, rebucket_steps=2, fuse=3, graph=4, force_generic=5, draw_reuse=6, bins_pool=7,
                   inject_failure=8, bins_pages=9, async_sort=10, skip_unseen=11, spawn_chunk_rows=12,
                   hash_window=13, hash_window_launches=14, dense_sorts=15, stage_bins=16)
    # (OPTIONS is pinned as it stands - the numbers 0 .. 16, every one once: tests/test_fragment_program_bins_build.py - so the
    # switches that came after it have a table of their own; option() looks a name up in both)
    MORE_OPTIONS = dict(line_bins=17)

    @classmethod
    def option_number(cls, name):
        """TH_OPT_* of the switch `name` (include/tendrils_hip.h)"""
        return cls.OPTIONS[name] if name in cls.OPTIONS else cls.MORE_OPTIONS[name]

    def option(self, name, value=None):
        """A switch between equivalent paths of the library (th_option_set / _get; no switch changes a result): returns the
        current value, sets `value` first if given.  "stage_bins": a draw() pass with a fragment program takes the pipeline the
        pass without it would; "line_bins": beside it, so does a pass whose fragment program reads th_line(f) - alone it changes
        nothing."""
        number = self.option_number(name)
        if value is not None:
            call("th_option_set", self._ctx, number, int(value))
        out = C.c_int64(0)
        call("th_option_get", self._ctx, number, C.byref(out))
        return out.value

    def fetches_taps(self, source):
        """does a sample pass from `source` (as the library sees it) go through th_spawn_sample_sharded?"""
        if self.sharded_spawn != "auto":
            return bool(self.sharded_spawn)
        if source < 0 or self._global_height in (0, self.shape[1]):
            return False
        q = _capi.CommInfo()
        call("th_comm_query", self._ctx, C.byref(q))
        return bool(q.active)

    def deposit_flow(self, view_size, time, speed_limit):
        """The flow pass of Tendrils.draw(): (previous -> current) lines blended into the flow texture
        (src/index.js:295-303, src/particles.js:147-158).  Returns the number of fragments."""
        u = deposit_uniforms(view_size, time, speed_limit)
        n = C.c_uint64(0)
        call("th_flow_deposit", self._ctx, C.byref(u), C.byref(n))
        return int(n.value)

    def export_lines(self, view_size, time, speed_limit):
        """The line list of draw() ([n, 12] float32: p0.xy, p1.xy, c0, c1 in stream order) for offline rendering."""
        u = deposit_uniforms(view_size, time, speed_limit)
        n = C.c_uint64(0)
        call("th_export_lines", self._ctx, C.byref(u), None, 0, C.byref(n))
        out = np.empty((int(n.value), 12), np.float32)
        if n.value:
            call("th_export_lines", self._ctx, C.byref(u), out.ctypes.data_as(_capi._fp), n.value, C.byref(n))
        return out

    def stats(self, speed_limit):
        c = _capi.Counters()
        call("th_stats", self._ctx, C.c_float(speed_limit), C.byref(c))
        return {k: getattr(c, k) for k, _ in _capi.Counters._fields_}

    def _measure_args(self, program, uniforms, buffer):
        if not isinstance(program, MeasureProgram) or not program.handle:
            raise TypeError("measure: %r is no compiled MeasureProgram" % (program,))
        handle, block, size = program_block(program, uniforms or {})
        index = buffer.index if isinstance(buffer, StateBuffer) else int(buffer)
        return (self._ctx, handle, None if block is None else C.byref(block), size, index), block

    def measure(self, program, uniforms=None, buffer=0, everywhere=False):
        """The reduction of a MeasureProgram over ring buffer `buffer` (th_measure_run): a Measure - taken, particles, and sum,
        min, max per channel.  Read-only: the ring stays in the slot order it is held in and nothing else of the context
        changes.  everywhere: over every rank's band of a row-band job (th_measure_global - every rank calls it, all get the
        same bits); without a communicator the same as the local measure."""
        args, _block = self._measure_args(program, uniforms, buffer)
        out = _capi.MeasureResult()
        call("th_measure_global" if everywhere else "th_measure_run", *args, C.byref(out))
        return Measure(out, program.channels)

    def measure_async(self, program, uniforms=None, buffer=0):
        """... enqueued only (th_measure_async): the device address the 144-byte th_measure_result lands at once the context's
        stream gets there (sync()), valid until this context's next measure"""
        args, _block = self._measure_args(program, uniforms, buffer)      # (the block is copied when the launch is enqueued)
        out = C.c_void_p()
        call("th_measure_async", *args, C.byref(out))
        return out.value

    def _density_args(self, w, h, view_size, slot, buffer, into):
        if into not in ("texture", "spawn_image"):
            raise ValueError("density: into=%r (\"texture\" or \"spawn_image\")" % (into,))
        u = _capi.DensityUniforms()
        u.viewSize[0], u.viewSize[1] = float(view_size[0]), float(view_size[1])
        u.w, u.h, u.slot = int(w), int(h), int(slot)
        u.dest = _capi.VIEW_TEXTURE if into == "texture" else _capi.VIEW_SPAWN_IMAGE
        return u, (buffer.index if isinstance(buffer, StateBuffer) else int(buffer))

    def density(self, w, h, view_size, slot=0, buffer=0, into="texture"):
        """The particles of ring buffer `buffer` counted, and their velocities summed, on a w x h grid over the view
        (th_density): the image goes into caller texture `slot` (into="texture": a Blend view, a screen program's unit) or
        becomes the spawner's image (into="spawn_image").  Returns a Density: the five counts, read() for the texels.
        Read-only towards the ring, as measure()."""
        u, index = self._density_args(w, h, view_size, slot, buffer, into)
        info = _capi.DensityInfo()
        call("th_density", self._ctx, C.byref(u), index, C.byref(info))
        if into == "texture":
            self.textures[int(slot)] = None          # (blend.py: whoever uploaded into the slot before no longer holds it)
        return Density(self, info, w, h, into, slot)

    def density_async(self, w, h, view_size, slot=0, buffer=0, into="texture"):
        """... enqueued only (th_density_async): the device address the 40-byte th_density_info lands at once the context's
        stream gets there (sync()), valid until this context's next density"""
        u, index = self._density_args(w, h, view_size, slot, buffer, into)
        out = C.c_void_p()
        call("th_density_async", self._ctx, C.byref(u), index, C.byref(out))
        if into == "texture":
            self.textures[int(slot)] = None
        return out.value

    @staticmethod
    def _select_args(box, speed, stride, phase, inert, buffer):
        u = _capi.SelectUniforms()
        u.stride, u.phase = int(stride), int(phase)
        if box is not None:
            u.flags |= _capi.SELECT_BOX
            u.box[:] = [float(v) for v in box]
        if speed is not None:                        # (lo, hi) in speed units: the library compares the SQUARED speed
            u.flags |= _capi.SELECT_SPEED
            lo, hi = np.float32(speed[0]), np.float32(speed[1])
            with np.errstate(over="ignore"):
                u.speed2[0], u.speed2[1] = float(lo * lo), float(hi * hi)
        if inert:
            u.flags |= _capi.SELECT_INERT
        return u, (buffer.index if isinstance(buffer, StateBuffer) else int(buffer))

    def select(self, box=None, speed=None, stride=1, phase=0, inert=False, buffer=0, capacity=None):
        """The particles of ring buffer `buffer` that match (th_select): inside box = (x0, y0, x1, y1) (half-open, state
        coordinates), with a speed in speed = (lo, hi) (closed; each bound squared in float32), whose texel index % stride ==
        phase; live ones only unless inert.  Returns a Selection, its records in increasing texel: all `matched` of them
        (capacity=None: counted first, then fetched), or the first min(matched, capacity).  Read-only towards the ring, as
        measure()."""
        u, index = self._select_args(box, speed, stride, phase, inert, buffer)
        info = _capi.SelectInfo()
        if capacity is None:
            call("th_select", self._ctx, C.byref(u), index, None, 0, C.byref(info))
            capacity = int(info.matched)
        records = np.zeros(max(int(capacity), 1), SELECTED)
        call("th_select", self._ctx, C.byref(u), index, records.ctypes.data_as(C.POINTER(_capi.Selected)), int(capacity), C.byref(info))
        return Selection(info, records)

    def select_async(self, capacity, box=None, speed=None, stride=1, phase=0, inert=False, buffer=0):
        """... enqueued only (th_select_async): the device addresses (records, info) that up to `capacity` 32-byte th_selected
        records and the 32-byte th_select_info land at once the context's stream gets there (sync()), valid until this
        context's next select; capacity=0 counts only (records: None)"""
        u, index = self._select_args(box, speed, stride, phase, inert, buffer)
        records, info = C.c_void_p(), C.c_void_p()
        call("th_select_async", self._ctx, C.byref(u), index, int(capacity), C.byref(records), C.byref(info))
        return records.value, info.value

    def _histogram_args(self, channel, mode, bins, clauses):
        if isinstance(channel, str):
            if channel not in HIST_CHANNELS:
                raise ValueError("histogram: channel %r (one of %s)" % (channel, ", ".join(HIST_CHANNELS)))
            channel = HIST_CHANNELS[channel]
        buffer = clauses.pop("buffer", 0)
        unknown = set(clauses) - {"box", "speed", "stride", "phase", "inert"}
        if unknown:
            raise TypeError("histogram: unexpected clause(s) %s" % ", ".join(sorted(unknown)))
        select, index = self._select_args(clauses.get("box"), clauses.get("speed"), clauses.get("stride", 1), clauses.get("phase", 0),
                                          clauses.get("inert", False), buffer)
        u = _capi.HistogramUniforms()
        u.select = select
        u.channel, u.mode, u.bins = int(channel), int(mode), int(bins)
        return u, index

    def histogram(self, channel, bins, range, box=None, speed=None, stride=1, phase=0, inert=False, buffer=0):
        """How one scalar of the state is distributed (th_histogram): the particles of ring buffer `buffer` that match select()'s
        clauses, counted per bin of `channel` - "x", "y", "vx", "vy", "speed2", "speed" or a TH_HIST_* number - over `bins`
        (1 .. 4096) equal bins of range = (lo, hi), lo inclusive, hi exclusive, binned in float32.  Returns a Histogram.
        Read-only towards the ring, as select()."""
        u, index = self._histogram_args(channel, _capi.HIST_LINEAR, bins, dict(box=box, speed=speed, stride=stride, phase=phase, inert=inert, buffer=buffer))
        u.lo, u.hi = float(range[0]), float(range[1])
        counts, info = np.zeros(max(int(bins), 0), np.uint32), _capi.HistogramInfo()
        call("th_histogram", self._ctx, C.byref(u), index, counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info))
        return Histogram(info, counts, u.lo, u.hi)

    def histogram_async(self, channel, bins, range, box=None, speed=None, stride=1, phase=0, inert=False, buffer=0):
        """... enqueued only (th_histogram_async): the device addresses (counts, info) that the `bins` uint32 counts and the
        48-byte th_histogram_info land at once the context's stream gets there (sync()), valid until this context's next
        histogram"""
        u, index = self._histogram_args(channel, _capi.HIST_LINEAR, bins, dict(box=box, speed=speed, stride=stride, phase=phase, inert=inert, buffer=buffer))
        u.lo, u.hi = float(range[0]), float(range[1])
        counts, info = C.c_void_p(), C.c_void_p()
        call("th_histogram_async", self._ctx, C.byref(u), index, C.byref(counts), C.byref(info))
        return counts.value, info.value

    def _key_pass(self, channel, bins, shift, prefix, clauses):
        """one TH_HIST_KEY pass: (the counts as int64, th_histogram_info)"""
        u, index = self._histogram_args(channel, _capi.HIST_KEY, bins, dict(clauses))
        u.key_prefix, u.key_shift = int(prefix), int(shift)
        counts, info = np.zeros(bins, np.uint32), _capi.HistogramInfo()
        call("th_histogram", self._ctx, C.byref(u), index, counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info))
        return counts.astype(np.int64), info

    def quantiles(self, channel, q, **clauses):
        """Exact order statistics of `channel` over the particles that match (select()'s clauses, `buffer` among them): for each
        q in [0, 1] the element of rank k = min(floor(q * n), n - 1) of the n = matched - nan values in ascending order (-0.0
        below +0.0), as float32 - bit for bit what sorting them gives.  Radix select over the monotone key of the float: three
        TH_HIST_KEY passes of 11, 11 and 10 bits, the prefix narrowed from `below` and the cumulative counts; ranks whose
        prefixes coincide share their passes.  q a float: a float32, a sequence: a float32 array; None when n == 0."""
        scalar = np.ndim(q) == 0
        qs = [float(v) for v in np.atleast_1d(q)]
        if not all(0.0 <= v <= 1.0 for v in qs):
            raise ValueError("quantiles: q outside [0, 1]")
        (bins, shift), rest = QUANTILE_PASSES[0], QUANTILE_PASSES[1:]
        counts, info = self._key_pass(channel, bins, shift, 0, clauses)
        n = int(info.matched) - int(info.nan)
        if n <= 0:
            return None
        ranks = [min(int(np.floor(v * n)), n - 1) for v in qs]
        # (the first pass has no prefix: nothing is below it)
        reached = int(info.below) + np.cumsum(counts)
        prefixes = {k: int(np.searchsorted(reached, k, side="right")) << shift for k in set(ranks)}
        for bins, shift in rest:
            passes = {}
            for k, prefix in prefixes.items():
                if prefix not in passes:
                    counts, info = self._key_pass(channel, bins, shift, prefix, clauses)
                    passes[prefix] = int(info.below) + np.cumsum(counts)
                prefixes[k] = prefix | (int(np.searchsorted(passes[prefix], k, side="right")) << shift)
        out = key_float(np.array([prefixes[k] for k in ranks], np.uint32))
        return out[0] if scalar else out

    def follow(self, indices, depth=64):
        """Follow the particles at texels `indices` - anything np.asarray(..., np.uint32) takes, Selection.index in particular:
        whole-texture indices, strictly increasing, inside this context's rows - in a history of `depth` samples on the device
        (th_follow_set).  Returns a Follow: .sample(time=0.0, buffer=0), .paths(last=None), .info, .stop().  Read-only towards
        the ring, as select(); replaces the set followed before, whose Follow raises from then on."""
        return Follow(self, indices, depth)

    @staticmethod
    def generateLUT(shape):                          # src/particles.js:171-190
        w, h = max(shape[0], 2), max(shape[1], 2)
        inv_x, inv_y = 1 / (w - 1), 1 / (h - 1)
        data = np.zeros(shape[0] * shape[1] * 2, np.float32)
        k = 0
        for i in range(w):
            for j in range(h):
                if k + 1 < data.size:
                    data[k] = i * inv_x
                    data[k + 1] = j * inv_y
                k += 2
        return data

    @staticmethod
    def applyUpdate(state, update):                  # src/particles.js:192-195
        if callable(update):
            return update(state)
        state.update(update or {})
        return state


def logic_uniforms(u):
    """dict of reference uniform names -> C struct (double -> fp32 as gl.uniform1f does)."""
    s = _capi.LogicUniforms()
    vs = u.get("viewSize", (1.0, 1.0))
    s.viewSize[0], s.viewSize[1] = float(vs[0]), float(vs[1])
    for name, _ in _capi.LogicUniforms._fields_:
        if name == "viewSize":
            continue
        setattr(s, name, _as_float(u.get(name, 0.0)))
    return s


def run_pass(particles, program, uniforms, target):
    """One full-screen pass of `program` into `target` (screen.render(), src/particles.js:143)."""
    ctx = particles._ctx
    kind = program.kind
    if kind == LOGIC:
        s = logic_uniforms(uniforms)
        call("th_step", ctx, C.byref(s), target)
    elif kind == "spawn-init":
        call("th_spawn_init", ctx, target)
    elif kind == "spawn-ball":
        s = _capi.SpawnBallUniforms(radius=float(uniforms.get("radius", 1)), speed=float(uniforms.get("speed", 0)))
        call("th_spawn_ball", ctx, C.byref(s), target)
    elif kind in ("spawn-sample", "spawn-direct"):
        s = _capi.SpawnSampleUniforms()
        for name in ("spawnSize", "jitter"):
            v = uniforms.get(name, (1.0, 1.0))
            getattr(s, name)[0], getattr(s, name)[1] = float(v[0]), float(v[1])
        for name in ("time", "speed", "bias", "flowDecay"):
            setattr(s, name, float(uniforms.get(name, 0.0)))
        m = uniforms.get("spawnMatrix", (1, 0, 0, 0, 1, 0, 0, 0, 1))
        for k in range(9):
            s.spawnMatrix[k] = float(m[k])
        s.samples = int(program.fixed.get("samples", 0))
        s.apply = int(program.fixed.get("apply", 2))
        src = uniforms.get("spawnData")
        if hasattr(src, "bind_for"):                      # the spawner's own image buffer: uploaded on use
            src.bind_for(particles)
        source = src if isinstance(src, int) else src.source_index()
        if source >= 0 and target == _capi.TH_TARGET_RING:
            # the C side resolves ring indices AFTER utils.step() rotated the ring (the order the
            # pass sees); `source` was taken from the pre-rotation list
            source = (source + 1) % len(particles.buffers)
        if kind == "spawn-sample" and particles.fetches_taps(source):
            call("th_spawn_sample_sharded", ctx, C.byref(s), source, target)      # every rank, collectively
        else:
            call("th_spawn_sample" if kind == "spawn-sample" else "th_spawn_direct", ctx, C.byref(s), source, target)
    elif kind == "user":
        if not program.handle:
            raise ValueError("user program %r was disposed" % (program.fixed.get("name"),))
        block = program.pack(uniforms)
        source = _program_source(particles, uniforms, target)
        call("th_program_run", ctx, program.handle, C.byref(block) if block is not None else None,
             C.sizeof(block) if block is not None else 0, source, target)
    elif kind == "step":
        if target != _capi.TH_TARGET_RING:
            raise ValueError("a step program steps the ring: it has no other target")
        times = np.array([uniforms.get("time", 0.0)], np.float64).astype(np.float32)
        run_step_program(particles, program, uniforms, times, np.float32(uniforms.get("dt", 0.0)), 1)
    else:
        raise ValueError("unknown program kind %r" % (kind,))


def _program_source(particles, uniforms, target):
    """the spawnData of a caller's pass as the library names it (TH_SOURCE_NONE without one)"""
    src = uniforms.get("spawnData")
    if src is None:
        return _capi.TH_SOURCE_NONE
    if hasattr(src, "bind_for"):                  # a spawner's own image buffer: uploaded on use
        src.bind_for(particles)
    source = src if isinstance(src, int) else src.source_index()
    if source >= 0 and target == _capi.TH_TARGET_RING:
        source = (source + 1) % len(particles.buffers)      # (as for the sample passes: the order the pass sees)
    return source


def run_step_program(particles, program, uniforms, times, dt, n):
    """n steps of a step program over the ring in one call (th_step_program_run): step k sees times[k], dt and k."""
    if not program.handle:
        raise ValueError("step program %r was disposed" % (program.fixed.get("name"),))
    block = program.pack(uniforms)
    source = _program_source(particles, uniforms, _capi.TH_TARGET_RING)
    times = np.ascontiguousarray(times, np.float32)
    call("th_step_program_run", particles._ctx, program.handle, C.byref(block) if block is not None else None,
         C.sizeof(block) if block is not None else 0, source, times.ctypes.data_as(_capi._fp), C.c_float(float(dt)), int(n))


default = Particles
