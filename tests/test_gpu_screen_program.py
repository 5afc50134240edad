"""Screen programs on the GPU (include/tendrils_hip.h "screen programs"; tendrils_amd/csrc/th_screen.hip and th_screen_prelude.inc):
a full-screen pass the caller wrote, over the view images, the colour map and the caller's textures.  Every comparison is on the
bytes (RGBA8) or on the fp32 bit patterns: under -ffp-contract=off every operation involved is one rounded fp32 operation or an
integer one.  The references are the library's own passes for the same job (th_view_copy, th_view_fill) and the restatement of
the colour-map blend (tests/blend_restatement.py).  The programs read through the accessors alone; each is compiled once."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_restatement as R
import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import Program, ScreenProgram
from tendrils_amd.tendrils import View

from helpers import ROOT, bits_equal
from test_program_build import DRIFT

pytestmark = pytest.mark.gpu

F = np.float32
FORMAT = {"rgba32f": _capi.TEX_RGBA32F, "rgba8": _capi.TEX_RGBA8, "l32f": _capi.TEX_L32F}
TEX, FRAMES, IMAGE = _capi.VIEW_TEXTURE, _capi.VIEW_FRAMES, _capi.VIEW_SPAWN_IMAGE
BUFFER, SCREEN, COLORMAP, FLOW = _capi.VIEW_BUFFER, _capi.VIEW_SCREEN, _capi.VIEW_COLORMAP, _capi.VIEW_FLOW
TO_VIEW, TO_MAP, TO_TEX = _capi.SCREEN_TARGET_VIEW, _capi.SCREEN_TARGET_COLORMAP, _capi.SCREEN_TARGET_TEXTURE
SHAPES = ((37, 23), (300, 2), (1, 1))      # odd and below a workgroup per row; a row longer than a workgroup; one texel


class Colour(C.Structure):
    _fields_ = [("rgba", C.c_float * 4)]


class Count(C.Structure):
    _fields_ = [("n", C.c_int32)]


COPY = """__device__ float4 th_screen(const th_screen_pass &s)
{
    return th_tex(s, 0, s.uv.x, s.uv.y);
}
"""

FILL = """struct Colour { float rgba[4]; };
__device__ float4 th_screen(const th_screen_pass &s)
{
    const Colour &u = th_uniforms<Colour>(s);
    return make_float4(u.rgba[0], u.rgba[1], u.rgba[2], u.rgba[3]);
}
"""

COORDS = """__device__ float4 th_screen(const th_screen_pass &s)
{
    return make_float4((float)s.x, (float)s.y, s.uv.x, s.uv.y);
}
"""

SHAPE_OF = """__device__ float4 th_screen(const th_screen_pass &s)
{
    const float2 r = th_tex_res(s, 0);
    return make_float4(s.res.x, s.res.y, r.x, r.y);
}
"""

# texture2D(unit k, (1 - uv.x, uv.y)) summed over the first n units, in order
SUM = """struct Count { int n; };
__device__ float4 th_screen(const th_screen_pass &s)
{
    const int n = th_uniforms<Count>(s).n;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < n; ++k) {
        const float4 t = th_tex(s, k, 1.0f - s.uv.x, s.uv.y);
        a = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
    }
    return a;
}
"""

# every accessor at unit n, which the caller leaves unbound
BEYOND = """struct Count { int n; };
__device__ float4 th_screen(const th_screen_pass &s)
{
    const int n = th_uniforms<Count>(s).n;
    const float4 a = th_tex(s, n, s.uv.x, s.uv.y), b = th_texel(s, n, s.x, s.y), c = th_tex(s, -1, 0.5f, 0.5f);
    const float2 r = th_tex_res(s, n);
    return make_float4(a.x + b.x + c.x + r.x, a.y + b.y + c.y + r.y, a.z + b.z + c.z, a.w + b.w + c.w);
}
"""

# a 3 x 3 box over unit 0: rows top to bottom, texels left to right, then * (1 / 9)
BOX = """__device__ float4 th_screen(const th_screen_pass &s)
{
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const float4 t = th_texel(s, 0, s.x + dx, s.y + dy);
            a = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
        }
    const float k = 1.0f / 9.0f;
    return make_float4(a.x * k, a.y * k, a.z * k, a.w * k);
}
"""


@pytest.fixture(scope="module")
def programs():
    progs = dict(
        copy=ScreenProgram.from_source(COPY, name="copy"),
        fill=ScreenProgram.from_source(FILL, Colour, name="fill"),
        coords=ScreenProgram.from_source(COORDS, name="coords"),
        shape_of=ScreenProgram.from_source(SHAPE_OF, name="shape_of"),
        sum=ScreenProgram.from_source(SUM, Count, name="sum"),
        beyond=ScreenProgram.from_source(BEYOND, Count, name="beyond"),
        box=ScreenProgram.from_source(BOX, name="box"),
        drift=Program.from_source(DRIFT, name="drift"),
    )
    yield progs
    for p in progs.values():
        p.dispose()


def make(view=(16, 9), n=8, buffers=0, **options):
    options = dict(options, numBuffers=buffers)
    t = ta.Tendrils(View(*view), options)
    t.resize()
    t.setup(n)
    return t


def units_table(units):
    tab = (_capi.ScreenUnit * max(len(units), 1))()
    for i, (source, index) in enumerate(units):
        tab[i].source, tab[i].index = source, index
    return tab


def run(ctx, prog, units=(), target=TO_VIEW, index=0, gl_blend=1, block=None):
    call("th_screen_run", ctx, prog.handle, None if block is None else C.byref(block), 0 if block is None else C.sizeof(block),
         units_table(units), len(units), target, index, int(gl_blend))


def status_of(ctx, prog, units=(), target=TO_VIEW, index=0, gl_blend=1, block=None, size=None, n=None):
    lib = _capi.load()
    handle = prog.handle if hasattr(prog, "handle") else prog
    size = (0 if block is None else C.sizeof(block)) if size is None else size
    status = lib.th_screen_run(ctx, handle, None if block is None else C.byref(block), size, units_table(units),
                               len(units) if n is None else n, target, index, int(gl_blend))
    return status, lib.th_last_error().decode()


def upload(ctx, slot, fmt, texels):
    t = np.ascontiguousarray(texels, np.uint8 if fmt == "rgba8" else F)
    w, h = (t.size, 1) if fmt == "l32f" else (t.shape[1], t.shape[0])
    call("th_texture_upload", ctx, slot, FORMAT[fmt], t.ctypes.data_as(C.c_void_p), w, h)


def read_slot(ctx, slot, shape, dtype=F):
    out = np.empty(shape, dtype)
    call("th_texture_download", ctx, slot, out.ctypes.data_as(C.c_void_p))
    return out


def read_map(ctx):
    w, h = C.c_int32(), C.c_int32()
    call("th_colormap_shape", ctx, C.byref(w), C.byref(h))
    out = np.empty((h.value, w.value, 4), F)
    call("th_colormap_download", ctx, out.ctypes.data_as(_capi._fp))
    return out


def set_image(t, buffer, image):
    """the bytes of `image` into one of t.buffers (None: the screen), through the device pointer of the bound view image; what
    was bound stays bound"""
    import torch
    from tendrils_amd.sharding import device_view
    was = t._bound
    t._bind_view(buffer)
    ptr = C.c_void_p()
    call("th_view_device_ptr", t.particles._ctx, C.byref(ptr))
    call("th_sync", t.particles._ctx)
    h, w = image.shape[:2]
    device_view(ptr.value, (h * w, 4), "|u1").copy_(torch.from_numpy(np.ascontiguousarray(image, np.uint8).reshape(-1, 4)))
    torch.cuda.synchronize()
    t._bind_view(was)


def random_image(rng, view):
    img = rng.integers(1, 255, (view[1], view[0], 4)).astype(np.uint8)
    img.reshape(-1, 4)[3::5, 3] = 0                      # alphas of 0 and 255 among them
    img.reshape(-1, 4)[1::7, 3] = 255
    img.reshape(-1, 4)[2::11, :3] = 255                  # ... and colours at both ends
    img.reshape(-1, 4)[5::13, :3] = 0
    return img


def assert_bits(got, want):
    same = bits_equal(got, want)
    assert same.all(), "%d of %d components differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])


def assert_bytes(got, want):
    same = got == want
    assert same.all(), "%d of %d bytes differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])


# ---- 1, 2: the library's own passes for the same job ----------------------------------------------------------------------
@pytest.mark.parametrize("view", SHAPES, ids=lambda v: "%dx%d" % v)
def test_copy_program_equals_th_view_copy(programs, view):
    rng = np.random.default_rng(view[0])
    front, screen = random_image(rng, view), random_image(rng, view)
    got = []
    for with_program in (False, True):
        t = make(view, buffers=2)
        set_image(t, t.buffers[0], front)
        set_image(t, None, screen)
        t._bind_view(None)
        if with_program:
            run(t.particles._ctx, programs["copy"], [(BUFFER, 0)], TO_VIEW, 0, 1)
        else:
            call("th_view_copy", t.particles._ctx, 0)
        got.append((t.read_view(), t.buffers[0].read()))
        t.dispose()
    (want, kept), (out, kept_too) = got
    assert (want != screen).any() and (kept == front).all() and (kept_too == front).all()
    assert_bytes(out, want)


@pytest.mark.parametrize("colour", ([0.3, 0.6, 0.9, 0.0], [0.2, 0.5, 0.1, 0.37], [0.9, 0.1, 0.4, 1.0], [1.7, -0.4, 0.5, 0.37],
                                    [0.25, 2.5, -3.0, 1.5], [0.5, 0.5, 0.5, -0.2]), ids=str)
def test_fill_program_equals_th_view_fill(programs, colour):
    view = (37, 23)
    under = random_image(np.random.default_rng(5), view)
    got = []
    for with_program in (False, True):
        t = make(view)
        set_image(t, None, under)
        if with_program:
            run(t.particles._ctx, programs["fill"], [], TO_VIEW, 0, 1, Colour(rgba=(C.c_float * 4)(*colour)))
        else:
            t.drawFill(colour)
        got.append(t.read_view())
        t.dispose()
    assert_bytes(got[1], got[0])
    assert colour[3] <= 0 or (got[0] != under).any()


# ---- 3: coordinates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda v: "%dx%d" % v)
def test_coordinates_and_shapes(programs, shape):
    w, h = shape
    t = make()
    ctx = t.particles._ctx
    upload(ctx, 0, "rgba32f", np.full((h, w, 4), 7.0, F))
    upload(ctx, 1, "rgba8", np.zeros((5, 11, 4), np.uint8))
    run(ctx, programs["coords"], [], TO_TEX, 0, 0)
    got = read_slot(ctx, 0, (h, w, 4))
    want = np.empty((h, w, 4), F)
    want[..., 0] = np.arange(w, dtype=F)[None, :]
    want[..., 1] = np.arange(h, dtype=F)[:, None]
    want[..., 2] = ((np.arange(w, dtype=F) + F(0.5)) / F(w)).astype(F)[None, :]
    want[..., 3] = ((np.arange(h, dtype=F) + F(0.5)) / F(h)).astype(F)[:, None]
    assert_bits(got, want)
    run(ctx, programs["shape_of"], [(TEX, 1)], TO_TEX, 0, 0)
    assert_bits(read_slot(ctx, 0, (h, w, 4)), np.broadcast_to(np.array([w, h, 11, 5], F), (h, w, 4)))
    t.dispose()


# ---- 4: every unit source and format through th_tex ----------------------------------------------------------------------------
def tap_sum(views, w, h):
    """SUM over `views` = [(format, texels)] for every texel of a w x h target, with the restatement's taps"""
    u = (F(1.0) - ((np.arange(w, dtype=F) + F(0.5)) / F(w)).astype(F)).astype(F)
    v = ((np.arange(h, dtype=F) + F(0.5)) / F(h)).astype(F)
    total = np.zeros((h, w, 4), F)
    for fmt, texels in views:
        tex = R.decode(fmt, texels)
        tap = R.nearest_fx16 if fmt == "rgba8" else R.nearest
        total = (total + tex[tap(v, tex.shape[0])[:, None], tap(u, tex.shape[1])[None, :]]).astype(F)
    return total


def test_every_unit_source_and_format_through_th_tex(programs):
    rng = np.random.default_rng(41)
    view, (w, h) = (10, 4), (24, 16)
    t = make(view, buffers=2)
    ctx = t.particles._ctx
    f32 = lambda *shape: rng.uniform(-2, 2, shape).astype(F)                  # noqa: E731
    u8 = lambda *shape: rng.integers(0, 256, shape).astype(np.uint8)         # noqa: E731
    tex = dict(rgba32f=f32(11, 13, 4), rgba8=u8(9, 17, 4), l32f=f32(32))
    frame_a, frame_b, image, cmap, flow = u8(6, 8, 4), u8(6, 8, 4), f32(7, 5, 4), f32(3, 3, 4), f32(4, 10, 4)
    back, screen = u8(4, 10, 4), u8(4, 10, 4)
    for slot, fmt in enumerate(("rgba32f", "rgba8", "l32f")):
        upload(ctx, slot, fmt, tex[fmt])
    upload(ctx, 3, "rgba32f", np.zeros((h, w, 4), F))                         # the target
    call("th_frames_resize", ctx, 8, 6)
    call("th_frames_upload", ctx, frame_a.ctypes.data_as(C.POINTER(C.c_uint8)))
    call("th_frames_rotate", ctx)
    call("th_frames_upload", ctx, frame_b.ctypes.data_as(C.POINTER(C.c_uint8)))      # buffers = [b, a]
    call("th_spawn_image_upload", ctx, image.ctypes.data_as(_capi._fp), 5, 7)
    call("th_colormap_upload", ctx, cmap.ctypes.data_as(_capi._fp), 3, 3)
    t.flow.set_pixels(flow)
    set_image(t, t.buffers[1], back)
    set_image(t, None, screen)
    t.buffers[0].bind()                                                       # (the screen is a unit while another image is bound)
    first = [((TEX, 0), ("rgba32f", tex["rgba32f"])), ((TEX, 1), ("rgba8", tex["rgba8"])), ((TEX, 2), ("l32f", tex["l32f"])),
             ((FRAMES, 0), ("rgba8", frame_b)), ((FRAMES, 1), ("rgba8", frame_a))]
    second = [((IMAGE, 0), ("rgba32f", image)), ((COLORMAP, 0), ("rgba32f", cmap)), ((FLOW, 0), ("rgba32f", flow)),
              ((BUFFER, 1), ("rgba8", back)), ((SCREEN, 0), ("rgba8", screen))]
    for group in (first, second, first + second[:3]):                        # (the last: all 8 units of one pass)
        units, views = [g[0] for g in group], [g[1] for g in group]
        run(ctx, programs["sum"], units, TO_TEX, 3, 0, Count(n=len(units)))
        assert_bits(read_slot(ctx, 3, (h, w, 4)), tap_sum(views, w, h))
    # a unit index at or beyond the bound units reads as zeros, through every accessor
    for units in ([], [g[0] for g in first]):
        upload(ctx, 3, "rgba32f", np.ones((h, w, 4), F))
        run(ctx, programs["beyond"], units, TO_TEX, 3, 0, Count(n=len(units)))
        assert_bits(read_slot(ctx, 3, (h, w, 4)), np.zeros((h, w, 4), F))
    t.dispose()


# ---- 5: neighbour taps, edge clamp, RGBA8 rounding ---------------------------------------------------------------------------------
def box_ref(image):
    tex = R.decode("rgba8", image)
    h, w = tex.shape[:2]
    total = np.zeros_like(tex)
    ys, xs = np.arange(h), np.arange(w)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            total = (total + tex[np.clip(ys + dy, 0, h - 1)[:, None], np.clip(xs + dx, 0, w - 1)[None, :]]).astype(F)
    c = (total * (F(1.0) / F(9.0))).astype(F)
    return ((np.clip(c, F(0.0), F(1.0)) * F(255.0)).astype(F) + F(0.5)).astype(F).astype(np.uint8)


def test_box_through_th_texel_clamps_at_the_edges_and_rounds_like_the_view(programs):
    view = (37, 23)
    front = random_image(np.random.default_rng(6), view)
    t = make(view, buffers=1)
    set_image(t, t.buffers[0], front)
    set_image(t, None, random_image(np.random.default_rng(7), view))          # (gl_blend = 0: nothing of it may remain)
    t._bind_view(None)
    run(t.particles._ctx, programs["box"], [(BUFFER, 0)], TO_VIEW, 0, 0)
    got, want = t.read_view(), box_ref(front)
    t.dispose()
    for what, part in (("top row", np.s_[0]), ("bottom row", np.s_[-1]), ("left column", np.s_[:, 0]), ("right column", np.s_[:, -1])):
        assert (got[part] == want[part]).all(), what
    assert_bytes(got, want)
    assert (want != front).any()


# ---- 6: a float target ---------------------------------------------------------------------------------------------------------------
def test_float_blend_into_the_colour_map(programs):
    rng = np.random.default_rng(8)
    before = rng.uniform(-1, 2, (3, 3, 4)).astype(F)
    t = make()
    ctx = t.particles._ctx
    for colour in ([0.3, 0.6, 0.9, 0.0], [0.2, 0.5, 0.1, 0.37], [1.7, -0.4, 0.5, 1.0], [0.25, 2.5, -3.0, 1.5]):
        src = np.broadcast_to(np.array(colour, F), (3, 3, 4)).copy()
        block = Colour(rgba=(C.c_float * 4)(*colour))
        call("th_colormap_upload", ctx, before.ctypes.data_as(_capi._fp), 3, 3)
        run(ctx, programs["fill"], [], TO_MAP, 0, 1, block)
        assert_bits(read_map(ctx), R.blend_stage(src, gl_blend=True, clear=False, dst=before))
        run(ctx, programs["fill"], [], TO_MAP, 0, 0, block)
        assert_bits(read_map(ctx), src)                                       # stored: nothing clamped
    t.dispose()


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_target_as_it_was(programs):
    view = (16, 9)
    rng = np.random.default_rng(9)
    t = make(view, buffers=2)
    ctx = t.particles._ctx
    lib = _capi.load()
    set_image(t, t.buffers[0], random_image(rng, view))
    set_image(t, t.buffers[1], random_image(rng, view))
    set_image(t, None, random_image(rng, view))
    cmap = rng.uniform(0, 1, (3, 3, 4)).astype(F)
    call("th_colormap_upload", ctx, cmap.ctypes.data_as(_capi._fp), 3, 3)
    upload(ctx, 0, "rgba32f", rng.uniform(0, 1, (4, 6, 4)).astype(F))
    upload(ctx, 1, "l32f", rng.uniform(0, 1, 12).astype(F))
    copy, fill = programs["copy"], programs["fill"]
    big = (C.c_uint8 * 1025)()

    def snapshot():
        return (t.read_view().tobytes(), t.buffers[0].read().tobytes(), t.buffers[1].read().tobytes(), read_map(ctx).tobytes(),
                read_slot(ctx, 0, (4, 6, 4)).tobytes(), read_slot(ctx, 1, (12,)).tobytes())

    t.buffers[1].bind()
    cases = {
        "the bound buffer as a unit": (dict(prog=copy, units=[(BUFFER, 1)]), "unit 0"),
        "the bound buffer as the second unit": (dict(prog=copy, units=[(BUFFER, 0), (BUFFER, 1)]), "unit 1"),
        "the colour map into itself": (dict(prog=copy, units=[(COLORMAP, 0)], target=TO_MAP), "unit 0"),
        "a slot as unit and target": (dict(prog=copy, units=[(TEX, 0)], target=TO_TEX, index=0), "unit 0"),
        "nine units": (dict(prog=copy, units=[(BUFFER, 0)] * 9), "9"),
        "a negative number of units": (dict(prog=copy, units=[(BUFFER, 0)], n=-1), "-1"),
        "an empty slot": (dict(prog=copy, units=[(TEX, 5)]), "slot 5"),
        "an empty target slot": (dict(prog=copy, units=[(BUFFER, 0)], target=TO_TEX, index=5), "slot 5"),
        "an L32F target slot": (dict(prog=copy, units=[(BUFFER, 0)], target=TO_TEX, index=1), "slot 1"),
        "frames before th_frames_resize": (dict(prog=copy, units=[(FRAMES, 0)]), "th_frames_resize"),
        "no spawn image": (dict(prog=copy, units=[(IMAGE, 0)]), "spawn image"),
        "a buffer beyond the ring": (dict(prog=copy, units=[(BUFFER, 2)]), "view buffer 2"),
        "an unknown source": (dict(prog=copy, units=[(7, 0)]), "source 7"),
        "an unknown target": (dict(prog=copy, units=[(BUFFER, 0)], target=3), "target 3"),
        "1025 uniform bytes": (dict(prog=fill, block=big, size=1025), "1025"),
        "null uniforms with a size": (dict(prog=fill, size=16), "null uniforms"),
        "a null program": (dict(prog=None, units=[(BUFFER, 0)]), "null program"),
        "a state program": (dict(prog=programs["drift"], units=[(BUFFER, 0)]), "state program"),
    }
    for what, (args, names) in cases.items():
        before = snapshot()
        status, message = status_of(ctx, **args)
        assert status == _capi.TH_ERR_INVALID and names in message, (what, status, message)
        assert snapshot() == before, what
        block = Colour(rgba=(C.c_float * 4)(*rng.uniform(0, 1, 3), 1.0))      # the context still runs a valid pass
        run(ctx, fill, [], TO_VIEW, 0, 1, block)
        assert t.buffers[1].read().tobytes() != before[2] and snapshot()[:2] == before[:2], what
    status, message = status_of(ctx, programs["drift"], [(BUFFER, 0)])
    assert "state program" in message and "screen program" in message        # both kinds named
    # the screen is a unit while a buffer is bound - and the feedback loop once it is bound itself
    t._bind_view(None)
    before = snapshot()
    status, message = status_of(ctx, copy, [(SCREEN, 0)])
    assert status == _capi.TH_ERR_INVALID and "unit 0" in message and snapshot() == before
    run(ctx, copy, [(BUFFER, 1)], TO_VIEW, 0, 1)
    # the other way round: th_program_run takes no screen program
    before = t.particles.read(0).tobytes()
    status = lib.th_program_run(ctx, copy.handle, None, 0, _capi.TH_SOURCE_NONE, 0)
    message = lib.th_last_error().decode()
    assert status == _capi.TH_ERR_INVALID and "state program" in message and "screen program" in message
    assert t.particles.read(0).tobytes() == before
    call("th_program_run", ctx, programs["drift"].handle, (C.c_uint8 * 4)(), 4, _capi.TH_SOURCE_NONE, 0)
    # the colour-map blend knows none of the new sources
    view_table = (_capi.BlendView * 1)()
    for source in (BUFFER, SCREEN, COLORMAP, FLOW):
        view_table[0].source, view_table[0].index, view_table[0].alpha = source, 0, 1.0
        assert lib.th_colormap_blend(ctx, view_table, 1, 1, 1) == _capi.TH_ERR_INVALID and b"unknown source" in lib.th_last_error()
    t.dispose()


# ---- 8: what a pass leaves alone -------------------------------------------------------------------------------------------------------
def test_the_simulation_does_not_notice_a_screen_pass(programs):
    """a 64 x 64 state over a 40 x 40 flow, tile-sorted slots re-sorted every 2 steps: two steps with screen passes into every
    kind of target in between - the state, the slot order and the counters are those of the run without them"""
    n = 64
    rng = np.random.default_rng(17)
    st = np.zeros((n, n, 4), F)
    st[..., :2] = rng.uniform(-1, 1, (n, n, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (n, n, 2))
    flow = np.zeros((40, 40, 4), F)
    flow[..., :2] = rng.uniform(-.01, .01, (40, 40, 2))
    flow[..., 2] = 90.0
    results = []
    for passes in (False, True):
        t = make((40, 40), n, buffers=1)
        ctx = t.particles._ctx
        call("th_option_set", ctx, 0, 1)                     # TH_OPT_BUCKET: always
        call("th_option_set", ctx, 1, 2)                     # TH_OPT_RESORT_STEPS
        t.particles.upload_texels(st)
        t.flow.set_pixels(flow)
        t.timer.time = 100.0
        upload(ctx, 0, "rgba32f", np.zeros((5, 7, 4), F))
        for _ in range(2):
            t.timer.tick()
            t.step()
        order, counters = _capi.SlotOrderInfo(), _capi.Counters()
        call("th_slot_order", ctx, C.byref(order))
        before = (order.sorted_buffers, order.sorts)
        if passes:
            t._bind_view(None)
            run(ctx, programs["copy"], [(BUFFER, 0)], TO_VIEW, 0, 1)
            run(ctx, programs["copy"], [(FLOW, 0)], TO_MAP, 0, 1)
            run(ctx, programs["box"], [(FLOW, 0)], TO_TEX, 0, 0)
            call("th_slot_order", ctx, C.byref(order))
            assert (order.sorted_buffers, order.sorts) == before
        for _ in range(2):
            t.timer.tick()
            t.step()
        call("th_slot_order", ctx, C.byref(order))
        call("th_stats", ctx, float(t.state["speedLimit"]), C.byref(counters))
        results.append((t.particles.read(0), t.particles.read(1), order.sorted_buffers, order.sorts, counters.respawned, bytes(counters)))
        t.dispose()
    (a0, a1, *a), (b0, b1, *b) = results
    assert a[1] > 0 and a == b                                # (the slot order was live)
    assert_bits(b0, a0)
    assert_bits(b1, a1)


# ---- 9: the demo's order, on the Python host -----------------------------------------------------------------------------------------------
def test_the_demos_last_pass_with_a_copy_program_equals_copy_buffer(programs):
    """src/demo.main.js:1084-1102 with a copy shader where the demo binds its blur: draw() into buffers[0]; bind the screen,
    drawFade(), the pass over buffers[0], stepBuffers()"""
    from test_gpu_view_buffers import inputs
    n, view = 96, (96, 54)
    cur, prev = inputs(n, view, 3)
    got = []
    for with_program in (False, True):
        opts = ta.defaults()
        opts["numBuffers"] = 1
        opts["state"].update(baseColor=[1, 0.7, 0.3, 0.6], flowColor=[0.2, 1, 0.9, 0.3], fadeColor=[0.1, 0.2, 0.3, 0.25])
        t = ta.Tendrils(View(*view), opts)
        t.resize()
        t.setup(n)
        t.particles.upload_texels(cur, 0)
        t.particles.upload_texels(prev, 1)
        t.timer.time = 2500.0
        for _ in range(3):
            t.timer.tick()
            t.step().draw()
            t.screen.bind()
            t.drawFade()
            if with_program:
                t.screenShader(programs["copy"], views=[t.buffers[0]])
            else:
                t.copyBuffer(0)
            t.stepBuffers()
        got.append((t.read_view(), t.buffers[0].read()))
        t.dispose()
    (want, front), (out, front_too) = got
    assert front.any() and (want != 0).any()
    assert_bytes(front_too, front)
    assert_bytes(out, want)


def test_screen_shader_resolves_the_hosts_objects(programs):
    """colorMap, flow, an AudioTexture, a texture slot, the screen and a buffer as views; the colour map and a slot as targets;
    blend=None follows the GL state the host tracks"""
    from tendrils_amd.blend import AudioTexture
    rng = np.random.default_rng(12)
    t = make((10, 4), buffers=1)
    ctx = t.particles._ctx
    cmap, flow, bins = rng.uniform(0, 1, (3, 3, 4)).astype(F), rng.uniform(-1, 1, (4, 10, 4)).astype(F), rng.uniform(0, 1, 16).astype(F)
    slot0 = rng.uniform(0, 1, (2, 5, 4)).astype(F)
    screen, back = random_image(rng, (10, 4)), random_image(rng, (10, 4))
    t.colorMap.set_pixels(cmap)
    t.flow.set_pixels(flow)
    upload(ctx, 0, "rgba32f", slot0)
    upload(ctx, 2, "rgba32f", np.zeros((16, 24, 4), F))
    set_image(t, None, screen)
    set_image(t, t.buffers[0], back)
    audio = AudioTexture(None, bins)
    assert not t.blending                                                     # before the first step(): nothing is blended
    views = [t.colorMap, t.flow, audio, 0, t.buffers[0]]
    t.buffers[0].bind()
    with pytest.raises(ta.TendrilsHipError):                                  # (target None: the bound buffer, which is among the views)
        t.screenShader(programs["sum"], dict(n=5), views)
    views[4] = t.screen
    t.screenShader(programs["sum"], dict(n=5), views, target=2)
    want = tap_sum([("rgba32f", cmap), ("rgba32f", flow), ("l32f", bins), ("rgba32f", slot0), ("rgba8", screen)], 24, 16)
    assert_bits(read_slot(ctx, 2, (16, 24, 4)), want)
    t.screenShader(programs["fill"], dict(rgba=[0.2, 0.4, 0.6, 0.5]), target=t.colorMap)
    assert_bits(t.colorMap.read(), np.broadcast_to(np.array([0.2, 0.4, 0.6, 0.5], F), (3, 3, 4)))
    t.screenShader(programs["fill"], dict(rgba=[1.0, 1.0, 1.0, 0.5]), target=t.colorMap, blend=True)
    src = np.broadcast_to(np.array([1.0, 1.0, 1.0, 0.5], F), (3, 3, 4)).copy()
    assert_bits(t.colorMap.read(), R.blend_stage(src, True, False, np.broadcast_to(np.array([0.2, 0.4, 0.6, 0.5], F), (3, 3, 4))))
    with pytest.raises(TypeError):
        t.screenShader(programs["drift"])
    with pytest.raises(TypeError):
        t.screenShader(programs["copy"], views=[object()])
    t.dispose()


# ---- 10: a row band -------------------------------------------------------------------------------------------------------------------------
def test_a_row_band_renders_into_replicated_targets_only(programs):
    rng = np.random.default_rng(13)
    texels, before = rng.uniform(-1, 1, (5, 7, 4)).astype(F), rng.uniform(0, 1, (9, 17, 4)).astype(F)
    got = []
    for band in (dict(), dict(rows=8, row0=8, globalHeight=16)):
        t = make((16, 9), 16, **band)
        ctx = t.particles._ctx
        upload(ctx, 0, "rgba32f", texels)
        call("th_colormap_upload", ctx, before.ctypes.data_as(_capi._fp), 17, 9)
        run(ctx, programs["box"], [(TEX, 0)], TO_MAP, 0, 1)
        got.append(read_map(ctx))
        if band:
            view = t.read_view()
            status, message = status_of(ctx, programs["copy"], [(TEX, 0)], TO_VIEW, 0, 1)
            assert status == _capi.TH_ERR_UNSUPPORTED and "row-band" in message
            assert (t.read_view() == view).all()
        t.dispose()
    assert (got[0] != before).any()
    assert_bits(got[1], got[0])


# ---- 11: query, life cycle ----------------------------------------------------------------------------------------------------------------
def test_query_reports_no_scratch_and_no_lds(programs):
    t = make()
    for name in ("copy", "box"):
        info = programs[name].query(t.particles)
        assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0, (name, info)
        assert 0 < info["vgprs"] <= 512 and 0 < info["sgprs"] <= 128 and 0 < info["code_bytes"] < 16384, (name, info)
    t.dispose()


def test_a_destroyed_screen_program_keeps_running_where_it_was_loaded():
    view = (37, 23)
    under = random_image(np.random.default_rng(14), view)
    prog = ScreenProgram.from_source(FILL, Colour, name="fill_once")
    plain, t = make(view), make(view)
    for x in (plain, t):
        set_image(x, None, under)
    block = Colour(rgba=(C.c_float * 4)(0.9, 0.1, 0.4, 0.37))
    run(t.particles._ctx, prog, [], TO_VIEW, 0, 1, block)
    handle = C.c_void_p(prog.handle.value)
    prog.dispose()                                                            # th_program_destroy
    call("th_screen_run", t.particles._ctx, handle, C.byref(block), C.sizeof(block), units_table([]), 0, TO_VIEW, 0, 1)
    for _ in range(2):
        plain.drawFill(list(block.rgba))
    assert_bytes(t.read_view(), plain.read_view())
    plain.dispose(), t.dispose()


# ---- 12: the library a product host ships -----------------------------------------------------------------------------------------------------
RELEASE = os.path.join(ROOT, "tendrils_amd", "lib", "release", "libtendrils_hip.so")
CHILD = r'''
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd.particles import ScreenProgram
from tendrils_amd.tendrils import View
lib = _capi.load()
assert os.path.realpath(lib._name) == os.path.realpath(RELEASE), lib._name
assert not hasattr(lib, "th_comm_loopback_id")
prog = ScreenProgram.from_source(SOURCE, name="copy")
out = []
for with_program in (False, True):
    t = ta.Tendrils(View(37, 23), dict(numBuffers=1))
    t.resize(); t.setup(8)
    t.buffers[0].bind()
    t.drawFill([0.9, 0.1, 0.4, 0.6])
    t.screen.bind()
    t.drawFill([0.2, 0.5, 0.1, 0.7])
    if with_program:
        t.screenShader(prog, views=[t.buffers[0]], blend=True)
        assert prog.query(t.particles)["scratch_bytes"] == 0
    else:
        t.copyBuffer(0)
    out.append(t.read_view())
    t.dispose()
assert out[0].any() and (out[0] == out[1]).all()
prog.dispose()
print("release ok")
'''


def test_release_library_runs_a_screen_program():
    if not os.path.exists(RELEASE):
        subprocess.check_call(["make", "-j3", "-C", os.path.join(ROOT, "tendrils_amd", "csrc"), "release"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, TH_LIB=RELEASE)
    code = "ROOT = %r\nRELEASE = %r\nSOURCE = %r\n" % (ROOT, RELEASE, COPY) + CHILD
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "release ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
