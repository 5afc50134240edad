"""What the passes refuse, word for word (include/tendrils_hip.h: th_colormap_blend, th_screen_run, th_spawn_sample, th_spawn_direct,
th_program_run, th_draw_program_run), and what a pass is handed as `spawnData` whichever entry point resolves the name.  The
entry points share the host code that turns a TH_SOURCE_* / TH_VIEW_* name into memory (tendrils_amd/csrc/th_spawn.hip,
th_blend.hip, th_program.hip): every rejection is pinned by its status and its WHOLE th_last_error() text, and after every one
a valid call of the same entry point goes through.  An RGBA8 image of more than 65536 texels a side reaches no pass: th_texture_upload
refuses such a texture and th_frames_resize such frames (both pinned below), so the passes' own tap-size rule has nothing left to refuse."""
import ctypes as C

import numpy as np
import pytest

from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.particles import DrawProgram, Particles, Program, ScreenProgram

from helpers import bits_equal, hashed_state

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, UNSUPPORTED = _capi.TH_ERR_INVALID, _capi.TH_ERR_UNSUPPORTED
TEX, FRAMES, IMAGE = _capi.VIEW_TEXTURE, _capi.VIEW_FRAMES, _capi.VIEW_SPAWN_IMAGE
BUFFER, SCREEN, COLORMAP, FLOW = _capi.VIEW_BUFFER, _capi.VIEW_SCREEN, _capi.VIEW_COLORMAP, _capi.VIEW_FLOW
TO_VIEW, TO_MAP, TO_TEX = _capi.SCREEN_TARGET_VIEW, _capi.SCREEN_TARGET_COLORMAP, _capi.SCREEN_TARGET_TEXTURE
NONE, FROM_FLOW, FROM_IMAGE = _capi.TH_SOURCE_NONE, _capi.TH_SOURCE_FLOW, _capi.TH_SOURCE_IMAGE
RGBA32F_SLOT, L32F_SLOT, RGBA8_SLOT, EMPTY_SLOT = 0, 1, 2, 5
OWN_TARGET = " is the memory this pass renders into: a pass cannot sample its own target"
BIG_FRAMES = "bad frame shape %dx%d (frames are RGBA8 images: at most 65536 a side)"
BAND_GATHER = ("sampling the particle texture on a row-band shard (4 of 8 rows) reads every band: gather buffer 0 first "
               "(th_state_gather / th_state_gather_ptr)")

KEEP = """__device__ float4 th_main(const th_pass &p)
{
    return p.self;
}
"""

PAINT = """__device__ float4 th_screen(const th_screen_pass &s)
{
    return make_float4(s.uv.x, s.uv.y, 0.5f, 1.0f);
}
"""

LINES = """__device__ th_vertex th_vertex_main(const th_vertex_pass &v)
{
    th_vertex o;
    o.position = make_float2(v.state.x, v.state.y);
    o.color = v.state;
    return o;
}
"""

# the texels of spawnData one by one: lane i returns texel i of the dw x dh texture the pass was handed, tapped at the texel's
# centre; the lanes beyond it return the shape
DUMP = """__device__ float4 th_main(const th_pass &p)
{
    const float2 r = th_data_res(p);
    const int dw = (int)r.x, n = dw * (int)r.y, i = (int)p.index;
    if (i >= n) return make_float4(r.x, r.y, -1.0f, -1.0f);
    return th_data(p, ((float)(i % dw) + 0.5f) / r.x, ((float)(i / dw) + 0.5f) / r.y);
}
"""


def upload(ctx, slot, fmt, texels, w, h):
    call("th_texture_upload", ctx, slot, fmt, texels.ctypes.data_as(C.c_void_p), w, h)


@pytest.fixture(scope="module")
def programs():
    """one trivial program of each kind"""
    progs = dict(keep=Program.from_source(KEEP, name="keep"), paint=ScreenProgram.from_source(PAINT, name="paint"),
                 lines=DrawProgram.from_source(LINES, name="lines"))
    yield progs
    for p in progs.values():
        p.dispose()


@pytest.fixture
def world(programs):
    """8 x 8 particles, 3 ring buffers, f32, a 16 x 8 flow field, 2 view buffers, textures of 4 x 2 texels; a row band of the
    same texture (rows 4..7 of 8).  Fresh for every test: no frames, no spawn image"""
    rng = np.random.default_rng(5)
    whole = Particles(None, dict(shape=[8, 8]))
    whole.setup(3)
    band = Particles(None, dict(shape=[8, 4], row0=4, globalHeight=8))
    band.setup(3)
    for p in (whole, band):
        call("th_flow_resize", p._ctx, 16, 8)
    ctx = whole._ctx
    call("th_view_buffers", ctx, 2)
    upload(ctx, RGBA32F_SLOT, _capi.TEX_RGBA32F, rng.uniform(0, 1, (2, 4, 4)).astype(F), 4, 2)
    upload(ctx, L32F_SLOT, _capi.TEX_L32F, rng.uniform(0, 1, (2, 4)).astype(F), 4, 2)
    upload(ctx, RGBA8_SLOT, _capi.TEX_RGBA8, rng.integers(0, 256, (2, 4, 4)).astype(np.uint8), 4, 2)
    yield dict(whole=whole, band=band, **programs)
    whole.dispose(), band.dispose()


def refused(name, args, status, message):
    lib = _capi.load()
    got = getattr(lib, name)(*args)
    text = lib.th_last_error().decode()
    print("%s -> %d %r" % (name, got, text))
    assert (got, text) == (status, message)


def blend_args(ctx, views, n=None):
    table = (_capi.BlendView * max(len(views), 1))()
    for i, (source, index) in enumerate(views):
        table[i].source, table[i].index, table[i].alpha = source, index, 0.5
    return ctx, table, len(views) if n is None else n, 1, 1


def screen_args(ctx, prog, units=(), target=TO_VIEW, index=0):
    table = (_capi.ScreenUnit * max(len(units), 1))()
    for i, (source, index_) in enumerate(units):
        table[i].source, table[i].index = source, index_
    return ctx, prog.handle, None, 0, table, len(units), target, index, 1


def test_colormap_blend_refusals(world):
    ctx = world["whole"]._ctx
    good = (TEX, RGBA32F_SLOT)

    def check(views, message, n=None):
        refused("th_colormap_blend", blend_args(ctx, views, n), INVALID, message)
        call("th_colormap_blend", *blend_args(ctx, [good, (TEX, RGBA8_SLOT)]))

    check([(TEX, 8)], "view 0: texture slot 8 outside 0..7")
    check([(TEX, -1)], "view 0: texture slot -1 outside 0..7")
    check([good, (TEX, EMPTY_SLOT)], "view 1: texture slot 5 is empty (call th_texture_upload)")
    check([(FRAMES, 2)], "view 0: frame buffer 2 (OpticalFlow has buffers 0 and 1)")
    check([good, good, (FRAMES, 1)], "view 2: no frame buffers (call th_frames_resize)")
    check([(IMAGE, 0)], "view 0: no spawn image (call th_spawn_image_upload)")
    for source in (BUFFER, SCREEN, COLORMAP, FLOW, 7):
        check([good, (source, 0)], "view 1: unknown source %d" % source)
    check([], "a blend takes 1..8 views (got 0)")
    check([good] * 9, "a blend takes 1..8 views (got 9)")
    refused("th_colormap_blend", (ctx, None, 1, 1, 1), INVALID, "a blend takes 1..8 views (got 1)")
    call("th_colormap_blend", *blend_args(ctx, [good]))
    # the tap-size rule: an RGBA8 image of 65537 texels a side is refused where it is made, texture and frames alike
    refused("th_texture_upload", (ctx, EMPTY_SLOT, _capi.TEX_RGBA8, np.zeros(4, np.uint8).ctypes.data_as(C.c_void_p), 65537, 1),
            INVALID, "bad texture 65537x1 (an RGBA8 texture: at most 65536 a side) or null texels")
    refused("th_frames_resize", (ctx, 65537, 1), INVALID, BIG_FRAMES % (65537, 1))
    check([(FRAMES, 0)], "view 0: no frame buffers (call th_frames_resize)")          # (the refused resize made none)
    call("th_frames_resize", ctx, 4, 2)
    refused("th_frames_resize", (ctx, 1, 65537), INVALID, BIG_FRAMES % (1, 65537))
    call("th_colormap_blend", *blend_args(ctx, [(FRAMES, 0), (FRAMES, 1)]))


def test_screen_run_refusals(world):
    whole, band, paint = world["whole"], world["band"], world["paint"]
    ctx = whole._ctx

    def check(message, units=(), status=INVALID, context=ctx, valid_target=TO_VIEW, **target):
        refused("th_screen_run", screen_args(context, paint, units, **target), status, message)
        call("th_screen_run", *screen_args(context, paint, [(FLOW, 0)], target=valid_target))

    check("unit 0: texture slot 8 outside 0..7", [(TEX, 8)])
    check("unit 1: texture slot 5 is empty (call th_texture_upload)", [(FLOW, 0), (TEX, EMPTY_SLOT)])
    check("unit 0: frame buffer 2 (OpticalFlow has buffers 0 and 1)", [(FRAMES, 2)])
    check("unit 2: no frame buffers (call th_frames_resize)", [(FLOW, 0), (FLOW, 0), (FRAMES, 0)])
    check("unit 0: no frame buffers (call th_frames_resize)", [(FRAMES, 1)], context=band._ctx, valid_target=TO_MAP, target=TO_MAP)
    check("unit 0: no spawn image (call th_spawn_image_upload)", [(IMAGE, 0)])
    check("unit 0: no view buffer 2 (there are 2)", [(BUFFER, 2)])
    check("unit 1: no view buffer -1 (there are 2)", [(BUFFER, 0), (BUFFER, -1)])
    check("unit 0: unknown source 7", [(7, 0)])
    check("a screen pass takes 0..8 units (got 9) - or null units", [(FLOW, 0)] * 9)
    refused("th_frames_resize", (ctx, 65537, 1), INVALID, BIG_FRAMES % (65537, 1))
    check("unit 0: no frame buffers (call th_frames_resize)", [(FRAMES, 0)])         # (the refused resize made none)
    call("th_frames_resize", ctx, 4, 2)
    call("th_screen_run", *screen_args(ctx, paint, [(FRAMES, 0), (FRAMES, 1)]))
    # a unit that is the pass's own target
    check("unit 0 (TH_VIEW_TEXTURE 0)" + OWN_TARGET, [(TEX, RGBA32F_SLOT)], target=TO_TEX, index=RGBA32F_SLOT)
    check("unit 1 (TH_VIEW_SCREEN 0)" + OWN_TARGET, [(BUFFER, 1), (SCREEN, 0)])
    call("th_view_bind", ctx, 1)
    check("unit 0 (TH_VIEW_BUFFER 1)" + OWN_TARGET, [(BUFFER, 1)])
    call("th_view_bind", ctx, -1)
    check("unit 0 (TH_VIEW_COLORMAP 0)" + OWN_TARGET, [(COLORMAP, 0)], target=TO_MAP)
    # the texture target
    check("target: texture slot 8 outside 0..7", target=TO_TEX, index=8)
    check("target: texture slot 5 is empty (call th_texture_upload)", target=TO_TEX, index=EMPTY_SLOT)
    check("target: texture slot 1 holds a one-channel texture (a pass renders into RGBA32F or RGBA8)", target=TO_TEX, index=L32F_SLOT)
    call("th_screen_run", *screen_args(ctx, paint, [(TEX, RGBA32F_SLOT)], TO_TEX, RGBA8_SLOT))
    check("unknown screen target 3", target=3)
    # the target is looked at before the units
    check("unknown screen target -1", [(TEX, 8)], target=-1)
    check("screen pass into the view on a row-band shard (4 of 8 rows): a band's view image holds only what it owns",
          status=UNSUPPORTED, context=band._ctx, valid_target=TO_MAP)


@pytest.mark.parametrize("entry", ["th_spawn_sample", "th_spawn_direct", "th_program_run"])
def test_spawn_data_refusals(world, entry):
    whole, band, keep = world["whole"], world["band"], world["keep"]
    uniforms = _capi.SpawnSampleUniforms(samples=2, apply=1)

    def args(p, source):
        if entry == "th_program_run":
            return p._ctx, keep.handle, None, 0, source, 0
        return p._ctx, C.byref(uniforms), source, 0

    def check(p, source, message):
        refused(entry, args(p, source), INVALID, message)
        call(entry, *args(p, FROM_FLOW))

    check(whole, 99, "bad spawnData source 99")
    check(whole, 3, "bad spawnData source 3")                      # (one past the ring)
    check(whole, FROM_IMAGE, "no spawn image (call th_spawn_image_upload)")
    check(band, FROM_IMAGE, "no spawn image (call th_spawn_image_upload)")
    check(band, 0, BAND_GATHER)
    check(band, 1, BAND_GATHER.replace("buffer 0", "buffer 1"))
    if entry != "th_program_run":
        check(whole, NONE, "bad spawnData source -5")
        check(band, NONE, "bad spawnData source -5")
    else:
        call(entry, *args(whole, NONE)), call(entry, *args(band, NONE))
    for source in (0, 1, 2):
        call(entry, *args(whole, source))
    # a ring of one buffer: refused before anything is resolved (the render target 7 would be refused too)
    one = Particles(None, dict(shape=[8, 8]))
    one.setup(1)
    needs = "%s needs at least 2 state buffers (have 1)" % ("a pass" if entry == "th_program_run" else "spawn pass")
    refused(entry, args(one, FROM_FLOW)[:-1] + (7,), INVALID, needs)
    one.setup(2)
    call(entry, *args(one, FROM_FLOW))
    one.dispose()


def test_programs_of_the_wrong_kind_and_draw_programs_on_a_band(world):
    whole, band = world["whole"], world["band"]
    keep, paint, lines = world["keep"], world["paint"], world["lines"]
    state, screen, draw = "state program (th_program_compile)", "screen program (th_screen_program_compile)", "draw program (th_draw_program_compile)"
    fragments = C.c_uint64()
    refused("th_program_run", (whole._ctx, paint.handle, None, 0, NONE, 0), INVALID, "th_program_run runs a %s: 'paint' is a %s" % (state, screen))
    refused("th_program_run", (whole._ctx, lines.handle, None, 0, NONE, 0), INVALID, "th_program_run runs a %s: 'lines' is a %s" % (state, draw))
    call("th_program_run", whole._ctx, keep.handle, None, 0, NONE, 0)
    refused("th_screen_run", screen_args(whole._ctx, keep), INVALID, "th_screen_run runs a %s: 'keep' is a %s" % (screen, state))
    call("th_screen_run", *screen_args(whole._ctx, paint))
    refused("th_draw_program_run", (whole._ctx, paint.handle, None, 0, _capi.TH_PASS_FLOW, C.byref(fragments)), INVALID,
            "th_draw_program_run runs a %s: 'paint' is a %s" % (draw, screen))
    call("th_draw_program_run", whole._ctx, lines.handle, None, 0, _capi.TH_PASS_FLOW, C.byref(fragments))
    refused("th_draw_program_run", (whole._ctx, lines.handle, None, 0, 2, C.byref(fragments)), INVALID, "unknown pass 2")
    # no pass of a draw program is valid on a band: the whole texture's context runs the valid one
    refused("th_draw_program_run", (band._ctx, lines.handle, None, 0, _capi.TH_PASS_FLOW, C.byref(fragments)), UNSUPPORTED,
            "draw program on a row-band shard (4 of 8 rows): a band's pass goes through the owners' exchange, which carries the built-in stages alone")
    call("th_draw_program_run", whole._ctx, lines.handle, None, 0, _capi.TH_PASS_VIEW, C.byref(fragments))
    big = "uniform block of 1025 bytes (at most 1024)"
    block = (C.c_uint8 * 1025)()
    refused("th_program_run", (whole._ctx, keep.handle, block, 1025, NONE, 0), INVALID, big)
    call("th_program_run", whole._ctx, keep.handle, block, 1024, NONE, 0)
    refused("th_screen_run", (whole._ctx, paint.handle, block, 1025, None, 0, TO_VIEW, 0, 1), INVALID, big)
    call("th_screen_run", whole._ctx, paint.handle, block, 1024, None, 0, TO_VIEW, 0, 1)
    refused("th_draw_program_run", (whole._ctx, lines.handle, block, 1025, _capi.TH_PASS_FLOW, C.byref(fragments)), INVALID, big)
    call("th_draw_program_run", whole._ctx, lines.handle, block, 1024, _capi.TH_PASS_FLOW, C.byref(fragments))


# ---- one spawnData, whoever resolves the name ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["f32", "f16"])
def test_a_state_program_and_the_direct_spawn_are_handed_the_same_spawn_data(oracle, packed):
    """8 x 4 particles, 3 ring buffers, a 5 x 3 flow field, a 3 x 2 spawn image.  Per source: a state program writes out the
    texture it was handed as spawnData, texel by texel - the uploaded one (the ring's, as the ring format stores it) - and
    th_spawn_direct from that source gives, on the bits, what it gives from a spawn image holding THOSE texels (the image's own
    pass: the restatement's result)"""
    w, h = 8, 4
    rng = np.random.default_rng(23)
    p = Particles(None, dict(shape=[w, h], stateFormat=_capi.TH_STATE_F16 if packed else _capi.TH_STATE_F32))
    p.setup(3)
    for k in range(3):
        p.upload_texels(hashed_state(w, 31 + k)[:h], k)
    flow, image = rng.uniform(-1, 1, (3, 5, 4)).astype(F), rng.uniform(0, 1, (2, 3, 4)).astype(F)
    call("th_flow_resize", p._ctx, 5, 3)
    call("th_flow_upload", p._ctx, flow.ctypes.data_as(_capi._fp))
    call("th_spawn_image_upload", p._ctx, image.ctypes.data_as(_capi._fp), 3, 2)
    dump = Program.from_source(DUMP, name="dump")
    ring = [p.read(k) for k in range(3)]
    assert packed == any((ring[k] != hashed_state(w, 31 + k)[:h]).any() for k in range(3))
    uniforms = dict(spawnSize=(0.75, 0.5), jitter=(0.0, 0.0), speed=0.25, bias=1.0, flowDecay=0.0, spawnMatrix=(1, 0, 0, 0, 1, 0, 0, 0, 1))
    block = _capi.SpawnSampleUniforms(time=1234.5, speed=0.25, bias=1.0, samples=0, apply=0)
    block.spawnSize[0], block.spawnSize[1] = uniforms["spawnSize"]
    for k, v in enumerate(uniforms["spawnMatrix"]):
        block.spawnMatrix[k] = v
    want_u = oracle.spawn_sample_uniforms(w, h, 1234.5, 0, 0, **uniforms)
    got = np.empty((h, w, 4), F)
    def direct(source):
        call("th_spawn_direct", p._ctx, C.byref(block), source, _capi.TH_TARGET_TARGETS)
        out = np.empty((h, w, 4), F)
        call("th_targets_download", p._ctx, out.ctypes.data_as(_capi._fp))
        return out

    assert bits_equal(direct(FROM_IMAGE), oracle.spawn_direct(want_u, image)).all()
    for source, data in ((FROM_IMAGE, image), (FROM_FLOW, flow), (0, ring[0]), (1, ring[1]), (2, ring[2])):
        dh, dw = data.shape[:2]
        call("th_program_run", p._ctx, dump.handle, None, 0, source, _capi.TH_TARGET_TARGETS)
        call("th_targets_download", p._ctx, got.ctypes.data_as(_capi._fp))
        lanes = got.reshape(-1, 4)
        seen = np.ascontiguousarray(lanes[:dw * dh].reshape(dh, dw, 4))
        assert bits_equal(seen, data).all(), source
        assert (lanes[dw * dh:] == np.array([dw, dh, -1, -1], F)).all(), source
        from_source = direct(source)
        call("th_spawn_image_upload", p._ctx, seen.ctypes.data_as(_capi._fp), dw, dh)
        assert bits_equal(from_source, direct(FROM_IMAGE)).all(), source
        assert (from_source[..., 2:] != 0).any(), source
    for k in range(3):                                            # (the passes into `targets` left the ring alone)
        assert bits_equal(p.read(k), ring[k]).all()
    dump.dispose()
    p.dispose()
