"""The colour-map blend on the GPU (th_colormap_blend and the textures it reads, tendrils_amd/csrc/th_blend.hip): against the
captures of the reference's own Blend (tests/golden/blend_*.npz) and against the restatement (tests/blend_restatement.py) -
both bit for bit: the restatement reproduces every capture exactly (tests/test_blend_restatement.py), and the HIP pass is the
same sequence of single fp32 operations."""
import ctypes as C

import numpy as np
import pytest

import blend_restatement as R
import tendrils_amd as ta
from tendrils_amd import _capi
from tendrils_amd._capi import call
from tendrils_amd.blend import AudioTexture, Blend
from tendrils_amd.optical_flow import OpticalFlow
from tendrils_amd.spawn.pixels import PixelSpawner
from tendrils_amd.tendrils import View

from helpers import bits_equal, golden, load

pytestmark = pytest.mark.gpu

F = np.float32
FORMAT = {"rgba32f": _capi.TEX_RGBA32F, "rgba8": _capi.TEX_RGBA8, "l32f": _capi.TEX_L32F}
TEX, FRAMES, IMAGE = _capi.VIEW_TEXTURE, _capi.VIEW_FRAMES, _capi.VIEW_SPAWN_IMAGE


def make(n=8, view=(16, 9), **options):
    t = ta.Tendrils(View(*view), options)
    t.resize()
    t.setup(n)
    return t


@pytest.fixture
def tendrils():
    t = make()
    yield t
    t.dispose()


def upload(ctx, slot, fmt, texels):
    t = np.ascontiguousarray(texels, np.uint8 if fmt == "rgba8" else F)
    w, h = (t.size, 1) if fmt == "l32f" else (t.shape[1], t.shape[0])
    call("th_texture_upload", ctx, slot, FORMAT[fmt], t.ctypes.data_as(C.c_void_p), w, h)


def table(views):
    tab = (_capi.BlendView * max(len(views), 1))()
    for i, (source, index, alpha) in enumerate(views):
        tab[i].source, tab[i].index, tab[i].alpha = source, index, alpha
    return tab


def read_map(ctx):
    w, h = C.c_int32(), C.c_int32()
    call("th_colormap_shape", ctx, C.byref(w), C.byref(h))
    out = np.empty((h.value, w.value, 4), F)
    call("th_colormap_download", ctx, out.ctypes.data_as(_capi._fp))
    return out


def hip_blend(ctx, views, w, h, gl_blend=True, clear=True, prefill=None):
    """the colour map of shape w x h (holding `prefill`) after one th_colormap_blend of `views` = [(source, index, alpha)]"""
    if prefill is None:
        call("th_colormap_resize", ctx, w, h)
    else:
        p = np.ascontiguousarray(prefill, F)
        call("th_colormap_upload", ctx, p.ctypes.data_as(_capi._fp), w, h)
    call("th_colormap_blend", ctx, table(views), len(views), int(gl_blend), int(clear))
    out = read_map(ctx)
    assert out.shape == (h, w, 4)
    return out


def assert_bits(got, want):
    same = bits_equal(got, want)
    assert same.all(), "%d of %d components differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])


# ---- the captures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", golden("blend"), ids=lambda p: p.split("/")[-1][:-4])
def test_hip_equals_capture_bit_for_bit(tendrils, path):
    fx = load(path)
    ctx = tendrils.particles._ctx
    views = R.fixture_views(fx)
    for k in sorted(set(int(v) for v in fx["views"])):
        fmt = {"audio": "l32f"}.get(fx["meta"]["formats"][k], fx["meta"]["formats"][k])
        upload(ctx, k, fmt, fx["tex%d" % k])
    w, h = fx["meta"]["target"]
    got = hip_blend(ctx, [(TEX, int(k), float(a)) for k, a in zip(fx["views"], fx["alphas"])], w, h,
                    fx["meta"]["glBlend"], fx["meta"]["clear"], fx.get("prefill"))
    assert_bits(got, fx["out"])
    assert_bits(got, R.blend(views, w, h, fx["meta"]["glBlend"], fx["meta"]["clear"], fx.get("prefill")))


# ---- seeded cases the captures do not cover: row tails, the grid's stride, the NEAREST clamp ---------------------------
def seeded_views(rng, w, h):
    """all three formats; one view 100 times as wide as the target, one of a single texel, texels outside 0..1"""
    return [("l32f", rng.uniform(-1, 1, 100 * w).astype(F), 0.35),
            ("rgba8", rng.integers(0, 256, (max(1, 2 * h - 1), 3 * w + 1, 4), dtype=np.uint8), 0.5),
            ("rgba32f", rng.uniform(-0.5, 1.5, (5, 7, 4)).astype(F), 0.45),
            ("rgba32f", rng.uniform(0, 1, (1, 1, 4)).astype(F), -0.2),
            ("rgba8", rng.integers(0, 256, (2 * h, 2 * w, 4), dtype=np.uint8), 0.15)]       # every tap on a texel boundary


@pytest.mark.parametrize("w,h", [(1, 1), (63, 3), (64, 1), (65, 3), (257, 3), (1031, 521)],
                         ids=lambda v: str(v))
def test_hip_equals_restatement_bit_for_bit(tendrils, w, h):
    """widths around the wave and the workgroup, one row and three; 1031 x 521 = 537 151 texels is more than the capped grid's
    2048 x 256 lanes: the grid-stride loop runs twice for some lanes"""
    rng = np.random.default_rng(1000 * w + h)
    ctx = tendrils.particles._ctx
    views = seeded_views(rng, w, h)
    for k, (fmt, texels, _) in enumerate(views):
        upload(ctx, k, fmt, texels)
    named = [(TEX, k, a) for k, (_, _, a) in enumerate(views)]
    prefill = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(F)
    src = R.shader(views, w, h)                      # (the restatement's shader stage once: the four cases share it)
    for gl_blend, clear in ((True, True), (False, True), (True, False), (False, False)):
        got = hip_blend(ctx, named, w, h, gl_blend, clear, None if clear else prefill)
        assert_bits(got, R.blend_stage(src, gl_blend, clear, prefill))
    # n = 1, every format on its own
    for k in range(3):
        got = hip_blend(ctx, [named[k]], w, h, True, True)
        assert_bits(got, R.blend([views[k]], w, h, True, True))


def test_texture_slots_keep_their_texels_and_change_shape(tendrils):
    ctx = tendrils.particles._ctx
    rng = np.random.default_rng(3)
    for fmt, texels in (("rgba8", rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)), ("l32f", rng.uniform(-1, 1, 33).astype(F)),
                        ("rgba32f", rng.uniform(0, 1, (2, 9, 4)).astype(F)), ("rgba32f", rng.uniform(0, 1, (2, 9, 4)).astype(F))):
        upload(ctx, 7, fmt, texels)                  # the same slot: another format, another shape, the same shape again
        back = np.empty_like(texels)
        call("th_texture_download", ctx, 7, back.ctypes.data_as(C.c_void_p))
        assert (back.view(np.uint8) == texels.view(np.uint8)).all()


# ---- the sources inside the context ----------------------------------------------------------------------------------------
def test_frames_and_spawn_image_blend_like_the_same_texels_as_textures(tendrils):
    ctx = tendrils.particles._ctx
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (10, 12, 4), dtype=np.uint8)
    b = rng.integers(0, 256, (10, 12, 4), dtype=np.uint8)
    image = rng.uniform(0, 1, (7, 5, 4)).astype(F)
    call("th_frames_resize", ctx, 12, 10)
    call("th_frames_upload", ctx, a.ctypes.data_as(C.POINTER(C.c_uint8)))
    call("th_frames_rotate", ctx)
    call("th_frames_upload", ctx, b.ctypes.data_as(C.POINTER(C.c_uint8)))           # buffers = [b, a]
    call("th_spawn_image_upload", ctx, image.ctypes.data_as(_capi._fp), 5, 7)
    upload(ctx, 0, "rgba8", a)
    upload(ctx, 1, "rgba8", b)
    upload(ctx, 2, "rgba32f", image)
    w, h = 17, 9
    want = hip_blend(ctx, [(TEX, 1, 0.5), (TEX, 0, 0.25), (TEX, 2, 0.3)], w, h)
    assert_bits(want, R.blend([("rgba8", b, 0.5), ("rgba8", a, 0.25), ("rgba32f", image, 0.3)], w, h))
    assert_bits(hip_blend(ctx, [(FRAMES, 0, 0.5), (FRAMES, 1, 0.25), (IMAGE, 0, 0.3)], w, h), want)
    call("th_frames_rotate", ctx)                                                    # buffers = [a, b]
    assert_bits(hip_blend(ctx, [(FRAMES, 1, 0.5), (FRAMES, 0, 0.25), (IMAGE, 99, 0.3)], w, h), want)
    assert not bits_equal(hip_blend(ctx, [(FRAMES, 0, 0.5), (FRAMES, 1, 0.25), (IMAGE, 0, 0.3)], w, h), want).all()


# ---- the consumer: the view pass looks the blended map up ---------------------------------------------------------------------
def particle_lines(rng, n, aspect):
    prev = np.zeros((n, n, 4), F)
    prev[..., :2] = rng.uniform(-0.8, 0.8, (n, n, 2)) * [1.0, aspect]
    prev[..., 2:] = rng.uniform(-.01, .01, (n, n, 2))
    cur = prev.copy()
    cur[..., :2] += rng.uniform(-.08, .08, (n, n, 2)).astype(F)
    return cur, prev


def test_view_draw_reads_the_blended_map_like_an_uploaded_one():
    n, view = 64, (64, 36)
    rng = np.random.default_rng(5)
    cur, prev = particle_lines(rng, n, 36 / 64)
    texels = rng.uniform(0, 1, (5, 7, 4)).astype(F)
    frame = rng.integers(0, 256, (6, 9, 4), dtype=np.uint8)
    images = []
    cmap = None
    for how in ("blended", "uploaded", "none"):
        t = make(n, view)
        t.state.update(speedAlpha=0.5, colorMapAlpha=0.6, baseColor=[1, 1, 1, 0.3])
        ctx = t.particles._ctx
        t.particles.upload_texels(cur, 0)
        t.particles.upload_texels(prev, 1)
        if how == "blended":
            upload(ctx, 0, "rgba32f", texels)
            upload(ctx, 1, "rgba8", frame)
            cmap = hip_blend(ctx, [(TEX, 0, 0.7), (TEX, 1, 0.6)], 13, 11)
        elif how == "uploaded":
            t.colorMap.set_pixels(cmap)
        t.timer.time = 1000.0
        t.draw()
        images.append(t.read_view())
        t.dispose()
    assert images[0].any() and (images[0] == images[1]).all()
    assert (images[0] != images[2]).any()                    # (the map shows in the view: the comparison is not empty)


# ---- what a blend leaves alone -------------------------------------------------------------------------------------------
def test_steps_around_a_blend_give_the_bits_of_steps_without_one():
    """a 64 x 64 state over a 40 x 40 flow, tile-sorted slots re-sorted every 2 steps: single steps, a fused run and its
    statistics, with blends in between - the state, the counters and the slot order are those of the run without blends"""
    n = 64
    rng = np.random.default_rng(17)
    st = np.zeros((n, n, 4), F)
    st[..., :2] = rng.uniform(-1, 1, (n, n, 2))
    st[..., 2:] = rng.uniform(-.01, .01, (n, n, 2))
    flow = np.zeros((40, 40, 4), F)
    flow[..., :2] = rng.uniform(-.01, .01, (40, 40, 2))
    flow[..., 2] = 90.0
    texels = rng.uniform(0, 1, (5, 7, 4)).astype(F)
    results = []
    for blends in (False, True):
        t = make(n, (40, 40))
        ctx = t.particles._ctx
        call("th_option_set", ctx, 0, 1)                     # TH_OPT_BUCKET: always
        call("th_option_set", ctx, 1, 2)                     # TH_OPT_RESORT_STEPS
        call("th_option_set", ctx, 2, 2)                     # TH_OPT_REBUCKET_STEPS
        t.particles.upload_texels(st)
        t.flow.set_pixels(flow)
        t.timer.time = 100.0
        upload(ctx, 0, "rgba32f", texels)
        call("th_colormap_resize", ctx, 24, 16)

        def blend():
            if blends:
                call("th_colormap_blend", ctx, table([(TEX, 0, 0.5)]), 1, 1, 1)
        blend()
        for _ in range(3):
            t.timer.tick()
            t.step()
            blend()
        t.step_n(4)
        blend()
        counters = _capi.Counters()
        call("th_stats", ctx, float(t.state["speedLimit"]), C.byref(counters))
        blend()
        t.timer.tick()
        t.step()
        order = _capi.SlotOrderInfo()
        call("th_slot_order", ctx, C.byref(order))
        results.append((t.particles.read(0), t.particles.read(1), bytes(counters), order.sorted_buffers, order.sorts))
        if blends:
            assert_bits(read_map(ctx), R.blend([("rgba32f", texels, 0.5)], 24, 16))
        t.dispose()
    (a0, a1, ac, ab, asorts), (b0, b1, bc, bb, bsorts) = results
    assert asorts > 0 and (ab, asorts) == (bb, bsorts)        # (the slot order was live)
    assert_bits(b0, a0)
    assert_bits(b1, a1)
    assert ac == bc


def test_a_blend_between_the_flow_pass_and_the_view_pass_keeps_the_line_records():
    n, view = 64, (64, 36)
    rng = np.random.default_rng(23)
    cur, prev = particle_lines(rng, n, 36 / 64)
    texels = rng.uniform(0, 1, (5, 7, 4)).astype(F)
    out = []
    for blends in (False, True):
        t = make(n, view)
        t.state.update(speedAlpha=0.5, colorMapAlpha=0.0, baseColor=[1, 0.7, 0.3, 0.3])
        ctx = t.particles._ctx
        t.particles.upload_texels(cur, 0)
        t.particles.upload_texels(prev, 1)
        t.timer.time = 1000.0
        upload(ctx, 0, "rgba32f", texels)
        u = _capi.DepositUniforms(time=1000.0, speedLimit=float(t.state["speedLimit"]))
        u.viewSize[0], u.viewSize[1] = t.viewSize
        frags, vfrags = C.c_uint64(), C.c_uint64()
        call("th_flow_deposit", ctx, C.byref(u), C.byref(frags))
        if blends:
            call("th_colormap_blend", ctx, table([(TEX, 0, 0.5)]), 1, 1, 1)
        r = t.render_uniforms()
        call("th_view_draw", ctx, C.byref(r), C.byref(vfrags))
        out.append((t.read_view(), t.flow.read(), frags.value, vfrags.value))
        t.dispose()
    assert out[0][2] == out[1][2] > 0 and out[0][3] == out[1][3] > 0
    assert (out[0][0] == out[1][0]).all() and out[0][0].any()
    assert_bits(out[1][1], out[0][1])


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_carry_a_message_and_leave_the_context_usable(tendrils):
    ctx = tendrils.particles._ctx
    texels = np.random.default_rng(2).uniform(0, 1, (3, 4, 4)).astype(F)
    upload(ctx, 0, "rgba32f", texels)
    call("th_colormap_resize", ctx, 9, 5)
    lib = _capi.load()
    eight = [(TEX, 0, 0.1)] * 8
    cases = {"no views": ([(TEX, 0, 1.0)], 0), "nine views": (eight + [(TEX, 0, 0.1)], 9), "an empty slot": ([(TEX, 3, 1.0)], 1),
             "a slot outside the table": ([(TEX, 8, 1.0)], 1), "a negative slot": ([(TEX, -1, 1.0)], 1),
             "frames not yet sized": ([(TEX, 0, 1.0), (FRAMES, 0, 1.0)], 2), "a third frame": ([(FRAMES, 2, 1.0)], 1),
             "no spawn image": ([(IMAGE, 0, 1.0)], 1), "an unknown source": ([(3, 0, 1.0)], 1)}
    for what, (views, n) in cases.items():
        status = lib.th_colormap_blend(ctx, table(views), n, 1, 1)
        assert status == 1, what                                  # TH_ERR_INVALID
        assert lib.th_last_error(), what
    assert lib.th_colormap_blend(ctx, None, 1, 1, 1) == 1 and lib.th_last_error()
    bad = np.zeros(4, F)
    for args in ((8, 0, 1, 1), (-1, 0, 1, 1), (0, 3, 1, 1), (0, 0, 0, 1), (0, 0, 1, -1), (0, 1, 65537, 1)):
        slot, fmt, w, h = args
        assert lib.th_texture_upload(ctx, slot, fmt, bad.ctypes.data_as(C.c_void_p), w, h) == 1 and lib.th_last_error(), args
    assert lib.th_texture_upload(ctx, 0, 0, None, 1, 1) == 1 and lib.th_last_error()
    assert lib.th_texture_download(ctx, 5, bad.ctypes.data_as(C.c_void_p)) == 1 and lib.th_last_error()
    assert lib.th_colormap_resize(ctx, 0, 4) == 1 and lib.th_last_error()
    # the map, the texture and the context are as they were
    assert not read_map(ctx).any()
    assert_bits(hip_blend(ctx, eight, 9, 5), R.blend([("rgba32f", texels, 0.1)] * 8, 9, 5))
    tendrils.timer.tick()
    tendrils.step()
    assert tendrils.particles.read(0).shape == (8, 8, 4)


# ---- a row band ----------------------------------------------------------------------------------------------------------------
def test_a_row_band_blends_like_a_whole_texture():
    fx = load([p for p in golden("blend") if "npot" in p][0])
    t = make(16, (16, 9), rows=6, row0=10, globalHeight=16)
    ctx = t.particles._ctx
    for k, fmt in enumerate(fx["meta"]["formats"]):
        upload(ctx, k, fmt, fx["tex%d" % k])
    got = hip_blend(ctx, [(TEX, int(k), float(a)) for k, a in zip(fx["views"], fx["alphas"])], 17, 9)
    t.dispose()
    assert_bits(got, fx["out"])


# ---- the host classes: the demo's frame loop ----------------------------------------------------------------------------------
def test_python_blend_and_audio_texture_through_two_frames(tendrils):
    first = load([p for p in golden("blend") if "first_frame" in p][0])
    demo = load([p for p in golden("blend") if "demo" in p][0])
    t = tendrils
    mic, track = AudioTexture(None, 8), AudioTexture(None, 16)
    optical_flow = OpticalFlow(t)
    optical_flow.resize([12, 10])
    optical_flow.set_pixels(demo["tex2"])
    blend = Blend(None, dict(views=[mic.texture, track.texture, optical_flow.frame(0)], alphas=[0.1, 0.3, 0.8]))
    assert blend.resolution == [1, 1]
    t.colorMap.set_pixels(np.full((2, 2, 4), 0.5, F))          # an older host copy ...
    t.colorMap.shape = [24, 16]                                # ... that colorMap.shape = shape (src/demo.main.js:504) drops
    assert not t.colorMap.read().any()
    for frame, fx in enumerate((first, demo)):
        mic.frequencies(fx["raw0"]).apply()
        track.waveform(fx["raw1"]).apply()
        blend.draw(t.colorMap)                                 # before the first step(): the GL's initial state, unblended
        assert blend.resolution == [24, 16]
        assert_bits(t.colorMap.read(), fx["out"])
        t.colorMap.bind()                                      # (a bind after a device-side blend uploads nothing older)
        assert_bits(t.colorMap.read(), fx["out"])
        t.timer.tick()
        t.step()                                               # leaves blending enabled
        assert t.blending
    # the override, a frame that has rotated, a texture named twice, the spawner's buffer
    blend.draw(t.colorMap, gl_blend=False)
    assert_bits(t.colorMap.read(), first["out"])
    optical_flow.step()
    blend.draw(t.colorMap, None, True)
    assert_bits(t.colorMap.read(), demo["out"])
    spawner = PixelSpawner()
    image = np.random.default_rng(4).uniform(0, 1, (7, 5, 4)).astype(F)
    spawner.setPixels(image)
    twice = Blend(views=[track, track, spawner.buffer], alphas=[0.2, 0.3, 0.4])
    twice.draw(t.colorMap, clear=False)
    want = R.blend([("l32f", demo["tex1"], 0.2), ("l32f", demo["tex1"], 0.3), ("rgba32f", image, 0.4)], 24, 16, True, False,
                   demo["out"])
    assert_bits(t.colorMap.read(), want)
    with pytest.raises(ValueError):
        Blend(views=[], alphas=[]).draw(t.colorMap)
    with pytest.raises(TypeError):
        Blend(views=[object()], alphas=[1]).draw(t.colorMap)
