"""The density map on the GPU (include/tendrils_hip.h "density map"; tendrils_amd/csrc/th_density.hip): the particles' count
and summed velocity on a grid over the view, in a texture slot or the spawn image.  The reference is numpy over the state in
TEXEL order - what was uploaded, or Particles.read() - evaluating the header's expressions in np.float32 and np.int64; never
the code under test.  Every accumulation of the library is an integer addition, so texels are compared bit for bit and the five
counts exactly, whatever order the ring is held in.

Shapes, particles onto grid: 5 x 3 onto 4 x 3 (15 of 64 lanes), 100 x 37 onto 7 x 5 and 97 x 61 (a ragged last workgroup; heavy
contention on 35 cells), 48 x 48 with every particle in one cell (the worst contention, sums only integers get exact) and
1024 x 600 onto 160 x 90 (614 400 slots: 300 blocks of 2048, a lane takes eight slots of each).  Beyond 768 blocks a workgroup
takes a RUN of consecutive blocks and its LDS window lives on from one to the next: 1536 x 1100 particles (825 blocks, runs of
two) in clusters of 3000 consecutive texels, so that windows open, stay, move inside a block and are flushed."""
import ctypes as C

import numpy as np
import pytest

import tendrils_amd as ta
from tendrils_amd import _capi, sharding
from tendrils_amd._capi import call
from tendrils_amd.blend import Blend
from tendrils_amd.particles import Density

from helpers import bits_equal, hashed_state, pack_state, unpack_state
from test_gpu_measure_program import SORTED_SHAPES, context, slot_order_read, sorted_buffers, step_until_sorted, tendrils

pytestmark = pytest.mark.gpu

F = np.float32
INERT = F(-1e6)
VIEW = (1.0, 0.9)                          # with positions over +-1.2: a share outside on both axes
CASES = [((5, 3), (4, 3)), ((100, 37), (7, 5)), ((100, 37), (97, 61)), ((1024, 600), (160, 90))]
COUNTS = ("particles", "live", "inside", "outside", "nonfinite_velocity")


# ---- the reference -------------------------------------------------------------------------------------------------------------
def quantum(v):
    """(q, finite) of velocity components: (int64) rint(clamp(v, -4, 4) * 2^32), ties to even; a non-finite v adds nothing"""
    v = np.asarray(v, F)
    finite = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        scaled = (np.clip(np.where(finite, v, F(0)), F(-4.0), F(4.0)) * F(4294967296.0)).astype(F)      # (exact: a power of two)
    return np.rint(scaled).astype(np.int64), finite


def classes(st, w, h, view):
    """per particle, in texel order: live, inside, cell (valid where inside)"""
    st = np.ascontiguousarray(st, F).reshape(-1, 4)
    x, y = st[:, 0], st[:, 1]
    live = ~((x == INERT) & (y == INERT))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((((x * F(view[0])) + F(1.0)) * F(0.5)) * F(w))
        fy = np.floor((((y * F(view[1])) + F(1.0)) * F(0.5)) * F(h))
        assert fx.dtype == F and fy.dtype == F
        inside = live & (fx >= F(0.0)) & (fx <= F(w - 1)) & (fy >= F(0.0)) & (fy <= F(h - 1))
    cell = np.where(inside, fy, F(0)).astype(np.int64) * w + np.where(inside, fx, F(0)).astype(np.int64)
    return live, inside, cell


def reference(st, w, h, view):
    """(texels [h, w, 4] float32, the five counts)"""
    st = np.ascontiguousarray(st, F).reshape(-1, 4)
    live, inside, cell = classes(st, w, h, view)
    at = cell[inside]
    count = np.bincount(at, minlength=w * h).astype(np.int64)
    assert count.max(initial=0) < 2 ** 32
    sums, bad = [], np.zeros(len(at), bool)
    for c in (2, 3):
        q, finite = quantum(st[inside, c])
        total = np.zeros(w * h, np.int64)
        np.add.at(total, at, np.where(finite, q, 0))
        sums.append(total)
        bad |= ~finite
    texels = np.stack([count.astype(F), (sums[0].astype(np.float64) * 2.0 ** -32).astype(F),
                       (sums[1].astype(np.float64) * 2.0 ** -32).astype(F), (count > 0).astype(F)], -1).reshape(h, w, 4)
    info = dict(particles=len(st), live=int(live.sum()), inside=int(inside.sum()), outside=int(live.sum() - inside.sum()),
                nonfinite_velocity=int(bad.sum()))
    return texels, info


def counts_of(d):
    return {k: getattr(d, k) for k in COUNTS}


def same(d, st, grid, view=VIEW):
    texels, info = reference(st, grid[0], grid[1], view)
    got = d.read()
    print("density %dx%d of %d particles: %s" % (grid[0], grid[1], info["particles"], counts_of(d)))
    assert got.shape == texels.shape
    assert counts_of(d) == info
    wrong = ~bits_equal(got, texels)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4], got[wrong][:4], texels[wrong][:4])
    return texels, info


def spread_state(w, h, seed):
    """hashed_state (positions in [-1, 1), one texel in seven inert) with the live positions scaled to about +-1.2 and the
    velocities to about +-3: a share outside the view, sums with bits all over the 2^-32 grid"""
    st = np.ascontiguousarray(hashed_state(w, seed, inert_mod=7, rows=(0, h)))
    live = ~((st[..., 0] == INERT) & (st[..., 1] == INERT))
    st[..., :2] = np.where(live[..., None], st[..., :2] * F(1.2), st[..., :2])
    st[..., 2:] = st[..., 2:] * F(300.0)
    return st


@pytest.fixture(scope="module")
def states():
    out = {}
    for w, h in sorted({shape for shape, _grid in CASES} | {(48, 48)}):
        st = spread_state(w, h, 31 + w)
        st.setflags(write=False)
        out[(w, h)] = st
    return out


# ---- 1: texel order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,grid", CASES, ids=lambda s: "%dx%d" % s)
def test_a_ring_in_texel_order_gives_numpys_bits(states, shape, grid):
    st = states[shape]
    p = context(shape, st)
    d = p.density(grid[0], grid[1], VIEW, slot=1)
    assert isinstance(d, Density)
    texels, info = same(d, st, grid)
    assert 0 < info["outside"] and info["live"] < info["particles"] and info["inside"] + info["outside"] == info["live"]
    assert texels[..., 0].sum() == info["inside"] and (texels[..., 1] != 0).any()
    assert bits_equal(p.density(grid[0], grid[1], VIEW, slot=1).read(), texels).all()      # again: the same bits
    assert bits_equal(p.read(0), st).all()                    # (the ring is as it was)
    p.dispose()


def test_every_particle_in_one_cell(states):
    st = np.array(states[(48, 48)])
    st[..., 0], st[..., 1] = F(0.3), F(-0.2)
    grid = (9, 7)
    p = context((48, 48), st)
    texels, info = same(p.density(grid[0], grid[1], VIEW), st, grid)
    assert info["inside"] == info["live"] == 48 * 48 and (texels[..., 0] > 0).sum() == 1
    # a float sum of these velocities depends on the order: the integer sum does not (and is what came back)
    vz = st[..., 2].reshape(-1)
    assert np.cumsum(vz, dtype=F)[-1] != np.cumsum(vz[::-1], dtype=F)[-1]
    p.dispose()


def test_a_run_of_blocks_keeps_moves_and_flushes_its_window():
    shape, grid, view = (1536, 1100), (640, 360), (1.0, 1.0)
    n = shape[0] * shape[1]
    assert (n + 2047) // 2048 > 768                               # (more blocks than workgroups: runs of two)
    rng = np.random.default_rng(5)
    group = np.arange(n) // 3000                                  # a cluster ends inside a block: the window has to move there
    centres = rng.uniform(-0.95, 0.95, (int(group.max()) + 1, 2))
    st = np.empty((n, 4), F)
    st[:, :2] = centres[group] + rng.normal(0.0, 0.03, (n, 2))    # sigma of ten cells: most of a cluster inside a 48-cell window, not all
    st[:, 2:] = rng.uniform(-3.0, 3.0, (n, 2))
    st[::11] = [INERT, INERT, 0, 0]
    st = st.reshape(shape[1], shape[0], 4)
    p = context(shape, st)
    texels, info = same(p.density(grid[0], grid[1], view, slot=1), st, grid, view)
    assert info["outside"] > 0 and texels[..., 0].max() > 8
    packed = context(shape, st, packed=True)
    same(packed.density(grid[0], grid[1], view), unpack_state(pack_state(st)), grid, view)
    packed.dispose()
    p.dispose()


# ---- 2: edge values planted at known texels ------------------------------------------------------------------------------------
def test_planted_edge_values_land_in_their_classes(states):
    shape, grid, view = (100, 37), (97, 61), (1.0, 1.0)
    w, h = grid
    st = np.array(states[shape])
    flat = st.reshape(-1, 4)
    below = F(1.0)
    for _ in range(8):                                           # the largest position that is still left of the right edge
        below = np.nextafter(below, F(-2.0))
        if classes(np.array([[below, 0, 0, 0]], F), w, h, view)[1][0]:
            break
    tie0, tie2 = F(2.0 ** -33), F(3 * 2.0 ** -33)
    planted = [
        (-1.0, -1.0, 0.5, 0.25),                                 # u exactly 0: cell (0, 0)
        (below, 0.5, 1.0, 1.0),                                  # the last column
        (1.0, 0.5, 1.0, 1.0),                                    # on the right edge: outside
        (0.5, 1.0, 1.0, 1.0),                                    # on the far edge of y: outside
        (np.inf, 0.0, 1.0, 1.0), (-np.inf, 0.0, 1.0, 1.0), (0.0, np.inf, 1.0, 1.0), (np.nan, 0.0, 1.0, 1.0), (0.0, np.nan, 1.0, 1.0),
        (-0.9, -0.9, np.nan, 1.0), (-0.9, -0.9, 1.0, np.inf), (-0.9, -0.9, -np.inf, np.nan),      # one particle each, whatever is not finite
        (-0.8, -0.9, 0.0, -0.0),
        (-0.7, -0.9, 5.0, -5.0),                                 # clamped to +-4
        (-0.6, -0.9, tie0, -tie0), (-0.5, -0.9, tie2, -tie2),    # ties: 0.5 -> 0, 1.5 -> 2
    ]
    flat[:] = [INERT, INERT, 0, 0]                               # alone in their cells: everyone else inert
    flat[:len(planted)] = np.array(planted, F)
    live, inside, cell = classes(st, w, h, view)
    assert list(live[:len(planted)]) == [True] * len(planted) and not live[len(planted):].any()
    assert list(inside[:len(planted)]) == [True, True] + [False] * 7 + [True] * 7
    assert cell[0] == 0 and cell[1] % w == w - 1 and below < F(1.0)
    assert not classes(np.array([[np.nextafter(below, F(2.0)), 0, 0, 0]], F), w, h, view)[1][0]
    q, finite = quantum(np.array([tie0, -tie0, tie2, -tie2, 5.0, -5.0, 0.0, -0.0, np.nan, np.inf], F))
    assert list(q[:8]) == [0, 0, 2, -2, 2 ** 34, -2 ** 34, 0, 0] and list(finite) == [True] * 8 + [False] * 2
    p = context(shape, st)
    texels, info = same(p.density(w, h, view), st, grid, view)
    assert info == dict(particles=3700, live=16, inside=9, outside=7, nonfinite_velocity=3)
    flat_t = texels.reshape(-1, 4)
    assert list(flat_t[cell[9]]) == [3.0, 1.0, 1.0, 1.0]         # three particles; only the finite components were added
    assert list(flat_t[cell[13]]) == [1.0, 4.0, -4.0, 1.0]
    assert list(flat_t[cell[14]]) == [1.0, 0.0, 0.0, 1.0] and list(flat_t[cell[15]]) == [1.0, 2.0 ** -31, -2.0 ** -31, 1.0]
    assert len({int(cell[k]) for k in (0, 1, 9, 12, 13, 14, 15)}) == 7
    # ... and among the hashed particles
    mixed = np.array(states[shape])
    mixed.reshape(-1, 4)[1000:1000 + len(planted)] = np.array(planted, F)
    p.upload_texels(mixed, 0)
    same(p.density(w, h, view), mixed, grid, view)
    p.dispose()


# ---- 3: tile-sorted slots and packed rings -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_tile_sorted_slots_give_the_bits_of_texel_order_and_stay_sorted(states, shape, view, fmt):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)                    # (velocities the integrator keeps: about +-0.01)
    t = tendrils(shape, view, st, fmt)
    p = t.particles
    step_until_sorted(t)
    is_sorted, perm_before, slots_before = slot_order_read(p, 0, fmt == "f16")
    assert is_sorted and not (perm_before == np.arange(perm_before.size)).all()
    grids = [tuple(view), (7, 5)]
    got = {}
    for b in (0, 1):
        for k, grid in enumerate(grids):
            d = p.density(grid[0], grid[1], t.viewSize, slot=2 * b + k, buffer=b)
            got[b, k] = (d, d.read())
    whole = t.density(slot=4)                                     # Tendrils.density: buffers[0] onto the flow's shape
    assert whole.shape == tuple(t.flow.shape) == tuple(view) and counts_of(whole) == counts_of(got[0, 0][0])
    assert bits_equal(whole.read(), got[0, 0][1]).all()
    again, perm_after, slots_after = slot_order_read(p, 0, fmt == "f16")
    assert again and (perm_after == perm_before).all() and (slots_after == slots_before).all()
    assert sorted_buffers(p) > 0
    if fmt == "f16":
        texels = np.zeros_like(slots_before)
        texels[perm_before] = slots_before
        decoded = unpack_state(texels).reshape(shape[1], shape[0], 4)
    for b in (0, 1):
        back = p.read(b)                                          # (texel order: from here on the ring is no longer sorted)
        if fmt == "f16" and b == 0:
            assert bits_equal(back, decoded).all()
        for k, grid in enumerate(grids):
            d, texels = got[b, k]
            want, info = reference(back, grid[0], grid[1], t.viewSize)
            assert counts_of(d) == info and info["inside"] > 0
            assert bits_equal(texels, want).all()
            same(p.density(grid[0], grid[1], t.viewSize, slot=7, buffer=b), back, grid, t.viewSize)      # ... and now in texel order
    t.dispose()


@pytest.mark.parametrize("shape,grid", [CASES[0], CASES[2], CASES[3]], ids=lambda s: "%dx%d" % s)
def test_a_packed_ring_in_texel_order(states, shape, grid):
    st = states[shape]
    p = context(shape, st, packed=True)
    decoded = unpack_state(pack_state(st))                        # what the 8-byte texels hold, by the numpy mirror of the codec
    assert bits_equal(p.read(0), decoded).all() and not bits_equal(decoded, st).all()
    same(p.density(grid[0], grid[1], VIEW), decoded, grid)
    p.dispose()


# ---- 4: read-only ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,view", SORTED_SHAPES, ids=["48x48", "100x37"])
def test_step_density_draw_leaves_the_bits_of_step_draw(states, shape, view):
    st = np.array(states[shape])
    st[..., 2:] = st[..., 2:] * F(1.0 / 300.0)
    a, b = tendrils(shape, view, st), tendrils(shape, view, st)
    for frame in range(3):
        for t in (a, b):
            t.timer.tick()
            t.step()
        before = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]      # (the twin is read as well: both take the same calls but the density)
        a.density()
        a.particles.density(13, 11, a.viewSize, slot=3, buffer=1, into="spawn_image")
        a.particles.density_async(5, 4, a.viewSize, slot=6)
        after = [slot_order_read(t.particles, k) for t in (a, b) for k in (0, 1)]
        for (s0, perm0, slots0), (s1, perm1, slots1) in zip(before, after):          # th_slot_order_read: the same thing before and after
            assert s0 == s1 and (perm0 == perm1).all() and (slots0 == slots1).all()
        for t in (a, b):
            t.draw()
        qa, qb = _capi.DrawInfo(), _capi.DrawInfo()
        call("th_draw_query", a.particles._ctx, C.byref(qa))
        call("th_draw_query", b.particles._ctx, C.byref(qb))
        assert (qa.pipeline, qa.fragments, qa.crowded_fragments) == (qb.pipeline, qb.fragments, qb.crowded_fragments)
        assert a.fragments == b.fragments > 0
        assert sorted_buffers(a.particles) == sorted_buffers(b.particles)
    assert sorted_buffers(a.particles) > 0
    assert any(s0 for s0, _perm, _slots in before)
    assert a.particles.stats(0.01) == b.particles.stats(0.01)          # (the respawned counter among them)
    assert bits_equal(a.flow.read(), b.flow.read()).all()
    assert (a.read_view() == b.read_view()).all() and a.read_view().any()
    for k in (0, 1):
        assert bits_equal(a.particles.read(k), b.particles.read(k)).all()
    a.dispose(); b.dispose()


# ---- 5: the destination ---------------------------------------------------------------------------------------------------------
def test_a_second_call_with_another_shape_leaves_exactly_the_second_grid(states):
    shape = (100, 37)
    st = states[shape]
    p = context(shape, st)
    same(p.density(97, 61, VIEW, slot=5), st, (97, 61))
    same(p.density(7, 5, VIEW, slot=5), st, (7, 5))
    same(p.density(33, 70, (0.5, 1.0), slot=5), st, (33, 70), (0.5, 1.0))
    p.dispose()


def test_the_spawn_image_receives_the_texels_a_slot_does_and_async_leaves_the_same(states):
    shape, grid = (100, 37), (31, 17)
    st = states[shape]
    p = context(shape, st)
    d = p.density(grid[0], grid[1], VIEW, slot=2)
    texels, info = same(d, st, grid)
    image = p.density(grid[0], grid[1], VIEW, slot=99, into="spawn_image")      # (the slot is ignored)
    assert counts_of(image) == info and bits_equal(image.read(), texels).all()
    # enqueue only, then the stream's end, then the 40 bytes where they landed
    address = p.density_async(grid[0], grid[1], VIEW, slot=6)
    assert address
    p.sync()
    landed = sharding.device_view(address, (5,), "<u8").cpu().numpy()
    assert [int(v) for v in landed] == [info[k] for k in COUNTS]
    assert bits_equal(Density(p, _capi.DensityInfo(), grid[0], grid[1], "texture", 6).read(), texels).all()
    p.dispose()


def colormap(p, w, h):
    out = np.empty((h, w, 4), F)
    call("th_colormap_download", p._ctx, out.ctypes.data_as(_capi._fp))
    return out


def test_a_blend_over_the_densitys_slot_equals_the_blend_over_the_uploaded_texels(states):
    shape, grid, cmap = (100, 37), (31, 17), (40, 23)
    st = states[shape]
    p = context(shape, st)
    ctx = p._ctx
    d = p.density(grid[0], grid[1], VIEW, slot=3)
    texels = np.ascontiguousarray(d.read())
    call("th_texture_upload", ctx, 5, _capi.TEX_RGBA32F, texels.ctypes.data_as(C.c_void_p), grid[0], grid[1])
    call("th_colormap_resize", ctx, cmap[0], cmap[1])
    views = (_capi.BlendView * 1)()
    views[0].source, views[0].alpha = _capi.VIEW_TEXTURE, 0.25
    pictures = []
    for slot in (3, 5):
        views[0].index = slot
        call("th_colormap_blend", ctx, views, 1, 0, 1)
        pictures.append(colormap(p, *cmap))
    assert bits_equal(pictures[0], pictures[1]).all() and pictures[0][..., 3].any()
    # the host's Blend takes the Density itself for a view
    t = tendrils((48, 48), (32, 24), np.array(states[(48, 48)]))
    dens = t.density(slot=0)
    t.colorMap.shape = [16, 12]
    Blend(None, dict(views=[dens], alphas=[0.5])).draw(t.colorMap, gl_blend=False)
    got = colormap(t.particles, 16, 12)
    want = dens_blend(reference(states[(48, 48)], 32, 24, t.viewSize)[0], 16, 12, 0.5)
    t.dispose()
    assert bits_equal(got, want).all() and got[..., 3].any()
    p.dispose()


def dens_blend(texels, w, h, alpha):
    """one RGBA32F view NEAREST at the target's texel centres, sum = (c.rgb * (c.a * alpha), c.a * alpha), stored (th_blend.hip)"""
    th, tw = texels.shape[:2]
    uvx = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    uvy = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    ix = np.clip(np.floor(uvx * F(tw)), 0, tw - 1).astype(int)
    iy = np.clip(np.floor(uvy * F(th)), 0, th - 1).astype(int)
    c = texels[iy][:, ix]
    a = (c[..., 3] * F(alpha)).astype(F)
    return np.concatenate([(c[..., :3] * a[..., None]).astype(F), a[..., None]], -1) + F(0.0)      # (the sum starts from zero)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_and_the_destination_stays(states):
    shape = (5, 3)
    p = context(shape, states[shape])
    lib, ctx = _capi.load(), p._ctx
    held = np.arange(3 * 2 * 4, dtype=F).reshape(2, 3, 4)
    image = held[::-1].copy()
    call("th_texture_upload", ctx, 2, _capi.TEX_RGBA32F, held.ctypes.data_as(C.c_void_p), 3, 2)
    call("th_spawn_image_upload", ctx, image.ctypes.data_as(_capi._fp), 3, 2)

    def uniforms(w=4, h=3, dest=_capi.VIEW_TEXTURE, slot=2, view=(1.0, 1.0)):
        u = _capi.DensityUniforms()
        u.viewSize[0], u.viewSize[1], u.w, u.h, u.dest, u.slot = view[0], view[1], w, h, dest, slot
        return u

    out, dev = _capi.DensityInfo(), C.c_void_p()
    good = uniforms()
    bad = [("null uniforms", None, 0), ("w = 0", uniforms(w=0), 0), ("h = 0", uniforms(h=0), 0), ("w < 0", uniforms(w=-4), 0),
           ("h < 0", uniforms(h=-1), 0), ("w * h > 2^22", uniforms(w=4096, h=1025), 0), ("w * h wraps", uniforms(w=65536, h=65536), 0),
           ("slot -1", uniforms(slot=-1), 0), ("slot 8", uniforms(slot=_capi.MAX_TEXTURES), 0),
           ("dest frames", uniforms(dest=_capi.VIEW_FRAMES), 0), ("dest 7", uniforms(dest=7), 0), ("dest -1", uniforms(dest=-1), 0),
           ("buffer -1", good, -1), ("buffer 2", good, 2),
           ("viewSize nan", uniforms(view=(np.nan, 1.0)), 0), ("viewSize inf", uniforms(view=(1.0, np.inf)), 0),
           ("viewSize -inf", uniforms(view=(-np.inf, 1.0)), 0)]
    for dest in (_capi.VIEW_TEXTURE, _capi.VIEW_SPAWN_IMAGE):
        for what, u, buffer in bad:
            if u is not None and u is not good and u.dest == _capi.VIEW_TEXTURE and "dest" not in what:
                u.dest = dest
            if dest == _capi.VIEW_SPAWN_IMAGE and "slot" in what:
                continue                                          # (the slot is ignored there)
            ref = None if u is None else C.byref(u)
            assert lib.th_density(ctx, ref, buffer, C.byref(out)) == _capi.TH_ERR_INVALID, what
            assert lib.th_last_error(), what
            assert lib.th_density_async(ctx, ref, buffer, C.byref(dev)) == _capi.TH_ERR_INVALID, what
    assert lib.th_density(ctx, C.byref(good), 0, None) == _capi.TH_ERR_INVALID
    assert lib.th_density(None, C.byref(good), 0, C.byref(out)) == _capi.TH_ERR_INVALID
    assert lib.th_density_async(None, C.byref(good), 0, C.byref(dev)) == _capi.TH_ERR_INVALID
    back = np.empty_like(held)
    call("th_texture_download", ctx, 2, back.ctypes.data_as(C.c_void_p))
    assert bits_equal(back, held).all()
    call("th_spawn_image_download", ctx, back.ctypes.data_as(_capi._fp))
    assert bits_equal(back, image).all()
    for slot in (0, 1, 3, 4, 5, 6, 7):                           # ... and no other slot came to hold anything
        assert lib.th_texture_download(ctx, slot, back.ctypes.data_as(C.c_void_p)) == _capi.TH_ERR_INVALID
    # the good call then replaces the 3 x 2 texture with the 4 x 3 grid
    call("th_density", ctx, C.byref(good), 0, C.byref(out))
    same(Density(p, out, 4, 3, "texture", 2), states[shape], (4, 3), (1.0, 1.0))
    p.dispose()
