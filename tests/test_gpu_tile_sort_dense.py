"""The plain re-sort of the fused launches (th_kernels.hip: tile_hist_dense_kernel, tile_scatter_dense_kernel): where all
2 * tiles + 2 sort classes fit a dense LDS histogram (kDenseTileBins = 4096) a workgroup counts them there; larger fields run
the open-addressed table as before.  Forced bucketing, a re-sort every 2 fused steps; after every sort the order is read back
(th_slot_order_read) and checked against a TH_BUCKET=0 context stepped alongside:
  perm is a bijection; every slot holds its particle's texel-order state, bit for bit; the chunk table tiles the slots without
  gaps, every chunk has one sort class and at most 4096 slots, the classes do not decrease; a slot's class is 2 * (the tile its
  particle tapped when the order was laid out) + one bit that is a property of the particle's row
for input in texel order (the first sort), in freshly sorted order, and in a stale one (40 steps at a large speed limit: a
4096-slot block then holds far more than 64 tiles), in both storage formats, with inert and NaN particles (the no-tap class).
A ring is sorted only over a field of at most half as many texels as it has particles (th_order.hip: sorting_possible), so:
  5000 and 4097 particles (a full block + a ragged one) over 64 x 32 (2 tiles, 6 classes: whole waves on one address)
  12289 particles (three blocks + one slot) over 96 x 64 (6 tiles, 14 classes)
  2049 x 2025 particles over 1920 x 1080 (4082 classes: the benchmark's field)
  2049 x 2113 particles over 2048 x 1056 (4226 classes: just above the dense cap - the table kernels run, dense_sorts stays 0)"""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal, pack_state, unpack_state

pytestmark = pytest.mark.gpu

TIME0 = 1000.0
TILE_SHIFT, CHUNK, DENSE_BINS = 5, 4096, 4096
CASES = {
    "5000_over_64x32": dict(shape=(100, 50), view=(64, 32)),
    "4097_over_64x32": dict(shape=(241, 17), view=(64, 32)),
    "12289_over_96x64": dict(shape=(12289, 1), view=(96, 64)),
    "1080p": dict(shape=(2049, 2025), view=(1920, 1080)),
    "above_the_cap": dict(shape=(2049, 2113), view=(2048, 1056)),
}


def make(case, fmt, bucket):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    shape, view = CASES[case]["shape"], CASES[case]["view"]
    opts = ta.defaults()
    opts.update(stateFormat=ta.TH_STATE_F16 if fmt == "f16" else ta.TH_STATE_F32, rows=shape[1], globalHeight=shape[1])
    t = ta.Tendrils(View(*view), opts)
    t.resize()
    t.setup(shape[0])
    assert t.particles.shape == list(shape) and t.flow.shape == list(view)
    t.state.update(damping=0.06)           # (damping * dt = 1: a velocity keeps its size, so the particles keep drifting)
    for k, v in dict(bucket=bucket, fuse=1, rebucket_steps=2).items():
        t.particles.option(k, v)
    return t


def inputs(case, fmt, view_size):
    (w, h), (fw, fh) = CASES[case]["shape"], CASES[case]["view"]
    rng = np.random.default_rng(w + 7 * h)
    st = np.empty((h, w, 4), np.float32)
    # over the whole field and a margin beyond it (taps clamp to the edge texels)
    st[..., 0] = rng.uniform(-1.1, 1.1, (h, w)) / view_size[0]
    st[..., 1] = rng.uniform(-1.1, 1.1, (h, w)) / view_size[1]
    st[..., 2:] = rng.uniform(-.03, .03, (h, w, 2))
    flat = st.reshape(-1, 4)
    some = rng.choice(flat.shape[0], flat.shape[0] // 50, replace=False)
    flat[some[::2]] = [-1e6, -1e6, 0, 0]
    flat[some[1::2], 0] = np.nan
    if fmt == "f16":
        st = unpack_state(pack_state(st))
    fl = np.zeros((fh, fw, 4), np.float32)
    fl[..., :2] = rng.uniform(-.01, .01, (fh, fw, 2))
    fl[..., 2] = TIME0 - 10.0
    return st, fl


def tiles_of(st, view_size, fw, fh):
    """th_kernels.hip: tile_key without its row bit, every operation rounded to fp32"""
    f = np.float32
    px, py = st[..., 0].ravel(), st[..., 1].ravel()
    taps = np.isfinite(px) & np.isfinite(py) & ((px != f(-1e6)) | (py != f(-1e6)))
    with np.errstate(invalid="ignore", over="ignore"):
        tx = np.clip((px * f(view_size[0]) + f(1)) * f(0.5 * fw), f(0), f(fw - 1))
        ty = np.clip((py * f(view_size[1]) + f(1)) * f(0.5 * fh), f(0), f(fh - 1))
    tx = np.where(taps, tx, 0).astype(np.int64)
    ty = np.where(taps, ty, 0).astype(np.int64)
    tiles_x = (fw + 31) >> TILE_SHIFT
    ntiles = tiles_x * ((fh + 31) >> TILE_SHIFT)
    return np.where(taps, (ty >> TILE_SHIFT) * tiles_x + (tx >> TILE_SHIFT), ntiles), ntiles


def read_order(t, fmt):
    from tendrils_amd import _capi
    n = t.particles.shape[0] * t.particles.shape[1]
    cap = n // CHUNK + 8192 + 8
    perm, chunks = np.empty(n, np.uint32), np.zeros((cap, 4), np.uint32)
    slots = np.empty((n, 2 if fmt == "f16" else 4), np.uint32)
    nchunks, is_sorted = C.c_uint32(0), C.c_int32(0)
    u32 = C.POINTER(C.c_uint32)
    _capi.call("th_slot_order_read", t.particles._ctx, 0, perm.ctypes.data_as(u32), chunks.ctypes.data_as(u32), cap, C.byref(nchunks),
               slots.ctypes.data_as(C.c_void_p), C.byref(is_sorted))
    assert is_sorted.value == 1, "the newest state is held in a tile-sorted order"
    assert 0 < nchunks.value <= cap
    state = unpack_state(slots) if fmt == "f16" else slots.view(np.float32)
    return perm, chunks[:nchunks.value], state


def check_order(t, fmt, case, at_sort, now, what):
    """at_sort / now: the texel-order state the order was laid out for / the ring's newest state (a TH_BUCKET=0 context's)"""
    (w, h), (fw, fh) = CASES[case]["shape"], CASES[case]["view"]
    n = w * h
    perm, chunks, state = read_order(t, fmt)
    assert perm.max() < n and (np.bincount(perm, minlength=n) == 1).all(), what + ": perm is no bijection"
    diff = ~bits_equal(state, now.reshape(-1, 4)[perm]).all(-1)
    assert not diff.any(), "%s: %d slots do not hold their particle's state, first slot %d" % (what, int(diff.sum()), int(np.argmax(diff)))
    start, count, key = (chunks[:, k].astype(np.int64) for k in range(3))
    assert start[0] == 0 and np.array_equal(start[1:], (start + count)[:-1]) and start[-1] + count[-1] == n, what + ": the chunks do not tile the slots"
    assert count.min() >= 1 and count.max() <= CHUNK, what + ": chunk sizes"
    assert (np.diff(key) >= 0).all(), what + ": sort classes decrease"
    tile, ntiles = tiles_of(at_sort, t.viewSize, fw, fh)
    assert key.max() <= 2 * ntiles + 1
    key_of_slot = np.repeat(key, count)                      # (one class per chunk; non-decreasing over the slots with the chunks' keys)
    wrong = (key_of_slot >> 1) != tile[perm]
    assert not wrong.any(), "%s: %d slots lie in a chunk of another tile, first slot %d" % (what, int(wrong.sum()), int(np.argmax(wrong)))
    rows_and_bits = np.unique((perm.astype(np.int64) // w) * 2 + (key_of_slot & 1))
    assert len(rows_and_bits) == len(np.unique(rows_and_bits >> 1)), what + ": the class's low bit is no property of the particle's row"
    return perm


def counters(t):
    from tendrils_amd import _capi
    info = _capi.SlotOrderInfo()
    _capi.call("th_slot_order", t.particles._ctx, C.byref(info))
    return int(info.sorts), int(t.particles.option("dense_sorts"))


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_sort_lays_out_a_valid_order_and_changes_no_result(case, fmt):
    s, r = make(case, fmt, 1), make(case, fmt, 0)
    st, fl = inputs(case, fmt, s.viewSize)
    for t in (s, r):
        t.particles.upload_texels(st)
        t.flow.set_pixels(fl)
        t.timer.time = TIME0

    def call(n):
        for t in (s, r):
            t.step_n(n)
        return r.particles.read(0).copy()

    # the first sort: input in texel order
    first = call(2)
    check_order(s, fmt, case, st, first, "first sort")
    # input in the order just laid out
    second = call(2)
    order = check_order(s, fmt, case, first, second, "sorted input")
    sorts, dense = counters(s)
    assert sorts == 2
    # 40 steps without a sort at five times the speed limit, then a sort of the stale order
    for t in (s, r):
        t.state.update(speedLimit=0.05)
        t.particles.option("rebucket_steps", 64)
    before = call(40)
    assert counters(s)[0] == 2
    for t in (s, r):
        t.particles.option("rebucket_steps", 2)
    now = call(2)
    check_order(s, fmt, case, before, now, "stale input")
    sorts, dense = counters(s)
    assert sorts == 3
    bins = 2 * tiles_of(st, s.viewSize, *CASES[case]["view"])[1] + 2
    assert dense == (sorts if bins <= DENSE_BINS else 0), "%d sort classes: which kernels counted" % bins
    assert counters(r) == (0, 0)
    if case in ("1080p", "above_the_cap"):
        # the input of the last sort really was stale: its 4096-slot blocks held particles of more than 64 tiles (the table kernels' LDS table)
        tiles = tiles_of(before, s.viewSize, *CASES[case]["view"])[0][order][:16 * CHUNK].reshape(16, CHUNK)
        assert min(len(np.unique(b)) for b in tiles) > 64
    for k in (0, 1):
        diff = ~bits_equal(s.particles.read(k), r.particles.read(k)).all(-1)
        assert not diff.any(), "ring buffer %d: %d texels differ from the TH_BUCKET=0 context's" % (k, int(diff.sum()))
    assert s.particles.stats(s.state["speedLimit"])["live"] == r.particles.stats(r.state["speedLimit"])["live"]
    s.dispose()
    r.dispose()
