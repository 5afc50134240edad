"""Who owns device memory (tendrils_amd/csrc/th_mem.hpp): every buffer of a context is a member that frees itself, so a
context that is created, walked through every allocation site and destroyed leaves the device's free memory where it was.

Six such cycles; the first is the baseline (the runtime keeps memory of its own - code objects, stream pools - the first time
a path runs), and after each of the others the device's free memory is not below the baseline by more than what the library
retained BEFORE its buffers owned themselves: 0 bytes per cycle, measured with this test body against a build of that
commit (profiles/context_memory.txt holds both libraries' six readings).  A member turned back into a raw pointer that nobody
frees shows as free memory falling: with `targets` (64 KiB per whole context, 32 KiB per band - 320 KiB a cycle) leaked, free
memory stood 2 MiB - the allocator's granule - below the first cycle's from the third cycle on, and the test failed there
(the same file): the device hands memory out in granules, so a small leak shows in steps, not every cycle -
and the smallest members (a flag word, a slot order's chunk count: a few KiB a cycle) would not fill a granule within six cycles:
a leak of one of those alone is not seen here.
No allocation here is meant to fail."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, FLOW, SMALL, TINY = 64, (96, 64), (48, 48), (40, 40)
CYCLES = 6
RETAINED_BEFORE = 0          # bytes per cycle (after the first) the library kept when every pointer was freed by hand


def inputs(view, seed=3):
    rng = np.random.default_rng(seed)
    prev = np.zeros((N, N, 4), np.float32)
    prev[..., :2] = rng.uniform(-0.2, 0.2, (N, N, 2)) * [1.0, view[1] / view[0]]      # a crowded middle: lists of many pages
    prev[..., 2:] = rng.uniform(-.012, .012, (N, N, 2))
    cur = prev.copy()
    cur[..., :2] += rng.uniform(-.1, .1, (N, N, 2)).astype(np.float32)
    base = np.zeros((view[1], view[0], 4), np.float32)
    base[..., :2] = rng.uniform(-.01, .01, (view[1], view[0], 2))
    base[..., 2] = 2400.0
    return cur, prev, base


def make(fmt, band=None):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    row0, rows = band if band else (0, N)
    opts.update(row0=row0, rows=rows, globalHeight=N, stateFormat=ta._capi.TH_STATE_F16 if fmt == "f16" else ta._capi.TH_STATE_F32)
    t = ta.Tendrils(View(*FLOW), opts)
    t.resize()
    t.setup(N)
    cur, prev, base = inputs(FLOW)
    t.particles.upload_texels(cur[row0:row0 + rows], 0)
    t.particles.upload_texels(prev[row0:row0 + rows], 1)
    t.flow.set_pixels(base)
    t.timer.time, t.timer.step = 2500.0, 1000.0 / 60.0
    t.state["noiseWeight"] = 0.0005
    return t


def walk_one_context(fmt):
    """every allocation site of a whole-texture context, once"""
    from tendrils_amd import flow_line
    from tendrils_amd.spawn.geometry import GeometryBuffer
    t = make(fmt)
    t.timer.tick()
    t.step()                                                   # the single step (its `seen` bytes once draws go through the bins)
    t.step_n(4)                                                # fused: the packed flow, the statistics' partials
    assert t.particles.stats(0.01)["particles"] == N * N           # (the fold of what the fused launch took, the pinned read-back)
    t.particles.option("fuse", 0)
    t.step_n(3)                                                # a captured graph and its time arrays
    t.particles.option("fuse", 1)
    assert t.particles.stats(0.01)["particles"] == N * N           # (the plain statistics pass: a packed ring's f32 staging)
    t.setupBuffers(2)                                          # a view-buffer ring of 2
    t.particles.draw_pipeline("stream")
    t.draw()                                                   # both passes, stream-ordered: per-line and per-fragment buffers, sort scratch
    assert t.fragments > 1000
    t.particles.draw_pipeline("bins")
    for _ in range(2):                                         # both passes through the bins: pool 4 / pages 1 - the store grows, the table widens
        t.timer.tick()
        t.step().draw()
    assert t.fragments > 1000 and t.read_view(t.buffers[0]).any()
    t.stepBuffers()
    t.gl.drawingBufferWidth, t.gl.drawingBufferHeight = SMALL  # a flow resize: flow, decoded plane, view images, bins
    t.resize()
    t.flow.set_pixels(inputs(SMALL)[2])
    t.timer.tick()
    t.step().draw()
    assert t.fragments > 1000
    t.gl.drawingBufferWidth, t.gl.drawingBufferHeight = TINY   # twice as many particles as flow texels: the slots can be tile-sorted
    t.resize()
    t.flow.set_pixels(inputs(TINY)[2])
    t.particles.option("bucket", 1)
    t.particles.option("resort_steps", 2)
    for _ in range(4):                                         # the sort's storage, the slot orders, the re-sort beside a draw
        t.timer.tick()
        t.step().draw()
    assert t.fragments > 1000
    image = GeometryBuffer()
    image.shape = (32, 32)
    image.draw(t.particles, np.array([-.5, -.5, .5, -.5, 0, .5, -.2, .1, .3, .2, 0, -.4, .1, .1, .6, .6, .1, .7], np.float32),
               t.viewSize, [1, 1, 1, 1])
    assert image.read().any()
    line = (np.array([[-.5, -.3], [0, .2], [.4, -.1], [.6, .5]], np.float32), np.array([0, 10, 20, 30], np.float64), False)
    flow_line.draw_lines(t.particles._ctx, dict(flow_line.defaults(), viewSize=t.viewSize), [line])
    assert len(t.export_lines()) > 100 and len(t.export_lines(view=True)) > 100      # the trail export, both passes' lines
    t.dispose()


def in_threads(world, body):
    err = [None] * world

    def run(r):
        try:
            body(r)
        except BaseException as e:          # noqa: BLE001 - handed to the main thread
            err[r] = e
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a rank is still waiting inside a collective"
    assert err == [None] * world, err


def walk_two_bands(pipeline):
    """two 64 x 32 bands over the in-process transport: th_draw_sharded and th_spawn_sample_sharded"""
    from tendrils_amd import _capi, sharding
    world, ident = 2, sharding.loopback_id()
    shards = [make("f32", sharding.shard_rows(N, world, r)) for r in range(world)]
    in_threads(world, lambda r: sharding.comm_join(shards[r].particles._ctx, ident, r, world))
    for t in shards:
        t.particles.draw_pipeline(pipeline)
    u = _capi.SpawnSampleUniforms(time=480.0, speed=0.01, bias=0.3, flowDecay=0.005, samples=3, apply=0)
    u.spawnSize[0], u.spawnSize[1] = 0.8, 0.8
    for k in range(9):
        u.spawnMatrix[k] = float(k in (0, 4, 8))

    def body(r):
        assert sharding.draw_sharded_native(shards[r], view=True) > 100
        _capi.call("th_spawn_sample_sharded", shards[r].particles._ctx, C.byref(u), 1, -1)      # from the particle texture into the ring
    in_threads(world, body)
    for t in shards:
        t.dispose()


def test_a_context_gives_back_what_it_took(monkeypatch):
    import torch
    monkeypatch.setenv("TH_BINS_POOL", "4")
    monkeypatch.setenv("TH_BINS_PAGES", "1")
    free = []
    for _ in range(CYCLES):
        walk_one_context("f32")
        walk_one_context("f16")
        walk_two_bands("stream")
        walk_two_bands("bins")
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        print("free after cycle %d: %d bytes (%+d against cycle 1)" % (len(free), free[-1], free[-1] - free[0]))
    for k in range(1, CYCLES):
        assert free[k] >= free[0] - RETAINED_BEFORE * k, "cycle %d: %d bytes below the first cycle's free memory" % (k + 1, free[0] - free[k])
