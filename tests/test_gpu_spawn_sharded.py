"""Best-sample spawning from the PARTICLE texture on row-band shards without a copy of the whole texture
(th_spawn_sample_sharded): every rank computes its taps, asks each tap's owner for that one texel, and runs the unchanged
apply / test / pick rounds over what comes back.  The ranks are contexts of this process joined by the in-process transport,
a thread each (as tests/test_gpu_loopback.py): what runs above the byte transport is what an RCCL job runs.  Every band must
equal the band of the unsharded th_spawn_sample bit for bit."""
import ctypes as C
import json
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from helpers import ROOT, bits_equal

pytestmark = pytest.mark.gpu

VIEW = (64, 36)
RING, TARGETS, FLOW = -1, -2, -3


def state(n, seed=19):
    """the state of test_particle_texture_sampling_on_shards_equals_unsharded: half the particles at rest, so that `bias`
    decides some picks"""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, n, 4), np.float32)
    st[..., :2] = rng.uniform(-1, 1, (n, n, 2))
    st[..., 2:] = rng.uniform(-.02, .02, (n, n, 2)) * (rng.random((n, n, 1)) < 0.5)
    return st


def make(n, st, band=None, fmt="f32", buffers=2):
    import tendrils_amd as ta
    from tendrils_amd.tendrils import View
    opts = ta.defaults()
    row0, rows = band if band else (0, n)
    opts.update(row0=row0, rows=rows, globalHeight=n, stateFormat=ta._capi.TH_STATE_F16 if fmt == "f16" else ta._capi.TH_STATE_F32)
    t = ta.Tendrils(View(*VIEW), opts)
    t.resize()
    t.setup(n, buffers)
    load(t, st, band)
    t.timer.time = 500.0
    return t


def load(t, st, band=None, flow=None):
    """every ring buffer back to `st` (the buffers differ a little, so that a pass reading the wrong one shows), targets cleared"""
    row0, rows = band if band else (0, st.shape[0])
    for k in range(len(t.particles.buffers)):
        t.particles.upload_texels(st[row0:row0 + rows] * np.float32(1.0 + 0.125 * k), k)
    t.targets.clear()
    if flow is not None:
        t.flow.set_pixels(flow)


def in_threads(world, body):
    """body(rank) on a thread per rank (a ctypes call releases the GIL: the ranks really meet inside the library)"""
    out, err = [None] * world, [None] * world

    def run(r):
        try:
            out[r] = body(r)
        except BaseException as e:          # noqa: BLE001 - handed to the main thread
            err[r] = e
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(300)
    assert not any(th.is_alive() for th in threads), "a rank is still waiting inside a collective"
    return out, err


def world_of(n, world, st, fmt="f32", buffers=2):
    from tendrils_amd import sharding
    ident = sharding.loopback_id()
    bands = [sharding.shard_rows(n, world, r) for r in range(world)]
    shards = [make(n, st, bands[r], fmt, buffers) for r in range(world)]
    _, err = in_threads(world, lambda r: sharding.comm_join(shards[r].particles._ctx, ident, r, world))
    assert err == [None] * world, err
    return shards, bands


def uniforms(samples, apply, time=480.0):
    from tendrils_amd import _capi
    u = _capi.SpawnSampleUniforms(time=time, speed=0.01, bias=0.3, flowDecay=0.005, samples=samples, apply=apply)
    u.spawnSize[0], u.spawnSize[1] = 0.8, 0.8
    u.jitter[0], u.jitter[1] = 0.003, 0.002
    for k in range(9):
        u.spawnMatrix[k] = float(k in (0, 4, 8))
    return u


def native(t, name, u, source, target):
    from tendrils_amd import _capi
    _capi.call(name, t.particles._ctx, C.byref(u), source, target)


def result(t, target):
    return t.targets.read() if target == TARGETS else t.particles.read(0 if target == RING else target)


def respawned(t):
    return t.particles.stats(0.01)["respawned"]


def spawner(t):
    from tendrils_amd.spawn import PixelSpawner, data_sample_frag
    sp = PixelSpawner(None, dict(shader=data_sample_frag(), buffer=t.particles.buffers[0], spawnSize=[0.8, 0.8], speed=0.01, bias=0.3))
    sp.jitter = [0.003, 0.002]
    t.timer.time = 480.0
    return sp


def check_accounting(infos, bands, n, samples):
    for q, (_, rows) in zip(infos, bands):
        assert q["taps"] == samples * rows * n and q["local_taps"] <= q["taps"]
    remote = sum(q["taps"] - q["local_taps"] for q in infos)
    assert sum(q["sent_bytes"] for q in infos) == sum(q["received_bytes"] for q in infos) == 20 * remote
    return remote


@pytest.mark.parametrize("n,world,fmt", [(96, 2, "f32"), (100, 3, "f32"), (96, 4, "f32"), (64, 2, "f16"), (100, 3, "f16"), (96, 4, "f16")])
def test_sharded_spawn_equals_unsharded_across_shapes(n, world, fmt):
    """PixelSpawner.spawn on shards that hold the job's communicator goes through th_spawn_sample_sharded by itself; n = 100 over
    3 ranks: bands of 34 / 33 / 33 rows.  Same state, uniforms and time as the gathered path's test."""
    from tendrils_amd import sharding
    st = state(n)
    whole = make(n, st, None, fmt)
    if fmt == "f16":                               # what the packed texels decode to is what everybody starts from
        st = whole.particles.read(0)
        load(whole, st)
    before = whole.particles.read(0)
    spawner(whole).spawn(whole)
    want, want_count = whole.particles.read(0), respawned(whole)
    whole.dispose()
    assert not bits_equal(want, before).all() and 0 < want_count < n * n
    shards, bands = world_of(n, world, st, fmt)
    assert [rows for _, rows in bands] == ([34, 33, 33] if (n, world) == (100, 3) else [n // world] * world)

    def body(r):
        t = shards[r]
        assert t.particles.fetches_taps(1) and not t.particles.fetches_taps(FLOW)
        spawner(t).spawn(t)
        return sharding.spawn_query(t)
    infos, err = in_threads(world, body)
    assert err == [None] * world, err
    for t, (row0, rows) in zip(shards, bands):
        assert bits_equal(t.particles.read(0), want[row0:row0 + rows]).all()
    assert sum(respawned(t) for t in shards) == want_count
    assert check_accounting(infos, bands, n, 2) > 0 and all(q["chunks"] == 1 for q in infos)
    # no hidden gather: the plain pass on a shard still wants its copy of the whole texture
    import tendrils_amd as ta
    with pytest.raises(ta.TendrilsHipError, match="th_state_gather"):
        native(shards[0], "th_spawn_sample", uniforms(2, 1), 1, RING)
    for t in shards:
        t.dispose()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_apply_modes_sample_counts_and_targets(fmt):
    """All four apply modes, 2 and 5 candidates, into the ring (the source named after the rotation), the targets texture and
    an explicit buffer, from each buffer of a ring of three - and, where source and target are the same storage, the texels
    read are still the ones from before the pass (what the same pass into another buffer makes of them)."""
    n, world = 100, 3
    st = state(n, 23)
    whole = make(n, st, None, fmt, 3)
    if fmt == "f16":
        st = whole.particles.read(0)
    shards, bands = world_of(n, world, st, fmt, 3)
    for apply in range(4):
        for samples in (2, 5):
            for source, target in ((1, RING), (2, RING), (0, TARGETS), (2, 0), (1, 2)):
                u = uniforms(samples, apply)
                load(whole, st)
                for t, band in zip(shards, bands):
                    load(t, st, band)
                count0 = [respawned(t) for t in shards], respawned(whole)
                before = result(whole, 2 if target == RING else target)          # (the ring's last buffer becomes its first)
                native(whole, "th_spawn_sample", u, source, target)
                want = result(whole, target)
                assert not bits_equal(want, before).all()
                _, err = in_threads(world, lambda r: native(shards[r], "th_spawn_sample_sharded", u, source, target))
                assert err == [None] * world, (apply, samples, source, target, err)
                for t, (row0, rows) in zip(shards, bands):
                    assert bits_equal(result(t, target), want[row0:row0 + rows]).all(), (apply, samples, source, target)
                moved = sum(respawned(t) - c for t, c in zip(shards, count0[0]))
                assert moved == respawned(whole) - count0[1]
                assert (moved > 0) == (target != TARGETS)         # (passes into `targets` count apart)
    # source and target the same storage: buffer 2 from buffer 2 == what buffer 0 from buffer 2 receives
    u = uniforms(5, 1)
    for t, band in zip(shards, bands):
        load(t, st, band)
    _, err = in_threads(world, lambda r: native(shards[r], "th_spawn_sample_sharded", u, 2, 0))
    assert err == [None] * world, err
    apart = [t.particles.read(0) for t in shards]
    for t, band in zip(shards, bands):
        load(t, st, band)
    _, err = in_threads(world, lambda r: native(shards[r], "th_spawn_sample_sharded", u, 2, 2))
    assert err == [None] * world, err
    for t, a in zip(shards, apart):
        assert bits_equal(t.particles.read(2), a).all()
    for t in shards + [whole]:
        t.dispose()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_chunks_of_five_rows_give_the_same_bits(fmt):
    """TH_OPT_SPAWN_CHUNK_ROWS = 5 over bands of 34 / 33 / 33 rows: 7 chunks (from the longest band: the same on every rank),
    the last of 4 rows on rank 0 and of 3 on the others; same bits, same taps, same bytes as the call in one piece."""
    from tendrils_amd import sharding
    n, world, samples = 100, 3, 5
    st = state(n, 29)
    shards, bands = world_of(n, world, st, fmt)
    u = uniforms(samples, 1)

    def body(r):
        native(shards[r], "th_spawn_sample_sharded", u, 1, RING)
        return sharding.spawn_query(shards[r])
    whole_infos, err = in_threads(world, body)
    assert err == [None] * world, err
    want = [t.particles.read(0) for t in shards]
    counts = [respawned(t) for t in shards]
    for t, band in zip(shards, bands):
        load(t, st, band)
        assert t.particles.option("spawn_chunk_rows", 5) == 5
    infos, err = in_threads(world, body)
    assert err == [None] * world, err
    assert [q["chunks"] for q in infos] == [-(-34 // 5)] * world == [7] * world and [q["chunks"] for q in whole_infos] == [1] * world
    assert [rows % 5 for _, rows in bands] == [4, 3, 3]
    for t, w in zip(shards, want):
        assert bits_equal(t.particles.read(0), w).all()
    assert [respawned(t) - c for t, c in zip(shards, counts)] == counts
    for a, b in zip(infos, whole_infos):
        assert {k: v for k, v in a.items() if k != "chunks"} == {k: v for k, v in b.items() if k != "chunks"}
    check_accounting(infos, bands, n, samples)
    # a chunk longer than the band, and one row at a time
    for rows_at_a_time, chunks in ((64, 1), (1, 34)):
        for t, band in zip(shards, bands):
            load(t, st, band)
            t.particles.option("spawn_chunk_rows", rows_at_a_time)
        infos, err = in_threads(world, body)
        assert err == [None] * world, err
        assert [q["chunks"] for q in infos] == [chunks] * world
        for t, w in zip(shards, want):
            assert bits_equal(t.particles.read(0), w).all()
    for t in shards:
        t.dispose()


def test_worlds_of_one_and_replicated_sources():
    """No communicator (the band is the whole texture) and a communicator of one rank: the plain local pass, taps = local_taps,
    no bytes.  TH_SOURCE_FLOW on a shard of three: the flow is replicated - th_spawn_sample from it, nothing fetched."""
    import tendrils_amd as ta
    from tendrils_amd import sharding
    n = 64
    st = state(n, 31)
    rng = np.random.default_rng(5)
    flow = np.zeros((VIEW[1], VIEW[0], 4), np.float32)
    flow[..., :2] = rng.uniform(-.01, .01, (VIEW[1], VIEW[0], 2))
    flow[..., 2] = 470.0
    u = uniforms(2, 1)
    whole = make(n, st)
    native(whole, "th_spawn_sample", u, 1, RING)
    want, want_count = whole.particles.read(0), respawned(whole)
    load(whole, st, None, flow)
    native(whole, "th_spawn_sample", uniforms(5, 0), FLOW, RING)
    want_flow = whole.particles.read(0)
    assert not bits_equal(want_flow, want).all()
    for joined in (False, True):
        load(whole, st)
        if joined:
            sharding.comm_join(whole.particles._ctx, sharding.loopback_id(), 0, 1)
            assert sharding.comm_query(whole.particles._ctx)["world"] == 1
        count = respawned(whole)
        native(whole, "th_spawn_sample_sharded", u, 1, RING)
        assert bits_equal(whole.particles.read(0), want).all() and respawned(whole) - count == want_count > 0
        assert sharding.spawn_query(whole) == dict(taps=2 * n * n, local_taps=2 * n * n, sent_bytes=0, received_bytes=0, chunks=1)
    # a band without a communicator is no world of one: the plain pass's error, naming the gather
    lone = make(n, st, (16, 16))
    with pytest.raises(ta.TendrilsHipError, match="th_state_gather"):
        native(lone, "th_spawn_sample_sharded", u, 1, RING)
    lone.dispose()
    whole.dispose()
    world = 3
    shards, bands = world_of(n, world, st)
    for t, band in zip(shards, bands):
        load(t, st, band, flow)

    def body(r):
        native(shards[r], "th_spawn_sample_sharded", uniforms(5, 0), FLOW, RING)
        return sharding.spawn_query(shards[r])
    infos, err = in_threads(world, body)
    assert err == [None] * world, err
    for t, (row0, rows), q in zip(shards, bands, infos):
        assert bits_equal(t.particles.read(0), want_flow[row0:row0 + rows]).all()
        assert q == dict(taps=5 * rows * n, local_taps=5 * rows * n, sent_bytes=0, received_bytes=0, chunks=1)
        t.dispose()


def test_a_request_outside_the_owners_band_fails_the_spawn_on_every_rank():
    """TH_OPT_INJECT_FAILURE = 5 on rank 1: the first request it sends names a texel of its OWN band.  The rank that receives
    it finds it outside its band and fails on its own; every other rank returns that a peer failed - nobody waits in a
    collective - and the next spawn of the same world works."""
    import tendrils_amd as ta
    n, world, bad = 100, 3, 1
    st = state(n, 37)
    u = uniforms(2, 1)
    whole = make(n, st)
    native(whole, "th_spawn_sample", u, 1, RING)
    want = whole.particles.read(0)
    whole.dispose()
    shards, bands = world_of(n, world, st)
    shards[bad].particles.option("inject_failure", 5)
    _, err = in_threads(world, lambda r: native(shards[r], "th_spawn_sample_sharded", u, 1, RING))
    assert all(isinstance(e, ta.TendrilsHipError) for e in err), err
    owners = [r for r in range(world) if "outside its band" in str(err[r])]
    assert len(owners) == 1 and owners[0] != bad, [str(e) for e in err]
    for r in range(world):
        if r != owners[0]:
            assert "sharded spawn: rank %d failed" % owners[0] in str(err[r]), str(err[r])
    assert shards[bad].particles.option("inject_failure") == 0
    for t, band in zip(shards, bands):
        load(t, st, band)
    _, err = in_threads(world, lambda r: native(shards[r], "th_spawn_sample_sharded", u, 1, RING))
    assert err == [None] * world, err
    for t, (row0, rows) in zip(shards, bands):
        assert bits_equal(t.particles.read(0), want[row0:row0 + rows]).all()
        t.dispose()


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_world_of_one(tmp_path):
    """Particles.spawnSampleSharded through the Node host (a communicator of one rank; PixelSpawner routed by
    Particles.shardedSpawn): the same bytes as the Python host's sharding.spawn_sample_sharded."""
    from tendrils_amd import sharding
    n = 64
    st = state(n, 41)
    st.tofile(tmp_path / "state.bin")
    script = """
    const fs = require('fs');
    const T = require('./tendrils_amd/js');
    const { PixelSpawner, dataSampleFrag } = require('./tendrils_amd/js/spawn/pixels');
    const dir = process.argv[1];
    const b = fs.readFileSync(dir + '/state.bin');
    const t = new T.Tendrils({drawingBufferWidth: %d, drawingBufferHeight: %d}, {});
    t.resize(); t.setup(%d);
    t.particles.uploadTexels(new Float32Array(b.buffer, b.byteOffset, b.length / 4));
    t.particles.commInit(T.Particles.commLoopbackId(), 0, 1);
    const auto = t.particles.fetchesTaps(1);
    t.particles.shardedSpawn = true;
    const sp = new PixelSpawner(null, {shader: dataSampleFrag(), buffer: t.particles.buffers[0], spawnSize: [0.8, 0.8], speed: 0.01, bias: 0.3});
    t.timer.time = 480 - t.timer.step;
    sp.spawn(t);
    const out = t.particles.read(0);
    fs.writeFileSync(dir + '/out.bin', Buffer.from(out.buffer, out.byteOffset, out.byteLength));
    console.log(JSON.stringify({auto, query: t.particles.spawnQuery(), chunkRows: t.particles.option('spawnChunkRows')}));
    t.dispose();
    """ % (VIEW[0], VIEW[1], n)
    r = subprocess.run([NODE, "-e", script, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert info == {"auto": False, "query": {"taps": 2 * n * n, "localTaps": 2 * n * n, "sentBytes": 0, "receivedBytes": 0, "chunks": 1}, "chunkRows": 0}
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(n, n, 4)
    t = make(n, st)
    for k in range(2):
        t.particles.upload_texels(st, k)
    sharding.comm_join(t.particles._ctx, sharding.loopback_id(), 0, 1)
    from tendrils_amd.spawn import PixelSpawner, data_sample_frag
    sp = PixelSpawner(None, dict(shader=data_sample_frag(), buffer=t.particles.buffers[0], spawnSize=[0.8, 0.8], speed=0.01, bias=0.3))
    t.timer.time = 480.0 - t.timer.step
    q = sharding.spawn_sample_sharded(t, sp)
    want = t.particles.read(0)
    t.dispose()
    assert q == dict(taps=2 * n * n, local_taps=2 * n * n, sent_bytes=0, received_bytes=0, chunks=1)
    assert not bits_equal(want, st).all() and bits_equal(got, want).all()
