"""Best-sample spawning from the particle texture on row-band shards: the gathered path (th_state_gather + th_spawn_sample)
against th_spawn_sample_sharded, at worlds of 1 / 2 / 4 ranks ON ONE GPU - the ranks are contexts of this process joined by
the in-process transport, a host thread each, so what travels between them are device-to-device copies on one card: they
stand in for xGMI and say nothing about it.  No multi-GPU figure exists.  What the numbers do show: the kernels' and the
host round trips' cost of either path, and the bytes each rank would put on the links (th_spawn_query against the
all-gather's width x global_height x 16 x (P - 1) / P).

Per shape and world: the context's event timer around the call(s) on every rank, a barrier before each repetition, the
slowest rank of a repetition, the median over the repetitions after two warm-up rounds of both paths."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tendrils_amd as ta  # noqa: E402
from tendrils_amd import _capi, sharding  # noqa: E402
from tendrils_amd.tendrils import View  # noqa: E402

REPS = int(os.environ.get("TH_REPS", "7"))
SAMPLES = int(os.environ.get("TH_SAMPLES", "2"))            # data-sample.frag: the demo's spawnFastest
SHAPES = [int(v) for v in (sys.argv[1:] or ["4096", "8192"])]   # N x N particles; 8192: config 4


def band_state(n, row0, rows, seed):
    rng = np.random.default_rng(seed + row0)
    st = np.zeros((rows, n, 4), np.float32)
    st[..., :2] = rng.uniform(-1, 1, (rows, n, 2))
    st[..., 2:] = rng.uniform(-.02, .02, (rows, n, 2)) * (rng.random((rows, n, 1)) < 0.5)
    return st


def uniforms():
    u = _capi.SpawnSampleUniforms(time=480.0, speed=0.01, bias=0.3, flowDecay=0.005, samples=SAMPLES, apply=1)
    u.spawnSize[0], u.spawnSize[1] = 0.8, 0.8
    u.jitter[0], u.jitter[1] = 0.003, 0.002
    for k in range(9):
        u.spawnMatrix[k] = float(k in (0, 4, 8))
    return u


def run(n, world):
    ident = sharding.loopback_id()
    shards = []
    for r in range(world):
        row0, rows = sharding.shard_rows(n, world, r)
        opts = ta.defaults()
        opts.update(row0=row0, rows=rows, globalHeight=n)
        t = ta.Tendrils(View(64, 36), opts)
        t.resize(); t.setup(n)
        st = band_state(n, row0, rows, 7)
        t.particles.upload_texels(st, 0); t.particles.upload_texels(st, 1)
        shards.append(t)
    meet = threading.Barrier(world)
    times = {"gathered": [[0.0] * world for _ in range(REPS)], "fetched": [[0.0] * world for _ in range(REPS)]}
    infos, errors = [None] * world, [None] * world
    u = uniforms()

    def rank(r):
        try:
            ctx = shards[r].particles._ctx
            sharding.comm_join(ctx, ident, r, world)
            ms = C.c_float()

            def gathered():
                if world > 1:
                    _capi.call("th_state_gather", ctx, 0)           # (buffers[0] is the pass's ring[1] after the rotation)
                _capi.call("th_spawn_sample", ctx, C.byref(u), 1, -1)

            def fetched():
                _capi.call("th_spawn_sample_sharded", ctx, C.byref(u), 1, -1)
            for rep in range(-2, REPS):                            # two warm-up rounds of both, then alternating
                for name, call in (("gathered", gathered), ("fetched", fetched)):
                    _capi.call("th_sync", ctx)
                    meet.wait()
                    _capi.call("th_timer_start", ctx)
                    call()
                    _capi.call("th_timer_stop", ctx, C.byref(ms))
                    if rep >= 0:
                        times[name][rep][r] = ms.value
            infos[r] = sharding.spawn_query(shards[r])
        except BaseException as e:      # noqa: BLE001
            errors[r] = e
            meet.abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in shards:
        t.dispose()
    if any(errors):
        raise next(e for e in errors if e)
    out = {"n": n, "world": world, "samples": SAMPLES}
    for name, reps in times.items():
        slowest = [max(rep) for rep in reps]
        out[name + "_ms"] = round(float(np.median(slowest)), 3)
        out[name + "_ms_min_max"] = [round(min(slowest), 3), round(max(slowest), 3)]
    out["gather_bytes_per_rank"] = [n * (n - sharding.shard_rows(n, world, r)[1]) * 16 for r in range(world)]
    out["gather_copy_bytes"] = n * n * 16 if world > 1 else 0
    out["fetched_sent_bytes"] = [q["sent_bytes"] for q in infos]
    out["fetched_received_bytes"] = [q["received_bytes"] for q in infos]
    out["local_taps_share"] = [round(q["local_taps"] / max(q["taps"], 1), 4) for q in infos]
    out["chunks"] = infos[0]["chunks"]
    return out


if __name__ == "__main__":
    for n in SHAPES:
        for world in (1, 2, 4):
            print(json.dumps(run(n, world)), flush=True)
