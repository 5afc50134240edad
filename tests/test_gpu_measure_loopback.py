"""th_measure_global with MORE THAN ONE RANK on one GPU: the ranks are contexts of this process joined by the in-process
transport (th_comm_loopback_id; tests/test_gpu_loopback.py has the pattern - one host thread per rank), each holding a row band
of one texture, the bands unequal (100 rows over 3 ranks: 34 / 33 / 33).  Every rank launches its local measure, the 144-byte
blocks are all-gathered, and the library's fold folds them in rank order: every rank must return the same bytes, the exact
channels must equal the unsharded context's (and numpy's), a general sum must lie within the bound of any summation order
(tests/test_gpu_measure_program.py), and `particles` is the whole texture's texel count."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_loopback import in_threads, inputs, make, world_of
from test_gpu_measure_program import EXACT, GENERAL, RECT, WHERE, Rect, exact_channels, general_values, same_exact, within_bound

pytestmark = pytest.mark.gpu

F = np.float32
RECT_UNIFORMS = dict(x0=RECT[0], y0=RECT[1], x1=RECT[2], y1=RECT[3])


@pytest.fixture(scope="module")
def programs():
    from tendrils_amd.particles import MeasureProgram
    progs = dict(exact=MeasureProgram.from_source(EXACT, Rect, channels=3, name="exact"),
                 general=MeasureProgram.from_source(GENERAL, channels=1, name="general"),
                 where=MeasureProgram.from_source(WHERE, channels=4, name="where"))
    yield progs
    for p in progs.values():
        p.dispose()


@pytest.mark.parametrize("n,world", [(64, 2), (100, 3)])
def test_measure_global_over_loopback_with_row_bands(programs, n, world):
    view = (50, 27)
    cur, prev, base = inputs(n, view, 31 + world)
    one = make(n, view, cur, prev, base)
    want = {k: one.particles.measure(programs[k], RECT_UNIFORMS) for k in programs}
    one.dispose()
    shards = world_of(n, view, world, cur, prev, base)
    if world == 3:
        assert [t.particles.shape[1] for t in shards] == [34, 33, 33]

    def body(r):
        p = shards[r].particles
        return {k: p.measure(programs[k], RECT_UNIFORMS, everywhere=True) for k in programs}
    got, err = in_threads(world, body)
    assert err == [None] * world, err
    v = general_values(cur)
    y, x = np.mgrid[0:n, 0:n]
    where = np.stack([y, (y * n + x) % 7, np.full((n, n), n), x], -1).astype(F)
    for r in range(world):
        for k in programs:
            assert got[r][k].raw == got[0][k].raw, (r, k)                 # byte-identical blocks on every rank
            assert got[r][k].particles == n * n
        same_exact(got[r]["exact"], exact_channels(cur))
        same_exact(got[r]["where"], where)
        for k in ("exact", "where"):
            assert (got[r][k].sum == want[k].sum).all() and (got[r][k].min == want[k].min).all() and (got[r][k].max == want[k].max).all()
            assert got[r][k].taken == want[k].taken
        assert within_bound(got[r]["general"].sum[0], v)
        assert got[r]["general"].min[0] == v.min() == want["general"].min[0] and got[r]["general"].max[0] == v.max()
    # a local measure of one band is that band's alone
    local = shards[1].particles.measure(programs["where"])
    assert local.particles == n * shards[1].particles.shape[1] and local.min[0] == shards[1].particles._row0
    for t in shards:
        t.dispose()


def test_a_world_of_one_is_the_local_measure(programs):
    from tendrils_amd import _capi, sharding
    n, view = 64, (50, 27)
    cur, prev, base = inputs(n, view, 5)
    t = make(n, view, cur, prev, base)
    sharding.comm_join(t.particles._ctx, sharding.loopback_id(), 0, 1)
    assert sharding.comm_query(t.particles._ctx)["world"] == 1
    p = t.particles
    for k in programs:
        assert p.measure(programs[k], RECT_UNIFORMS, everywhere=True).raw == p.measure(programs[k], RECT_UNIFORMS).raw
    out = _capi.MeasureResult()
    _capi.call("th_measure_global", p._ctx, programs["general"].handle, None, 0, 0, C.byref(out))
    assert bytes(out) == p.measure(programs["general"]).raw and out.particles == n * n
    t.dispose()
