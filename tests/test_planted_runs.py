"""tests/planted_runs.py pinned on the CPU restatement: the layouts tests/test_gpu_blend_regimes.py draws plant exactly, runs
are ordered by the stream index i*H + m, the windows cover every adjacent pair of a run, and - the condition the GPU module
rests on - exchanging two neighbours of a run inside the visible window changes the restatement's bits of the texel: a
kernel that blends them in the wrong order cannot produce the expected flow field."""
import numpy as np
import pytest

import planted_runs as pr

LENGTHS = (1, 2, 63, 64, 65, 66, 126, 127, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


@pytest.mark.parametrize("ids", ["spread", "rows"])
@pytest.mark.parametrize("name", sorted(pr.LAYOUTS))
def test_layout_plants_exactly(oracle, name, ids):
    """plant() itself asserts that the restatement's coverage is the plan and 0 elsewhere; here also: the runs are the planned
    lengths, in rising stream order, of distinct particles of rows that draw, and every layout has its two corner texels and a
    bin in the partial bottom row of bins"""
    view, plan = pr.LAYOUTS[name]
    lay = pr.planted(oracle, name, ids)
    rows = set(pr.drawing_rows(oracle, pr.STATE, view).tolist())
    seen = set()
    for (m, i), (_, length) in zip(lay.runs, plan):
        stream = i * pr.STATE + m
        assert len(m) == length and (np.diff(stream) > 0).all() and set(m.tolist()) <= rows
        seen |= set(stream.tolist())
    assert len(seen) == lay.fragments == sum(length for _, length in plan)
    texels = {xy for xy, _ in plan}
    assert (0, 0) in texels and (view[0] - 1, view[1] - 1) in texels
    assert view[1] % pr.BIN and any(by == (view[1] - 1) // pr.BIN for _, by in pr.bins_of(view, plan))
    if ids == "rows":                 # consecutive slots of the drawing rows: the first run starts the first drawing row
        m, i = lay.runs[0]
        assert m.min() == min(rows) and i.min() == 0


def test_stream_order_is_column_major_by_hand(oracle):
    """A 4 x 4 state, every particle of its drawing rows but the last of the last row on one texel, all with a = 1 (|vel| = 2
    speedLimit, the same in both buffers: the fragment's value is its particle's velocity, and it replaces what was there).
    The texel ends as the particle of greatest i*H + m - the last column of the last but one drawing row - not as the last one
    in texel order (m*W + i), the last but one column of the last drawing row."""
    n, view = 4, (64, 36)
    rows = pr.drawing_rows(oracle, n, view)
    assert len(rows) >= 2
    who = [(m, i) for m in rows for i in range(n)][:-1]
    last_stream = max(who, key=lambda p: p[1] * n + p[0])
    last_texel = max(who, key=lambda p: p[0] * n + p[1])
    assert last_stream != last_texel and last_stream == (rows[-2], n - 1)
    prev = pr.parked(n)
    cx, cy = pr.texel_centre(view, 7, 9)
    for m, i in who:
        prev[m, i] = [cx, cy, 0.02, 0.001 * (m * n + i)]
    cur = prev.copy()
    cur[..., 0] += np.float32(1e-4)
    out, frags, cov = pr.deposit(oracle, cur, prev, np.zeros((view[1], view[0], 4), np.float32), view, coverage=True)
    assert frags == len(who) == cov[9, 7]
    m, i = last_stream
    assert out[9, 7, 0] == np.float32(0.02) and out[9, 7, 1] == prev[m, i, 3] and out[9, 7, 3] == 1.0
    # ... and plant() hands a run out in that order
    lay = pr.plant(oracle, n, view, [((7, 9), len(who))], "rows", seed=1)
    m, i = lay.runs[0]
    assert (m[-1], i[-1]) == last_stream and (np.diff(i * n + m) > 0).all()


@pytest.mark.parametrize("length", LENGTHS)
def test_windows_cover_every_adjacent_pair(length):
    starts = pr.windows(length)
    assert starts[0] == 0 and starts == sorted(set(starts)) and starts[-1] + pr.WINDOW >= length
    inside = set()
    for w0 in starts:
        inside |= {p for p in range(w0, min(w0 + pr.WINDOW, length) - 1)}         # (p, p + 1) both in [w0, w0 + 64)
    assert inside == set(range(length - 1))
    assert [pr.window_of(length, k)[0] for k in range(2 * len(starts))] == starts * 2


def window_pairs(lay, k):
    """every adjacent pair wholly inside the window velocity set k shows, of every run"""
    pairs = []
    for r, (_, length) in enumerate(lay.plan):
        w0, w1 = pr.window_of(length, k)
        pairs += [(r, p) for p in range(w0, w1 - 1)]
    return pairs


def sampled_sets(lay):
    """the velocity sets that show the first, a middle and the last window of some run of the layout"""
    ks = set()
    for _, length in lay.plan:
        nw = len(pr.windows(length))
        ks |= {0, nw // 2, nw - 1}
    return sorted(ks)


@pytest.mark.parametrize("name", sorted(pr.LAYOUTS))
def test_swapped_neighbours_show_in_the_restatement(oracle, name):
    """The sensitivity condition: for the first, a middle and the last window of every run (and whatever window the other runs
    show under the same velocity set), every adjacent pair wholly inside the window is swapped: at most 1 % of the swaps may
    leave the restatement's bits of the texel as they were.  (Measured: 1 of 37 109, in E4.)"""
    lay = pr.planted(oracle, name, "spread")
    tried = missed = 0
    for k in sampled_sets(lay):
        pairs = window_pairs(lay, k)
        if not pairs:
            continue
        share = pr.swap_sensitivity(oracle, lay, k, pairs)
        tried += len(pairs)
        missed += round((1.0 - share) * len(pairs))
    print("%s: %d of %d swaps unseen" % (name, missed, tried))
    assert tried >= 60 and missed <= 0.01 * tried, (missed, tried)


@pytest.mark.parametrize("name", sorted(pr.LAYOUTS))
def test_rows_ids_are_as_sensitive(oracle, name):
    """the same condition with the particles taken as consecutive slots (neighbours in a run are then neighbours in the
    state), as the GPU module draws every layout too: the first, a middle and the last velocity set of the layout, every
    adjacent pair inside the window each run then shows, the same 1 % cap"""
    lay = pr.planted(oracle, name, "rows")
    tried = missed = 0
    for k in sorted({0, lay.draws // 2, lay.draws - 1}):
        pairs = window_pairs(lay, k)
        share = pr.swap_sensitivity(oracle, lay, k, pairs)
        tried += len(pairs)
        missed += round((1.0 - share) * len(pairs))
    print("%s rows: %d of %d swaps unseen" % (name, missed, tried))
    assert tried >= 60 and missed <= 0.01 * tried, (missed, tried)


def test_giants_fallback_layout_plants_and_shows_its_order(oracle):
    """Case G of the GPU module (planted_runs.giant_fallback, a 2048 x 2048 state): plant() asserts coverage = plan; the run
    meets the conditions it is named for - more than kGiantWindow stream indices in one of giant_part_kernel's 1024 buckets
    over the span the run holds, and in blend_texel_windows' first 4096-wide bucket - and in each of the four windows the
    GPU module draws (GIANT_SETS) eight adjacent pairs, the window's first and last among them, are swapped (a draw of the
    restatement at this size takes most of a second: a sample, not all 63): the same 1 % cap, so none may go unseen."""
    lay, most, shift = pr.giant_fallback(oracle)
    (m, i), = lay.runs
    stream = i.astype(np.int64) * lay.n + m
    assert (np.diff(stream) > 0).all() and set(m.tolist()) <= set(pr.drawing_rows(oracle, lay.n, lay.view).tolist())
    assert lay.fragments == len(stream) > pr.BIN_CAP and shift == 12 and most > pr.CROWD_CAP
    assert np.count_nonzero(stream < (1 << shift)) > pr.CROWD_CAP
    tried = missed = 0
    for k in pr.giant_sets(lay):
        w0, w1 = pr.window_of(lay.fragments, k)
        pairs = [(0, int(p)) for p in np.unique(np.linspace(w0, w1 - 2, 8).astype(int))]
        share = pr.swap_sensitivity(oracle, lay, k, pairs)
        tried += len(pairs)
        missed += round((1.0 - share) * len(pairs))
    print("G: %d of %d swaps unseen" % (missed, tried))
    assert tried == 32 and missed <= 0.01 * tried, (missed, tried)


def test_the_older_crowded_recipe_is_blind_to_the_order(oracle):
    """Why tests/test_gpu_blend_regimes.py exists.  The crowded tests that came before it (crowded() of
    tests/test_gpu_binned_draw.py and its kin) draw every velocity from uniform(-.012, .012)^2 against speedLimit = 0.01: four
    fragments in ten have a = 1 and wipe out what was blended before them, the others forget quickly.  On a run of 1025
    fragments with that recipe, the states of two neighbours in stream order exchanged at 60 positions spread evenly over the
    run: the share of swaps that change the texel's bits is at most 10 % (measured: 1 of 60, the run's last pair) - a kernel
    that orders all but the last few fragments of a long run at random passes those tests."""
    lay = pr.plant(oracle, pr.STATE, (64, 36), [((20, 10), 1025)], "spread", seed=5)
    cur, prev = pr.old_recipe_velocities(lay)
    base = np.zeros((36, 64, 4), np.float32)
    pairs = [(0, int(p)) for p in np.linspace(0, 1023, 60).astype(int)]
    share = pr.swapped_share(lambda c, p: pr.deposit(oracle, c, p, base, lay.view)[0], lay, cur, prev, pairs)
    print("older recipe: %d of %d swaps seen" % (round(share * len(pairs)), len(pairs)))
    assert share <= 0.10
