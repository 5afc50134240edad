"""Planted runs: inputs for draw() in which every texel receives exactly the fragments a plan says, and in which the ORDER of
those fragments shows in the result (tests/test_planted_runs.py pins this module on the CPU restatement,
tests/test_gpu_blend_regimes.py draws the layouts below on the GPU).  numpy and the `oracle` fixture only.

Planting.  Every particle is parked at (5, 5), outside the view; a chosen one is put within 1e-3 of a texel's centre with
cur = prev + uniform(+-1e-3): its line then gives exactly one fragment, on that texel.  Only some rows of the state draw at
all (the reference's vertex lookup drifts: about half of the rows read `current` twice) - drawing_rows() finds them by
probing the restatement.

Making the order visible.  The flow pass blends dst = src*a + dst*(1 - a), a = min(|vel| / speedLimit, 1): a fragment with
a = 1 wipes out what came before it, one with a = 0 leaves dst as it is, bit for bit.  A run is ordered by stream index
(particle (row m, column i) has stream index i*H + m); for the window [w0, w0 + 64) of its positions the fragments inside
get speeds of 0.02 .. 0.2 speedLimit (each forgets little: all 64 stay in the result's bits), the fragments before it 0.2 ..
1.5 speedLimit and the fragments after it velocity 0.  K velocity sets over the same positions - the ordering kernels read keys
and places only - move the window over the whole run."""
import numpy as np

SPEED_LIMIT = 0.01
TIME = 2500.0
PARK = 5.0
WINDOW = 64
BIN = 16                     # th_bins.hip: bins of 16 x 16 texels, a texel's local index = ly * 16 + lx
BIN_CAP = 4096               # kBinCap: bins of more places are "large" (crowd_*_kernel)
RANK_MAX_RUN = 256           # kRankMaxRun = kOwnRun = kWaveRun
GIANT_RUN = 1024             # kGiantRun
CROWD_CAP = 2048             # kCrowdCap = kGiantWindow


def view_size(view):
    """Tendrils.resize(): cover_aspect(viewRes)"""
    m = max(view)
    return (m / view[0], m / view[1])


def texel_centre(view, x, y):
    """the state-space position that lands on the middle of texel (x, y)"""
    vs = view_size(view)
    return (((x + 0.5) / view[0]) * 2.0 - 1.0) / vs[0], (((y + 0.5) / view[1]) * 2.0 - 1.0) / vs[1]


def parked(n):
    st = np.zeros((n, n, 4), np.float32)
    st[..., :2] = PARK
    return st


def deposit(oracle, cur, prev, base, view, coverage=False):
    return oracle.flow_deposit(cur, prev, base, TIME, view_size=view_size(view), speedLimit=SPEED_LIMIT, coverage=coverage)


_rows = {}


def drawing_rows(oracle, n, view):
    """the rows of an n x n state whose lines draw: row r is put on texel r with cur.x = prev.x + 1e-4, and draws iff that
    texel's coverage is n (a row either draws whole or not at all at the power-of-two sizes used here: asserted)"""
    key = (n, tuple(view))
    if key not in _rows:
        fw, fh = view
        assert n <= fw * fh and n & (n - 1) == 0
        prev = parked(n)
        for r in range(n):
            prev[r, :, 0], prev[r, :, 1] = texel_centre(view, r % fw, r // fw)
        cur = prev.copy()
        cur[..., 0] += np.float32(1e-4)
        _, frags, cov = deposit(oracle, cur, prev, np.zeros((fh, fw, 4), np.float32), view, coverage=True)
        cov = cov.ravel()[:n]
        assert set(np.unique(cov)) <= {0, n} and frags == cov.sum(), np.unique(cov)
        _rows[key] = np.flatnonzero(cov == n)
    return _rows[key]


class Layout:
    """positions of both ring buffers (velocities 0) and, for every run of the plan, its particles in stream order"""

    def __init__(self, n, view, plan, cur, prev, runs, seed):
        self.n, self.view, self.plan, self.cur, self.prev, self.runs, self.seed = n, tuple(view), plan, cur, prev, runs, seed
        self.fragments = sum(length for _, length in plan)
        self.draws = max(len(windows(length)) for _, length in plan)

    def base(self):
        """the flow field every draw starts from"""
        rng = np.random.default_rng([self.seed, 7])
        return rng.uniform(-.01, .01, (self.view[1], self.view[0], 4)).astype(np.float32)


def plant(oracle, n, view, plan, ids="spread", seed=0):
    """plan: [((x, y), length)] on distinct texels.  ids says which particles make up the runs:
      "spread"          taken at random from all particles that draw: many workgroups emit into a bin, every list of it is used
      "rows"            consecutive slots of the drawing rows in texel order, run after run: a workgroup's 256 slots reserve
                        their places in one bin at a stroke, and the reservations start and end on and across the 256-place
                        page boundaries
      a list of arrays  the slot numbers m * n + i of every run, chosen by the caller
    Asserts that the restatement's coverage is the plan, and 0 elsewhere."""
    fw, fh = view
    assert len({xy for xy, _ in plan}) == len(plan) and all(0 <= x < fw and 0 <= y < fh and l > 0 for (x, y), l in plan)
    rows = drawing_rows(oracle, n, view)
    slots = (rows[:, None] * n + np.arange(n)[None, :]).ravel()          # the drawing particles, in texel order
    total = sum(length for _, length in plan)
    assert total <= slots.size, (total, slots.size)
    rng = np.random.default_rng([seed, 1])
    if isinstance(ids, str):
        assert ids in ("spread", "rows"), ids
        if ids == "spread":
            slots = rng.permutation(slots)
    else:                                      # the particles of every run, by the caller: slot numbers m * n + i
        assert [len(r) for r in ids] == [length for _, length in plan]
        chosen = np.concatenate(ids)
        assert len(set(chosen.tolist())) == total and set((chosen // n).tolist()) <= set(rows.tolist())
        slots = chosen
    prev = parked(n)
    cur = parked(n)
    runs, at = [], 0
    for (x, y), length in plan:
        mine = slots[at:at + length]
        at += length
        m, i = mine // n, mine % n
        by_stream = np.argsort(i * n + m, kind="stable")
        m, i = m[by_stream], i[by_stream]
        cx, cy = texel_centre(view, x, y)
        p = np.stack([cx + rng.uniform(-1e-3, 1e-3, length), cy + rng.uniform(-1e-3, 1e-3, length)], -1).astype(np.float32)
        d = rng.uniform(-1e-3, 1e-3, (length, 2)).astype(np.float32)
        prev[m, i, :2] = p
        cur[m, i, :2] = p + d
        runs.append((m, i))
    want = np.zeros((fh, fw), np.int64)
    for (x, y), length in plan:
        want[y, x] = length
    _, frags, cov = deposit(oracle, cur, prev, np.zeros((fh, fw, 4), np.float32), view, coverage=True)
    assert frags == total and (cov == want).all(), (frags, total, np.argwhere(cov != want)[:8])
    return Layout(n, view, list(plan), cur, prev, runs, seed)


def windows(run_length, size=WINDOW, overlap=2):
    """the starts of the windows of a run: every adjacent pair of its positions lies wholly inside one of them - and not as
    a window's last position with the first one behind it, the one pair a window does not show"""
    step = size - overlap
    starts = list(range(0, max(run_length - size, 0) + 1, step))
    if starts[-1] + size < run_length:
        starts.append(run_length - size)
    for p in range(run_length - 1):
        w = starts[min(p // step, len(starts) - 1)]
        assert w <= p and p + 1 < w + size, (run_length, p, w)
    return starts


def window_of(run_length, k):
    """[w0, w1) of the window that velocity set k shows of a run"""
    starts = windows(run_length)
    w0 = starts[k % len(starts)]
    return w0, min(w0 + WINDOW, run_length)


def velocities(layout, k, seed=0):
    """(cur, prev) of velocity set k: window k mod (windows of the run) of every run is visible"""
    rng = np.random.default_rng([layout.seed, seed, 2, k])
    cur, prev = layout.cur.copy(), layout.prev.copy()
    for (m, i), (_, length) in zip(layout.runs, layout.plan):
        w0, w1 = window_of(length, k)
        for buf in (cur, prev):
            speed = np.zeros(length)
            speed[:w0] = rng.uniform(0.2, 1.5, w0)
            speed[w0:w1] = rng.uniform(0.02, 0.2, w1 - w0)
            angle = rng.uniform(0, 2 * np.pi, length)
            buf[m, i, 2] = (speed * SPEED_LIMIT * np.cos(angle)).astype(np.float32)
            buf[m, i, 3] = (speed * SPEED_LIMIT * np.sin(angle)).astype(np.float32)
    return cur, prev


def old_recipe_velocities(layout, seed=0):
    """the velocities every crowded test drew before this module: uniform(-.012, .012)^2 against speedLimit = 0.01"""
    rng = np.random.default_rng([layout.seed, seed, 3])
    cur, prev = layout.cur.copy(), layout.prev.copy()
    for m, i in layout.runs:
        prev[m, i, 2:] = rng.uniform(-.012, .012, (len(m), 2))
        cur[m, i, 2:] = rng.uniform(-.012, .012, (len(m), 2))
    return cur, prev


def swapped_share(render, layout, cur, prev, pairs):
    """pairs: [(run, position)] - the states of the particles at `position` and `position + 1` of the run's stream order
    are exchanged (which is what blending the two in the wrong order does) and the texel rendered again: the share of the
    pairs whose swap changes its bytes.  render(cur, prev) -> image [fh, fw, 4].  Texels do not see each other, so one
    render carries one pair of every run."""
    want = render(cur, prev)
    by_run = {}
    for r, p in pairs:
        by_run.setdefault(r, []).append(p)
    seen = 0
    for j in range(max(len(v) for v in by_run.values())):
        c, q = cur.copy(), prev.copy()
        tried = []
        for r, ps in by_run.items():
            if j < len(ps):
                m, i = layout.runs[r]
                a, b = (m[ps[j]], i[ps[j]]), (m[ps[j] + 1], i[ps[j] + 1])
                for buf, src in ((c, cur), (q, prev)):
                    buf[a], buf[b] = src[b], src[a]
                tried.append(r)
        got = render(c, q)
        for r in tried:
            (x, y), _ = layout.plan[r]
            seen += got[y, x].tobytes() != want[y, x].tobytes()
    return seen / len(pairs)


def swap_sensitivity(oracle, layout, k, pairs, seed=0):
    """the share of the given adjacent pairs whose swap changes the restatement's bits of the run's flow texel, under
    velocity set k"""
    cur, prev = velocities(layout, k, seed)
    base = layout.base()
    return swapped_share(lambda c, p: deposit(oracle, c, p, base, layout.view)[0], layout, cur, prev, pairs)


# ---- the layouts of tests/test_gpu_blend_regimes.py ------------------------------------------------------------------------
def bin_texels(view, bx, by):
    """the texels of bin (bx, by) inside the view, in rising local order"""
    return [(x, y) for y in range(by * BIN, min(by * BIN + BIN, view[1])) for x in range(bx * BIN, min(bx * BIN + BIN, view[0]))]


def in_bin(view, bx, by, lengths, first=None, last=None):
    """runs of `lengths`, in rising local order, on texels dealt evenly over bin (bx, by); first / last: the texel of the
    first / last run instead"""
    tx = bin_texels(view, bx, by)
    k = len(lengths)
    picks = [tx[(2 * j + 1) * len(tx) // (2 * k)] for j in range(k)]
    if first is not None:
        picks[0] = first
    if last is not None:
        picks[-1] = last
    assert picks == sorted(picks, key=lambda t: (t[1], t[0])) and len(set(picks)) == k and set(picks) <= set(tx), picks
    return list(zip(picks, lengths))


def bins_of(view, plan):
    """{(bx, by): the run lengths of the bin in rising local order}"""
    out = {}
    for (x, y), length in sorted(plan, key=lambda r: (r[0][1], r[0][0])):
        out.setdefault((x // BIN, y // BIN), []).append(length)
    return out


def crowded_fragments(view, plan):
    """th_draw_query's crowded_fragments: the fragments of the bins of more than kBinCap places"""
    return sum(sum(v) for v in bins_of(view, plan).values() if sum(v) > BIN_CAP)


def batches(lengths):
    """bin_crowded's walk over a bin's texels (their run lengths in rising local order, empty texels left out - they change
    nothing): batches of whole texels of up to kCrowdCap fragments; a texel of more goes alone, in windows (None stands
    in front of it)"""
    out, t0 = [], 0
    while t0 < len(lengths):
        t1 = t0
        while t1 < len(lengths) and sum(lengths[t0:t1 + 1]) <= CROWD_CAP:
            t1 += 1
        if t1 > t0:
            out.append(lengths[t0:t1])
            t0 = t1
        else:
            out.append([None, lengths[t0]])
            t0 += 1
    return out


def layout_plans(view, names):
    """{name: plan} on a target of `view`; tests/test_gpu_blend_regimes.py says what each is for and asserts it.  Every
    layout has a run on texel (0, 0) and one on (fw - 1, fh - 1), and a bin in the target's partial bottom row of bins."""
    fw, fh = view
    bx1, by1 = (fw - 1) // BIN, (fh - 1) // BIN             # the last column / row of bins (partial)
    tl, br = (0, 0), (fw - 1, fh - 1)

    def corners(plan):
        used = {xy for xy, _ in plan}
        return plan + [(xy, l) for xy, l in ((tl, 2), (br, 3)) if xy not in used]
    P = {}

    def want(name):
        return name in names
    if want("A"):
        P["A"] = (in_bin(view, 0, 0, [1], first=tl) + in_bin(view, 1, 0, [255]) + in_bin(view, 2, 0, [256]) + in_bin(view, 0, 1, [256, 1])
                  + in_bin(view, 1, by1, [256] * 15 + [255]) + in_bin(view, bx1, by1, [256] * 16, last=br))
    if want("B"):
        P["B"] = in_bin(view, 0, 0, [256, 5, 5], first=tl) + in_bin(view, bx1, by1, [5, 257, 5], last=br)
    if want("C_2048"):
        P["C_2048"] = corners(in_bin(view, 1, by1, [256] * 8 + [257, 1791]))
    if want("C_2047"):
        P["C_2047"] = corners(in_bin(view, 1, by1, [256] * 7 + [255, 257, 1792]))
    if want("C_pad"):
        P["C_pad"] = (in_bin(view, 0, 0, [300, 1748], first=tl) + in_bin(view, 1, 0, [257, 1790]) + in_bin(view, 2, 0, [1025])
                      + in_bin(view, bx1, by1, [2000, 60, 5, 2000], last=br))
    if want("D"):
        P["D"] = in_bin(view, 0, 0, [3, 2049, 3], first=tl) + in_bin(view, 1, 1 if by1 > 1 else 0, [4096]) + in_bin(view, bx1, by1, [2048, 2048], last=br)
    if want("E1"):
        P["E1"] = corners(in_bin(view, 1, by1, [241] * 17))
    if want("E2"):
        P["E2"] = in_bin(view, 0, 0, [1, 255, 256, 257, 1023, 1024, 1025, 2048, 2049][::-1], first=tl) + [(br, 3)]
    if want("E3"):
        P["E3"] = in_bin(view, 0, 0, [4097], first=tl) + in_bin(view, bx1, by1, [4096, 1], last=br)
    if want("E4"):
        P["E4"] = in_bin(view, 0, 0, [256] * 16, first=tl) + in_bin(view, bx1, by1, [256] * 16 + [1], last=br)
    return P


NAMES = ("A", "B", "C_2048", "C_2047", "C_pad", "D", "E1", "E2", "E3", "E4")
LAYOUTS = {name: ((64, 36), plan) for name, plan in layout_plans((64, 36), NAMES).items()}
LAYOUTS.update({"F_" + name: ((50, 20), plan) for name, plan in layout_plans((50, 20), ("B", "E2")).items()})
STATE = 256                 # the layouts' state is 256 x 256


def planted(oracle, name, ids):
    """layout `name` planted (once per session)"""
    key = (name, ids)
    if key not in _planted:
        view, plan = LAYOUTS[name]
        _planted[key] = plant(oracle, STATE, view, plan, ids, seed=sorted(LAYOUTS).index(name) + 100)
    return _planted[key]


_planted = {}


def giant_fallback(oracle, n=2048, view=(64, 36)):
    """Case G: one texel receives every drawing particle of columns 0-3 of a 2048 x 2048 state (stream indices below 8192) and
    64 particles of column 2047 (indices from 2047 * 2048 on).  giant_part_kernel spreads its 1024 buckets over the indices
    the run holds - 4096 indices a bucket - so the first bucket holds columns 0 and 1, more than a window (kGiantWindow =
    2048): it must leave the run to crowd_blend_kernel, whose windows of stream indices start as wide and have to narrow.
    Returns (layout, the fragments in giant_part_kernel's fullest bucket, its bucket shift)."""
    rows = drawing_rows(oracle, n, view)
    ids = np.concatenate([(rows[:, None] * n + np.arange(4)[None, :]).ravel(), rows[:64] * n + (n - 1)])
    lay = plant(oracle, n, view, [((37, 21), len(ids))], [ids], seed=77)
    m, i = lay.runs[0]
    stream = i.astype(np.int64) * n + m
    width = int(stream.max() - stream.min())
    shift = 0
    while (width >> shift) >= 1024:
        shift += 1
    most = int(np.bincount((stream - stream.min()) >> shift).max())
    return lay, most, shift


def giant_sets(lay):
    """the velocity sets of case G that are drawn: the first window, two in the middle and the last"""
    return (0, lay.draws // 3, 2 * lay.draws // 3, lay.draws - 1)
