"""The primitives every pipeline shares - launch_exclusive_scan_u32, launch_texel_set_rank, launch_radix_sort_u32 / _u64
(th_sort.hip) and block_scan (th_math.hpp) - against plain numpy, exactly, at the sizes where their regimes change.  They run through the
test-only harness of tests/native/, which is linked against the shipped object (tests/prims.py); every device
buffer has guard words behind its stated size and a changed guard fails the call.

An empty bit range (end_bit == begin_bit) is outside the sort's contract and is not tested (th_kernels.hpp)."""
import zlib

import numpy as np
import pytest

import prims

pytestmark = pytest.mark.gpu

M = 1 << 20


def first_difference(got, want, block):
    """'' when equal, else the first differing index with its place in units of `block` (name, size) pairs"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    where = ", ".join("%s %d" % (name, i // size) for name, size in block)
    return "%d of %d differ, first at index %d (%s): got %d, reference %d" % (bad.size, got.size, i, where, got[i], want[i])


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- exclusive scan -------------------------------------------------------------------------------------------------------
# up to 1024 block sums (n <= 2^20) a thread of sort_scan_sums_kernel holds at most one; above, a contiguous share of
# per >= 2 - and at 2^20 + 1025 (1026 sums, per = 2: 513 threads at work) the last threads' shares are empty
SCAN_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, M - 1, M, M + 1, M + 1025, 3 * M + 7]


def scan_contents(kind, n):
    rng = np.random.default_rng(seed_of("scan", kind, n))
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "counts":                 # what the sort scans: small counts, many zeros
        return rng.integers(0, 5, n, dtype=np.uint32) * (rng.random(n) < 0.6)
    if kind == "wrap":                   # the running sum passes 2^32 (several times where n allows)
        return rng.integers(0x30000000, 0xffffffff, n, dtype=np.uint32, endpoint=True)
    if kind == "last":                   # all zeros but the last word
        a = np.zeros(n, np.uint32)
        a[-1] = 0xdeadbeef
        return a
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["ones", "counts", "wrap", "last"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_equals_the_running_sum(n, kind):
    data = scan_contents(kind, n).astype(np.uint32)
    if kind == "wrap" and n >= 8:
        assert int(data.astype(np.uint64).sum()) >= 1 << 32
    got = prims.exclusive_scan_u32(data)
    diff = first_difference(got, prims.scan_reference(data), [("block of 1024", 1024), ("run of 1024 blocks", 1024 * 1024)])
    assert not diff, "scan of %d words (%s): %s" % (n, kind, diff)


# ---- the rank of a texel set ----------------------------------------------------------------------------------------------
# either side of the scan's 1024-word block; the texel count is no multiple of 64: the last word holds 36 texels, the bits past
# them are clear and must stay uncounted
def texel_set_mask(kind, nwords):
    texels = 64 * (nwords - 1) + 36
    bits = np.zeros(64 * nwords, np.uint8)
    if kind == "full":
        bits[:texels] = 1
    elif kind == "random":
        bits[:texels] = np.random.default_rng(seed_of("texel set", nwords)).random(texels) < 0.3
    elif kind == "last":                 # only the last valid bit
        bits[texels - 1] = 1
    elif kind != "empty":
        raise KeyError(kind)
    return np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1), texels


@pytest.mark.parametrize("counted", [False, True], ids=["counts", "counted"])
@pytest.mark.parametrize("kind", ["empty", "full", "random", "last"])
@pytest.mark.parametrize("nwords", [1, 2, 1023, 1024, 1025])
def test_texel_set_rank_is_the_scan_of_the_popcounts(nwords, kind, counted):
    mask, texels = texel_set_mask(kind, nwords)
    assert mask.shape == (nwords,) and int(mask[-1]) >> 36 == 0
    want, members = prims.texel_set_reference(mask)
    assert members == dict(empty=0, full=texels, last=1).get(kind, members)
    given = None
    if counted:
        # counts that are NOT the mask's popcounts (each one more, the first 7 more): a launcher that counted all the same would
        # scan the popcounts and differ in every word behind the first
        given = (np.unpackbits(mask.view(np.uint8)).reshape(-1, 64).sum(axis=1) + 1).astype(np.uint32)
        given[0] += 6
        want, members = prims.scan_reference(given), int(given.sum())
    got, total = prims.texel_set_rank(mask, given)
    diff = first_difference(got, want, [("block of 1024", 1024)])
    assert not diff, "rank of %d words (%s, %s): %s" % (nwords, kind, "counted" if counted else "to count", diff)
    assert total == members


# ---- radix sort -----------------------------------------------------------------------------------------------------------
# plan shapes (make_plan: equal digits of at most 8 bits; the result lies in (b) after an odd number of passes)
#   u32  [0,1) 1 x 1   [0,7) 1 x 7   [0,8) 1 x 8   [0,11) 6 + 5   [0,21) 3 x 7   [0,32) 4 x 8
#   u64  [32,53) 3 x 7   [56,59) 1 x 3   [32,56) 3 x 8   [0,64) 8 x 8   [5,6) 1 x 1
U32_RANGES = [(0, 1), (0, 7), (0, 8), (0, 11), (0, 21), (0, 32)]
U64_RANGES = [(32, 53), (56, 59), (32, 56), (0, 64), (5, 6)]
# n classes: below a round (1, 2, 63), a round (64), tail round (65), tail wave (1023 / 1025), a wave (1024), tail block
# (4095 / 4097 / 3 * 4096 + 1), a block (4096), and 2^20 + 3 (257 blocks: 65 792 scanned words, 65 block sums)
SORT_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 1, M + 3]
CONTENTS = ["uniform", "equal", "sorted", "reversed", "two_digits", "outside"]


def sort_table(ranges, sizes):
    """Every n meets every bit range (13 x 6 / 13 x 5 cells - each cell one sort, the largest 1 M elements); across a row
    the key contents rotate and the values alternate between the positions (iota) and given values, shifted row by row, so
    that every content and both value arms meet every plan shape and every n class several times."""
    table = []
    for i, n in enumerate(sizes):
        for j, (b, e) in enumerate(ranges):
            table.append((n, b, e, CONTENTS[(i + j) % len(CONTENTS)], (i + j) % 2 == 0))
    return table


def sort_keys(dtype, n, begin, end, content):
    """Keys whose digits (bits [begin, end)) follow `content`; the bits outside the range are random in every content (there
    are none when the range is the whole key)."""
    rng = np.random.default_rng(seed_of("sort", np.dtype(dtype).name, n, begin, end, content))
    noise = rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), n, dtype=dtype)
    inside = dtype(((1 << (end - begin)) - 1) << begin)
    digits = noise & inside
    if content == "uniform":
        pass
    elif content == "equal":             # one digit: stability alone decides the output
        digits = np.full(n, digits[0], dtype)
    elif content == "sorted":
        digits = np.sort(digits)
    elif content == "reversed":
        digits = np.sort(digits)[::-1]
    elif content == "two_digits":        # only the range's lowest and highest digit
        digits = np.where(rng.random(n) < 0.5, inside, dtype(0))
    elif content == "outside":           # up to three neighbouring digits in long runs of ties: only the outside bits tell the keys apart
        digits = rng.integers(0, min(1 << (end - begin), 3), n).astype(dtype) << dtype(begin)
    else:
        raise KeyError(content)
    return (digits | (noise & ~inside)).astype(dtype)


def check_sort(dtype, n, begin, end, content, iota):
    keys = sort_keys(dtype, n, begin, end, content)
    assert keys.dtype == dtype and keys.shape == (n,)
    vals = None if iota else np.random.default_rng(seed_of("vals", n, begin, end)).integers(0, 1 << 32, n, dtype=np.uint32)
    got_k, got_v, in_b = prims.radix_sort(keys, vals, begin, end)
    want_k, want_v = prims.sort_reference(keys, vals, begin, end)
    what = "%s sort of %d by bits [%d, %d), %s keys, %s" % (np.dtype(dtype).name, n, begin, end, content, "iota" if iota else "given values")
    units = [("block of 4096", 4096), ("wave of 1024", 1024), ("round of 64", 64)]
    diff = first_difference(got_k, want_k, units)
    assert not diff, "%s: keys: %s" % (what, diff)
    diff = first_difference(got_v, want_v, units)
    assert not diff, "%s: values: %s" % (what, diff)
    assert in_b == prims.sort_passes(begin, end) & 1, "%s: result reported in buffer %d after %d passes" % (what, in_b, prims.sort_passes(begin, end))
    # "the result is the same on every run": the same bytes again
    again_k, again_v, again_b = prims.radix_sort(keys, vals, begin, end)
    assert again_k.tobytes() == got_k.tobytes() and again_v.tobytes() == got_v.tobytes() and again_b == in_b, what


@pytest.mark.parametrize("n,begin,end,content,iota", sort_table(U32_RANGES, SORT_SIZES))
def test_radix_sort_u32_is_the_stable_sort(n, begin, end, content, iota):
    check_sort(np.uint32, n, begin, end, content, iota)


@pytest.mark.parametrize("n,begin,end,content,iota", sort_table(U64_RANGES, SORT_SIZES))
def test_radix_sort_u64_is_the_stable_sort(n, begin, end, content, iota):
    check_sort(np.uint64, n, begin, end, content, iota)


def test_the_table_crosses_every_content_with_every_plan_shape():
    for ranges in (U32_RANGES, U64_RANGES):
        table = sort_table(ranges, SORT_SIZES)
        assert {(n, b, e) for n, b, e, _, _ in table} == {(n, b, e) for n in SORT_SIZES for b, e in ranges}
        for b, e in ranges:
            cells = [(c, i) for n, bb, ee, c, i in table if (bb, ee) == (b, e)]
            assert {c for c, _ in cells} == set(CONTENTS) and {i for _, i in cells} == {True, False}
        for n in SORT_SIZES:
            assert {i for nn, _, _, _, i in table if nn == n} == {True, False}


def test_radix_sort_large_puts_the_inner_scan_in_its_second_regime():
    """u64, n = 4096 * 4096 + 1, bits [32, 56): three 8-bit passes over 4097 blocks - the scan inside every pass runs over
    256 * 4097 > 2^20 words, sort_scan_sums_kernel with per = 2."""
    n, begin, end = 4096 * 4096 + 1, 32, 56
    assert 256 * -(-n // 4096) > M and prims.sort_passes(begin, end) == 3
    rng = np.random.default_rng(20)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    got_k, got_v, in_b = prims.radix_sort(keys, None, begin, end)
    perm = np.argsort(prims.sort_digits(keys, begin, end).astype(np.uint32), kind="stable")
    units = [("block of 4096", 4096), ("wave of 1024", 1024), ("round of 64", 64)]
    diff = first_difference(got_v, perm.astype(np.uint32), units)
    assert not diff, "values: " + diff
    diff = first_difference(got_k, keys[perm], units)
    assert not diff, "keys: " + diff
    assert in_b == 1


@pytest.mark.parametrize("key_bytes,begin,end", [(4, 0, 21), (4, 0, 32), (8, 32, 56), (8, 0, 64)])
def test_radix_sort_of_nothing_leaves_the_buffers_alone(key_bytes, begin, end):
    assert prims.radix_sort_empty(key_bytes, 5000, begin, end) == 0       # (n = 0: "the result is in (a)")


# ---- block_scan -----------------------------------------------------------------------------------------------------------
def block_scan_values(kind, N, dtype, rounds=3):
    rng = np.random.default_rng(seed_of("block_scan", kind, N, np.dtype(dtype).name))
    v = np.zeros((rounds, N), dtype)
    if kind == "random":
        v[:] = rng.integers(0, 1 << 20, (rounds, N))
    elif kind == "zeros":
        pass
    elif kind == "lane0":
        v[:, 0] = [7, 11, 13]
    elif kind == "last":
        v[:, N - 1] = [7, 11, 13]
    elif kind == "mixed":                # the three rounds differ in kind: what a stale LDS word of the round before would show
        v[0] = rng.integers(0, 1 << 20, N)
        v[2, N - 1] = 5
    elif kind == "wide":                 # above 2^32: a truncation to 32 bits anywhere shows
        v[:] = rng.integers(1 << 33, 1 << 52, (rounds, N), dtype=np.uint64)
    elif kind == "wrap":                 # u32 sums wrap mod 2^32 like the type
        v[:] = rng.integers(1 << 30, 1 << 32, (rounds, N), dtype=np.uint64).astype(dtype)
    else:
        raise KeyError(kind)
    return v


BLOCK_SCAN_CASES = [(N, dtype, kind) for N in (256, 1024) for dtype in (np.uint32, np.uint64)
                    for kind in ["random", "zeros", "lane0", "last", "mixed"] + (["wide"] if dtype == np.uint64 else ["wrap"])]


@pytest.mark.parametrize("N,dtype,kind", BLOCK_SCAN_CASES, ids=["%d-%s-%s" % (N, np.dtype(d).name, k) for N, d, k in BLOCK_SCAN_CASES])
def test_block_scan_three_rounds_on_one_lds_array(N, dtype, kind):
    v = block_scan_values(kind, N, dtype)
    before, totals = prims.block_scan(N, v)
    want_before, want_total = prims.block_scan_reference(v)
    for r in range(v.shape[0]):          # rounds 1 and 2 are the test of the LDS-reuse promise
        diff = first_difference(before[r], want_before[r], [("wave", 64)])
        assert not diff, "block_scan<%d, %s> (%s) round %d: prefix: %s" % (N, np.dtype(dtype).name, kind, r, diff)
        diff = first_difference(totals[r], np.full(N, want_total[r], dtype), [("wave", 64)])
        assert not diff, "block_scan<%d, %s> (%s) round %d: total: %s" % (N, np.dtype(dtype).name, kind, r, diff)
