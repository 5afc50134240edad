"""The optical-flow case table (tests/optical_flow_cases.py) held to what it claims, on the CPU: which of the kernel's two tap
paths every workgroup of every case takes, the kernel constants that this rests on, and the oracle's pass against an
independent numpy restatement of the shader at every case - before tests/test_gpu_optical_flow_paths.py holds the kernel to
the oracle at the same cases.  What is asserted about a case's mix is a condition on the case, not a measurement of the
kernel."""
import os
import re

import numpy as np
import pytest

import optical_flow_cases as oc
from helpers import ROOT, bits_equal, golden, load, noise_frame, synth_frame

CASE_IDS = [c["name"] for c in oc.CASES]


def test_noise_frame_is_rough_and_reproducible():
    a = noise_frame(64, 48, 7)
    assert a.shape == (48, 64, 4) and a.dtype == np.uint8 and (a[..., 3] == 255).all()
    assert (a == noise_frame(64, 48, 7)).all() and (a != noise_frame(64, 48, 8)).mean() > 0.7
    counts = np.bincount(a[..., :3].ravel(), minlength=256)          # 9216 bytes: 36 a value on average
    assert counts.min() > 10 and counts.max() < 80
    # neighbours are unrelated: the mean absolute difference of independent uniform bytes is 85.3
    assert np.abs(np.diff(a[..., :3].astype(np.int64), axis=1)).mean() > 75
    assert np.abs(np.diff(synth_frame(64, 48, 7)[..., :3].astype(np.int64), axis=1)).mean() < 10


def test_table_holds_every_kind():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for name in ("mixed", "mixed_inset", "at_the_limit", "just_over", "small_direct", "clamped_direct", "downscale", "sub_tile_output", "upscale",
                 "clamped", "zoomed_in", "odd_everything", "frame_1x1", "width_limit", "negative_offset", "zero_offset",
                 "edge_offset_staged", "edge_offset_direct", "lambda_zero_same_frames", "alpha_clamps", "view_size_zero"):
        assert name in oc.BY_NAME, name
    for name in oc.NOISE_KINDS:
        assert oc.BY_NAME[name]["frameKind"] == "noise", name
    assert oc.BY_NAME["width_limit"]["frame"] == [65536, 1]          # th_tap_fx16's documented largest size
    assert {c["mix"] for c in oc.CASES} == {"staged", "direct", "mixed", "limit", "over"}
    for c in oc.CASES:                                               # every case is small: a GPU test of a few milliseconds
        assert c["out"][0] * c["out"][1] <= 256 * 128 and c["frame"][0] * c["frame"][1] <= 512 * 288


def test_kernel_constants_the_classification_rests_on():
    """the tile and the LDS budget of optical_flow_kernel: whoever retunes them has to move the cases"""
    with open(os.path.join(ROOT, "tendrils_amd", "csrc", "th_kernels.hip")) as f:
        text = f.read()
    tile = re.search(r"constexpr int kOfTileW = (\d+), kOfTileH = (\d+);", text)
    lds = re.search(r"constexpr int kOfLdsTexels = (\d+);", text)
    assert tile and lds
    assert (int(tile.group(1)), int(tile.group(2)), int(lds.group(1))) == (oc.TILE_W, oc.TILE_H, oc.LDS_TEXELS) == (32, 8, 3072)
    assert "const bool tiled = bw * bh <= kOfLdsTexels;" in text


@pytest.mark.parametrize("case", oc.CASES, ids=CASE_IDS)
def test_case_reaches_the_paths_it_claims(case):
    tiles = oc.classify(case)
    ow, oh = case["out"]
    assert len(tiles) == -(-ow // oc.TILE_W) * -(-oh // oc.TILE_H)
    staged = [t["texels"] for t in tiles if t["staged"]]
    direct = [t["texels"] for t in tiles if not t["staged"]]
    print("%s: %d workgroups, %d staged, %d direct, boxes %d..%d" % (case["name"], len(tiles), len(staged), len(direct),
                                                                    min(staged + direct), max(staged + direct)))
    fw, fh = case["frame"]
    for t in tiles:
        # the kernel's box rule: the taps of the first and last column / row bound those of every column / row between
        assert t["box"] == t["reach"], t
        assert 0 <= t["box"][0] <= t["box"][1] < fw and 0 <= t["box"][2] <= t["box"][3] < fh, t
    mix = case["mix"]
    if mix in ("staged", "limit"):
        assert not direct
    if mix == "direct":
        assert not staged
    if mix == "mixed":
        assert 4 * len(staged) >= len(tiles) and 4 * len(direct) >= len(tiles)
    if mix == "limit":
        assert max(staged) == oc.LDS_TEXELS
    if mix == "over":
        assert staged and direct and oc.LDS_TEXELS < min(direct) <= oc.LDS_TEXELS + 96
    if case["clamps"] == "none":
        assert not oc.clamped_edges(case, tiles, "any")
    elif case["clamps"]:
        assert oc.clamped_edges(case, tiles, case["clamps"]) == {"x0", "x1", "y0", "y1"}


def test_reference_captures_reach_both_paths():
    """the captures of the reference shader (tests/golden/of_*.npz), by the paths their workgroups take: what
    tests/test_gpu_optical_flow.py pins to the reference itself on each side"""
    want = dict(of_default_64="staged", of_demo_96x64="staged", of_demo_240x135="staged", of_texel_offset_240x135="staged",
                of_c3_1080p="direct", of_downscale_64x32="direct", of_small_direct_32x16="direct", of_clamped_96x64="limit",
                of_upscale_96x64="staged", of_mixed_256x128="mixed")
    found = {os.path.basename(p)[:-4]: p for p in golden("of")}
    assert set(found) == set(want)
    for name, path in found.items():
        meta = load(path)["meta"]
        tiles = oc.classify(meta)
        staged = [t["texels"] for t in tiles if t["staged"]]
        if want[name] in ("staged", "limit"):
            assert len(staged) == len(tiles), name
        if want[name] == "limit":
            assert max(staged) == oc.LDS_TEXELS
        if want[name] == "direct":
            assert not staged, name
        if want[name] == "mixed":
            assert 4 * len(staged) >= len(tiles) and 4 * (len(tiles) - len(staged)) >= len(tiles)
    assert {load(found[n])["meta"].get("frameKind", "smooth") for n in found} == {"smooth", "noise"}


def test_small_direct_clamps_on_its_direct_workgroups():
    """(the issue's 160 x 90 -> 40 x 24 case: its direct workgroups are the left column's, which clamp at three edges; the fourth
    is clamped_direct's business)"""
    case = oc.BY_NAME["small_direct"]
    assert oc.clamped_edges(case, oc.classify(case), "direct") >= {"x1", "y0", "y1"}


@pytest.fixture(scope="module")
def passes(oracle):
    """per case: inputs, the oracle's field and the restatement's, computed once"""
    out = {}
    for case in oc.CASES:
        f0, f1, dst = oc.inputs(case)
        details = {}
        want = oc.expected(case, f1, f0, dst, details)
        out[case["name"]] = dict(dst=dst, same_frames=(f0 == f1).all(), oracle=oc.oracle_pass(oracle, case, f1, f0, dst),
                                 want=want, **details)
    return out


@pytest.mark.parametrize("case", oc.CASES, ids=CASE_IDS)
def test_oracle_matches_the_restatement_bits(passes, case):
    p = passes[case["name"]]
    same = bits_equal(p["oracle"], p["want"])
    assert same.all(), oc.mismatch(case, p["oracle"], p["want"], same)
    # the pass did something - but for the two cases without a gradient (one texel; no offset): velocity 0, alpha 0
    assert bits_equal(p["oracle"], p["dst"]).all() == (case["name"] in ("zero_offset", "frame_1x1"))


def test_the_edge_cases_are_the_edges_they_claim(passes):
    p = passes["lambda_zero_same_frames"]
    assert p["same_frames"]
    nan = np.isnan(p["want"][..., 0])
    assert 0.25 < nan.mean() < 0.9                       # 0 / 0 where the taps of both pairs fall into one texel each ...
    assert (p["want"][nan][:, 3] == 1).all()             # ... where min(NaN, 1) = 1 (fminf), so the blend keeps none of dst
    p = passes["alpha_clamps"]
    assert (p["t"] > 1).mean() > 0.25 and (p["a"][p["t"] > 1] == 1).all() and (p["a"] < 1).any()
    p = passes["zero_offset"]                            # no gradient: velocity 0, alpha 0, the field stays
    assert (p["a"] == 0).all() and bits_equal(p["want"], p["dst"]).all()
    for name in ("mixed", "mixed_inset", "at_the_limit", "just_over", "downscale"):          # an alpha that keeps some of dst somewhere
        a = passes[name]["a"]
        assert ((a > 0) & (a < 1)).mean() > 0.25, name
    # offset 1.5: every off-centre tap is a corner row / column of the frame
    for name in ("edge_offset_staged", "edge_offset_direct"):
        t, (fw, fh) = oc.taps(oc.BY_NAME[name]), oc.BY_NAME[name]["frame"]
        assert (t["x"][0] == 0).all() and (t["x"][2] == fw - 1).all() and (t["y"][0] == 0).all() and (t["y"][2] == fh - 1).all()
    t = oc.taps(oc.BY_NAME["view_size_zero"])
    assert np.isinf(t["x_coord"][1]).all() and set(np.unique(t["x"][1])) == {0, 191}
    t = oc.taps(oc.BY_NAME["width_limit"])
    assert t["x"][2].max() == 65535 and t["x"][0].min() == 0


def test_accumulation_oracle_matches_the_restatement(oracle):
    case = oc.BY_NAME["mixed"]
    fw, fh = case["frame"]
    frames = [noise_frame(fw, fh, 40 + k) for k in range(3)]
    dst = oc.inputs(case)[2]
    want = oc.accumulate(case, frames, dst, oc.expected)
    got = oc.accumulate(case, frames, dst, lambda c, v, l, d: oc.oracle_pass(oracle, c, v, l, d))
    for k in range(3):
        assert bits_equal(got[k], want[k]).all(), k
    assert not bits_equal(want[0], want[1]).all() and not bits_equal(want[1], want[2]).all()
    wrong = oc.expected(case, frames[2], frames[0], want[1])         # (`last` not rotated: the field would differ)
    assert not bits_equal(wrong, want[2]).all()


def test_padded_case_keeps_every_tap():
    """the condition the GPU test's padded run rests on: inside the doubled frame every tap is the texel it was, moved by the
    border, and the workgroups split as before"""
    case = oc.BY_NAME["mixed_inset"]
    big, _ = oc.padded(case)
    fw, fh = case["frame"]
    a, b = oc.taps(case), oc.taps(big)
    for axis, border in (("x", fw // 2), ("y", fh // 2)):
        for k in range(3):
            assert (b[axis][k] == a[axis][k] + border).all()
    assert [t["staged"] for t in oc.classify(big)] == [t["staged"] for t in oc.classify(case)]
    assert all(t["box"][0] >= fw // 2 and t["box"][2] >= fh // 2 for t in oc.classify(big))
