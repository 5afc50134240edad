"""optical_flow_kernel's two tap paths - the frame box staged in LDS, or every tap a global load, chosen per workgroup at run
time - at the shapes where they part (tests/optical_flow_cases.py; tests/test_optical_flow_cases.py holds every case to the
paths it claims and the oracle to an independent restatement, on the CPU).  Every case goes through the OpticalFlow mirror
and the whole field is compared with the oracle bit for bit, NaN equal to NaN; a mismatch names the workgroup of the first
differing texel and the path it took.  Then the kernel's own promise - both paths give the same bits - head on: the same
taps with the offset's sign flipped, and the same frame inside a larger one, where every box starts elsewhere.  Last, what
th_optical_flow and th_frames_resize refuse."""
import ctypes as C

import numpy as np
import pytest

import optical_flow_cases as oc
from helpers import bits_equal, noise_frame
from test_gpu_optical_flow import run_of
from test_gpu_pass_errors import refused

pytestmark = pytest.mark.gpu

F = np.float32
CASE_IDS = [c["name"] for c in oc.CASES]


def held_to_oracle(oracle, case, got, view, last, dst):
    want = oc.oracle_pass(oracle, case, view, last, dst)
    same = bits_equal(got, want)
    assert same.all(), oc.mismatch(case, got, want, same)
    return want


@pytest.mark.parametrize("case", oc.CASES, ids=CASE_IDS)
def test_case_matches_oracle_bits(oracle, case):
    f0, f1, dst = oc.inputs(case)
    held_to_oracle(oracle, case, run_of(case, f0, f1, dst), f1, f0, dst)


def test_flipped_offset_exchanges_the_taps(oracle):
    """offset -> -offset: the minus and plus taps trade places, every workgroup's box stays.  Each run is the oracle's, and the
    two differ (the gradient changes sign) - a kernel that took |offset| somewhere would give one field twice."""
    case = oc.BY_NAME["mixed"]
    flipped = dict(case, uniforms=dict(case["uniforms"], offset=-case["uniforms"]["offset"]))
    assert [t["box"] for t in oc.classify(flipped)] == [t["box"] for t in oc.classify(case)]
    f0, f1, dst = oc.inputs(case)
    a = held_to_oracle(oracle, case, run_of(case, f0, f1, dst), f1, f0, dst)
    b = held_to_oracle(oracle, flipped, run_of(flipped, f0, f1, dst), f1, f0, dst)
    assert not bits_equal(a, b).all()


def test_padded_frame_moves_every_box_and_no_result(oracle):
    """The inset mixed case (staged and direct workgroups, no tap clamped) inside a frame of twice its size, a border of noise
    all round, scaleUV and offset halved: every tap is the texel it was, so the field is the one it was, bit for bit - through
    box origins, LDS indices and a frame pitch that all differ.  (The workgroups split between the paths as before: the boxes
    keep their sizes.)"""
    case = oc.BY_NAME["mixed_inset"]
    big, embed = oc.padded(case)
    (fw, fh), a, b = case["frame"], oc.taps(case), oc.taps(big)
    for axis, border, n in (("x", fw // 2, fw), ("y", fh // 2, fh)):
        for k in range(3):
            assert (b[axis][k] == a[axis][k] + border).all()                     # the same texels, moved by the border ...
            assert border <= b[axis][k].min() and b[axis][k].max() < border + n     # ... so no tap reaches the border
    tiles = oc.classify(big)
    assert [t["staged"] for t in tiles] == [t["staged"] for t in oc.classify(case)]
    assert 4 * sum(t["staged"] for t in tiles) >= len(tiles) and 4 * sum(not t["staged"] for t in tiles) >= len(tiles)
    f0, f1, dst = oc.inputs(case)
    plain = held_to_oracle(oracle, case, run_of(case, f0, f1, dst), f1, f0, dst)
    big0, big1 = embed(f0, 0), embed(f1, 1)
    assert (big0[:fh // 2] != big1[:fh // 2]).any()                                 # (a border that a tap would notice)
    got = run_of(big, big0, big1, dst)
    same = bits_equal(got, plain)
    assert same.all(), oc.mismatch(big, got, plain, same)


def test_accumulation_and_frame_rotation(oracle):
    """One destination field through three passes on three frames: two render() calls without a step() between them (the
    second starts from the first one's output), then step(), a new frame, render().  Field after every pass = the oracle's."""
    import tendrils_amd as ta
    from tendrils_amd.optical_flow import OpticalFlow
    from tendrils_amd.tendrils import View
    case = oc.BY_NAME["mixed"]
    (fw, fh), (ow, oh) = case["frame"], case["out"]
    frames = [noise_frame(fw, fh, 40 + k) for k in range(3)]
    dst = oc.inputs(case)[2]
    want = oc.accumulate(case, frames, dst, lambda c, v, l, d: oc.oracle_pass(oracle, c, v, l, d))
    t = ta.Tendrils(View(ow, oh))
    t.resize()
    t.setup(8)
    t.flow.set_pixels(dst)
    of = OpticalFlow(t)
    of.resize(case["frame"])
    of.set_pixels(frames[0])
    of.step()
    of.set_pixels(frames[1])
    of.update(case["uniforms"])
    got = []
    of.render()
    got.append(t.flow.read())
    of.render()
    got.append(t.flow.read())
    of.step()
    of.set_pixels(frames[2])
    of.render()
    got.append(t.flow.read())
    t.dispose()
    for k in range(3):
        same = bits_equal(got[k], want[k])
        assert same.all(), "pass %d: %s" % (k, oc.mismatch(case, got[k], want[k], same))


# ---- what the entry points refuse ------------------------------------------------------------------------------------------------
def test_optical_flow_and_frames_resize_refusals(oracle):
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.particles import Particles
    invalid = _capi.TH_ERR_INVALID
    rng = np.random.default_rng(11)
    p = Particles(None, dict(shape=[8, 8]))
    p.setup(2)
    ctx = p._ctx
    call("th_flow_resize", ctx, 40, 24)
    flow = rng.uniform(-1, 1, (24, 40, 4)).astype(F)
    call("th_flow_upload", ctx, flow.ctypes.data_as(_capi._fp))

    def field():
        out = np.empty((24, 40, 4), F)
        call("th_flow_download", ctx, out.ctypes.data_as(_capi._fp))
        return out

    case = oc.BY_NAME["small_direct"]
    un = case["uniforms"]
    u = _capi.OpticalFlowUniforms()
    u.viewSize[0], u.viewSize[1], u.scaleUV[0], u.scaleUV[1] = un["viewSize"] + un["scaleUV"]
    u.offset, u.lambda_, u.time, u.speed, u.speedLimit = un["offset"], un["lambda"], un["time"], un["speed"], un["speedLimit"]
    # no frames yet: refused, nothing launched
    refused("th_optical_flow", (ctx, C.byref(u)), invalid, "no frame buffers (call th_frames_resize)")
    assert bits_equal(field(), flow).all()
    refused("th_optical_flow", (ctx, None), invalid, "null uniforms")
    # shapes that th_frames_resize refuses - and after each the context still has no frames
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -3), (0, 0), (1 << 14, 1 << 14)):
        refused("th_frames_resize", (ctx, w, h), invalid, "bad frame shape %dx%d" % (w, h))
    # th_tap_fx16 samples at most 65536 texels a side (a 16-bit coordinate times the size, in 32 bits)
    for w, h in ((65537, 1), (1, 65537), (1 << 20, 2)):
        refused("th_frames_resize", (ctx, w, h), invalid,
                "bad frame shape %dx%d (frames are RGBA8 images: at most 65536 a side)" % (w, h))
    refused("th_optical_flow", (ctx, C.byref(u)), invalid, "no frame buffers (call th_frames_resize)")
    assert bits_equal(field(), flow).all()
    # a refused resize leaves the frames that are there: 160 x 90 frames, then the valid pass is the oracle's
    f0, f1, _ = oc.inputs(case)
    call("th_frames_resize", ctx, 160, 90)
    call("th_frames_upload", ctx, f0.ctypes.data_as(C.POINTER(C.c_uint8)))
    call("th_frames_rotate", ctx)
    call("th_frames_upload", ctx, f1.ctypes.data_as(C.POINTER(C.c_uint8)))
    refused("th_frames_resize", (ctx, 65537, 90), invalid, "bad frame shape 65537x90 (frames are RGBA8 images: at most 65536 a side)")
    refused("th_frames_resize", (ctx, 160, 0), invalid, "bad frame shape 160x0")
    call("th_optical_flow", ctx, C.byref(u))
    got, want = field(), oc.oracle_pass(oracle, case, f1, f0, flow)
    same = bits_equal(got, want)
    assert same.all(), oc.mismatch(case, got, want, same)
    p.dispose()
