"""The colour-map blend's restatement (tests/blend_restatement.py) against the captures of the reference's own Blend /
AudioTexture / gl-fbo objects (tests/golden/blend_*.npz, tools/capture_blend.py): bit for bit, in every texel of every
capture - the blend stage of the captured GL (SRC_ALPHA / ONE_MINUS_SRC_ALPHA on a float target) included, so no case needs
a tolerance (largest deviation measured between capture and restatement: 0, profiles/colormap_blend.txt).  The host classes'
audio maps are checked against what the reference's AudioTexture made of the same analyser bytes."""
import numpy as np
import pytest

import blend_restatement as R
from helpers import bits_equal, golden, load

FIXTURES = golden("blend")
NAMES = ["blend_demo_24x16", "blend_eight_views_13x11", "blend_first_frame_24x16", "blend_noclear_17x9", "blend_npot_17x9",
         "blend_unit_target_1x1"]


def test_every_capture_is_there():
    assert [p.split("/")[-1][:-4] for p in FIXTURES] == NAMES


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_restatement_equals_capture_bit_for_bit(path):
    fx = load(path)
    assert fx["meta"]["floatBlend"] is True           # the captured GL blended on the float target itself (EXT_float_blend)
    w, h = fx["meta"]["target"]
    got = R.fixture_blend(fx)
    assert got.shape == fx["out"].shape == (h, w, 4)
    same = bits_equal(got, fx["out"])
    assert same.all(), "%d of %d components differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])


def test_captures_cover_what_they_are_for():
    fx = {n: load(p) for n, p in zip(NAMES, FIXTURES)}
    demo, first = fx["blend_demo_24x16"], fx["blend_first_frame_24x16"]
    assert demo["meta"]["glBlend"] and not first["meta"]["glBlend"]
    for k in ("tex0", "tex1", "tex2", "alphas", "views"):
        assert (demo[k] == first[k]).all()
    assert demo["meta"]["shapes"] == [[8, 1], [16, 1], [12, 10]]          # an AudioTexture of n bins is n x 1: the bins run along x
    assert not bits_equal(demo["out"], first["out"]).all()                  # the blend state shows
    assert (first["out"][..., 3] != 1.0).any() and (first["out"][:, 0] != first["out"][:, 23]).any()
    npot = fx["blend_npot_17x9"]
    assert npot["tex0"].max() > 1 and npot["tex0"].min() < 0 and npot["alphas"].max() > 1 and npot["alphas"].min() < 0
    assert npot["out"].max() > 1                                            # nothing is clamped in the blend
    assert not fx["blend_noclear_17x9"]["meta"]["clear"] and "prefill" in fx["blend_noclear_17x9"]
    eight = fx["blend_eight_views_13x11"]
    assert len(eight["views"]) == 8 and len(set(eight["views"].tolist())) < 8    # a texture named twice
    assert set(eight["meta"]["formats"]) == {"audio", "rgba8", "rgba32f"}
    assert fx["blend_unit_target_1x1"]["meta"]["target"] == [1, 1]


def test_rgba8_taps_differ_from_float_taps_where_the_captures_say_so():
    """blend_eight_views_13x11 has a 26 x 22 frame under a 13 x 11 target: every tap lands on a texel boundary, where the
    captured GL's fixed-point coordinate (8-bit textures) picks the texel below the one the float rule picks."""
    u = ((np.arange(13, dtype=np.float32) + np.float32(0.5)) / np.float32(13)).astype(np.float32)
    assert (R.nearest_fx16(u, 26) != R.nearest(u, 26)).any()
    assert (R.nearest_fx16(u, 26) <= R.nearest(u, 26)).all() and R.nearest_fx16(u, 26).min() == 0


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_host_audio_maps_equal_the_reference(path):
    from tendrils_amd.blend import AudioTexture
    fx = load(path)
    for k, (fmt, how) in enumerate(zip(fx["meta"]["formats"], fx["meta"]["maps"])):
        if fmt != "audio":
            continue
        raw, want = fx["raw%d" % k], fx["tex%d" % k]
        t = AudioTexture(None, len(raw))
        assert t.shape == [len(raw), 1] and not t.array.any()
        getattr(t, how)(raw)
        assert bits_equal(t.array, want).all()
        assert not t._texels.any()                    # the texture changes with apply(), not with the map
        t.apply()
        assert bits_equal(t._texels, want).all()


def test_audio_texture_from_an_array_and_maps_in_place():
    from tendrils_amd.blend import AudioTexture
    t = AudioTexture(None, np.array([0, 64, 128, 255], np.float32))
    assert t.array.tolist() == [0, 64, 128, 255] and t._texels.tolist() == [0, 64, 128, 255]
    t.waveform()                                       # data = this.array.data: in place
    assert t.array.tolist() == [-1.0, -0.5, 0.0, 127 / 128]
    t.assign([3, 2]).apply()                           # mapList over a shorter source leaves the rest
    assert t._texels.tolist() == [3.0, 2.0, 0.0, 127 / 128]
    assert AudioTexture(None, 4).frequencies(np.array([0, 1, 128, 255], np.uint8)).array.tolist() == [0, 1 / 256, 0.5, 255 / 256]
