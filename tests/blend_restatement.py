"""Restatement of the reference's colour-map blend (src/screen/blend/main.frag + src/blend/sum.glsl, drawn by
src/screen/blend/index.js under the GL state Tendrils.step() leaves) in numpy float32: one rounded operation per GLSL
operation, in the shader's order.  Pinned against captures of the reference's own Blend (tests/golden/blend_*.npz, written by
tools/capture_blend.py); the HIP pass (tendrils_amd/csrc/th_blend.hip) is the same sequence of single fp32 operations.

A view is (format, texels, alpha):
  "rgba32f"  [h, w, 4] f32   a float FBO (the image spawner's buffer)
  "rgba8"    [h, w, 4] u8    a non-float FBO (the optical-flow frames): UNORM8 -> (c * 257) * (1 / 65535), as the optical-flow
                             pass reads its frames
  "l32f"     [n] f32         an AudioTexture: n x 1 texels of one channel, sampled as (L, L, L, 1)
Every view is NEAREST / CLAMP_TO_EDGE, sampled at uv = gl_FragCoord.xy / resolution of the TARGET: a float texture at
texel = clamp(floor(uv * size), 0, size - 1) in fp32, an 8-bit one through the 16-bit fixed-point coordinate the captured GL
uses for such textures (nearest_fx16) - the two differ where uv * size lands on a texel boundary, and the captures have
such texels (blend_eight_views_13x11: a 26 x 22 frame under a 13 x 11 target, every tap on a boundary).
"""
import numpy as np

F = np.float32
FORMATS = {"rgba32f": 0, "rgba8": 1, "l32f": 2}          # TH_TEX_*


def nearest(u, n):
    """NEAREST + CLAMP_TO_EDGE: clamp(floor(u * n), 0, n - 1), fp32 (th_raster.hpp: dep_nearest)"""
    f = np.floor((u * F(n)).astype(F))
    return np.clip(f, 0, n - 1).astype(np.int64)


def nearest_fx16(u, n):
    """NEAREST + CLAMP_TO_EDGE on an 8-bit-per-channel texture, with the coordinate precision of the captured GL: clamp to
    [0, 1), truncate to 16 fractional bits, texel = (coord16 * n) >> 16 (th_kernels.hip: nearest_texel_fx16, as the optical-flow
    pass reads its frames)"""
    c = np.clip(u, F(0.0), F(65535.0 / 65536.0)).astype(F)
    fx = (c * F(65536.0)).astype(F).astype(np.int64)
    return (fx * n) >> 16


def decode(fmt, texels):
    """a view's texels as [h, w, 4] f32, the way texture2D returns them"""
    if fmt == "rgba32f":
        return np.ascontiguousarray(texels, F)
    if fmt == "rgba8":
        t = np.ascontiguousarray(texels, np.uint8).astype(F)
        return ((t * F(257.0)).astype(F) * (F(1.0) / F(65535.0))).astype(F)
    if fmt == "l32f":
        lum = np.ascontiguousarray(texels, F).reshape(1, -1)
        out = np.ones(lum.shape + (4,), F)
        out[..., 0] = out[..., 1] = out[..., 2] = lum
        return out
    raise ValueError(fmt)


def shader(views, w, h):
    """gl_FragColor of main.frag for every texel of a w x h target: [h, w, 4] f32"""
    uvx = ((np.arange(w, dtype=F) + F(0.5)) / F(w)).astype(F)
    uvy = ((np.arange(h, dtype=F) + F(0.5)) / F(h)).astype(F)
    total = np.zeros((h, w, 4), F)
    with np.errstate(all="ignore"):
        for fmt, texels, alpha in views:
            t = decode(fmt, texels)
            tap = nearest_fx16 if fmt == "rgba8" else nearest
            c = t[tap(uvy, t.shape[0])[:, None], tap(uvx, t.shape[1])[None, :]]
            a = (c[..., 3] * F(alpha)).astype(F)                           # color.a * alpha
            total[..., :3] = (total[..., :3] + (c[..., :3] * a[..., None]).astype(F)).astype(F)   # sum + vec4(color.rgb * a, a)
            total[..., 3] = (total[..., 3] + a).astype(F)
    return total


def blend_stage(src, gl_blend=True, clear=True, dst=None):
    """what the target holds after the GL has written the shader's output `src` over `dst` (zeros after the clear)"""
    if not gl_blend:
        return src
    dst = np.zeros_like(src) if (clear or dst is None) else np.ascontiguousarray(dst, F)
    with np.errstate(all="ignore"):
        sa = src[..., 3:4]
        ia = (F(1.0) - sa).astype(F)
        return ((src * sa).astype(F) + (dst * ia).astype(F)).astype(F)     # SRC_ALPHA, ONE_MINUS_SRC_ALPHA on a float target


def blend(views, w, h, gl_blend=True, clear=True, dst=None):
    """The target after Blend.draw(target, [w, h], clear): `dst` is the target before (zeros when None)."""
    return blend_stage(shader(views, w, h), gl_blend, clear, dst)


def fixture_views(fx):
    """(format, texels, alpha) of a blend_*.npz fixture's views"""
    names = {"audio": "l32f", "rgba8": "rgba8", "rgba32f": "rgba32f"}
    return [(names[fx["meta"]["formats"][int(k)]], fx["tex%d" % int(k)], float(a)) for k, a in zip(fx["views"], fx["alphas"])]


def fixture_blend(fx):
    w, h = fx["meta"]["target"]
    return blend(fixture_views(fx), w, h, fx["meta"]["glBlend"], fx["meta"]["clear"], fx.get("prefill"))
