"""The optical-flow cases that tests/test_optical_flow_cases.py (CPU) and tests/test_gpu_optical_flow_paths.py (GPU) share, and
a restatement of the pass in numpy float32 that both read them with.

optical_flow_kernel (tendrils_amd/csrc/th_kernels.hip) takes one of two paths per 32 x 8 workgroup tile, chosen at run time:
the box of frame texels that the tile's ten taps can reach is staged in LDS as gray values when it holds at most 3072 texels
("staged"), else every tap is a global load ("direct").  The cases are shapes and uniforms at which the two paths part: both
in one launch, a box of exactly 3072 texels and one just over, frames larger than the field, an output smaller than a tile,
clamped taps, frames with no smoothness.  `mix` is what a case is MEANT to reach; the CPU test holds every case to it with
`classify`, so that the GPU test knows which path it ran.

The restatement is written out from the shader (src/optical-flow/index.frag:55-81, src/utils/gray-scale.glsl, bezier.glsl,
src/flow/apply/state.glsl) and the tap rule of the captured reference run, one rounded fp32 operation per GLSL operation, in
the shader's order - not from the oracle (oracle/tendrils_oracle.c), which the CPU test holds to it bit for bit.
"""
import numpy as np

from helpers import of_inputs

F = np.float32
TILE_W, TILE_H, LDS_TEXELS = 32, 8, 3072           # kOfTileW, kOfTileH, kOfLdsTexels (pinned by the CPU test)


def _case(name, mix, frame, out, scaleUV, viewSize, offset, kind="smooth", clamps=None, shift8=(12, 6), **uniforms):
    """mix: "staged" / "direct" (every workgroup), "mixed" (at least a quarter of them on each side), "limit" (all staged, the
    largest box exactly LDS_TEXELS), "over" (the smallest direct box at most LDS_TEXELS + 96).  clamps: None, or the path
    whose workgroups must hold taps clamped at all four frame edges ("none": no tap of the case may be clamped)."""
    un = dict(viewSize=list(viewSize), scaleUV=list(scaleUV), offset=offset, speed=1.0, speedLimit=1.0, time=1234.5)
    un["lambda"] = 0.001
    un.update(uniforms)
    return dict(name=name, mix=mix, clamps=clamps, frame=list(frame), out=list(out), uniforms=un, frameKind=kind,
                seed=sum(map(ord, name)), shift8=list(shift8))


DEMO = dict(speed=0.08, speedLimit=0.01)            # src/demo.main.js:526-530 with the tendrils' speedLimit

CASES = [
    # ---- where the two paths part ----
    _case("mixed", "mixed", (256, 128), (256, 128), [1, -1], [1, 1], 0.12, "noise"),
    # ... and with every tap inside the frame (the mixed case clamps at all four edges): the case that `padded` can embed
    _case("mixed_inset", "mixed", (256, 256), (200, 100), [0.75, -0.75], [1, 1], 0.066, "noise", clamps="none"),
    _case("at_the_limit", "limit", (256, 96), (256, 96), [1, -1], [1, 1], 0.125, "noise"),
    _case("just_over", "over", (256, 96), (256, 96), [1, -1], [1, 1], 0.13, "noise"),
    _case("small_direct", "mixed", (160, 90), (40, 24), [-1, -1], [1, 1], 0.1, "noise", clamps="any"),
    _case("clamped_direct", "direct", (160, 90), (32, 24), [-1, -1], [1, 1], 0.1, "noise", clamps="direct"),
    _case("downscale", "direct", (512, 288), (64, 36), [-1, -1], [1, 64 / 36], 1.0 / 512, "noise"),
    _case("sub_tile_output", "staged", (37, 23), (5, 3), [1, 1], [1, 1], 0.05, **DEMO),
    _case("upscale", "staged", (16, 9), (96, 64), [-1, -1], [1, 1.5], 0.1, **DEMO),
    _case("clamped", "limit", (96, 64), (96, 64), [-2.5, 2.5], [1, 1], 0.1, "noise", clamps="staged"),
    _case("zoomed_in", "staged", (256, 128), (64, 32), [0.25, -0.25], [1, 1], 0.02, **DEMO),
    _case("odd_everything", "staged", (131, 67), (100, 45), [-1, -1], [1, 100 / 45], 0.07, **DEMO),
    # ---- edges of the tap rule and of the arithmetic after it ----
    _case("frame_1x1", "staged", (1, 1), (33, 9), [1, -1], [1, 1], 0.1, "noise"),
    _case("width_limit", "direct", (65536, 1), (64, 8), [1, -1], [1, 1], 0.01, "noise"),       # th_tap_fx16's largest size
    _case("negative_offset", "mixed", (256, 128), (256, 128), [1, -1], [1, 1], -0.12, "noise"),
    _case("zero_offset", "staged", (96, 64), (96, 64), [-1, -1], [1, 1.5], 0.0, "noise"),
    _case("edge_offset_staged", "staged", (48, 32), (96, 64), [1, -1], [1, 1], 1.5, "noise", clamps="staged"),
    _case("edge_offset_direct", "direct", (96, 64), (96, 64), [1, -1], [1, 1], 1.5, "noise", clamps="direct"),
    # 0 / 0: lambda = 0 gives gradMag = 0 wherever both pairs of taps fall into one texel (a small frame under a large field), and NaN
    # from there on; identical frames (shift8 = 0) keep the other texels finite
    _case("lambda_zero_same_frames", "staged", (16, 9), (96, 64), [1, -1], [1, 1], 1.0 / 128, "noise", shift8=(0, 0),
          **{"lambda": 0.0}),
    # length(vel) / speedLimit > 1: the bezier parameter leaves [0, 1] and the alpha clamps to 1
    _case("alpha_clamps", "staged", (96, 64), (96, 64), [-1, -1], [1, 1.5], 0.02, "noise", speed=0.08, speedLimit=0.01),
    # uv * scaleUV / 0 = +-inf on every column (no pixel centre of an even width is 0): every x tap clamps to an edge.  The
    # workgroups of the middle columns reach both edges (direct), the others one column of the frame (staged)
    _case("view_size_zero", "mixed", (192, 128), (96, 64), [1, -1], [0, 1], 0.1, "noise", clamps="any"),
]
BY_NAME = {c["name"]: c for c in CASES}
NOISE_KINDS = ("mixed", "at_the_limit", "just_over", "small_direct", "downscale", "clamped")       # must use the noise frames


def inputs(case):
    """(last frame, view frame, destination flow) of a case, as tests/helpers.py:of_inputs makes them for a fixture"""
    return of_inputs(case)


# ---- the tap rule ------------------------------------------------------------------------------------------------------------
def frame_uv(c, size, scale, view):
    """frame coordinate along one axis of the output texels `c` (an integer array) of `size`: the varying uv is the NDC of the
    pixel centre, (c + 0.5) * fl(2 / size) - 1 as the rasteriser of the captured run interpolates it; then
    posToUV(uv * scaleUV / viewSize) = (1 * (p + 1)) / 2 (index.frag:56)"""
    with np.errstate(all="ignore"):
        uv = (np.asarray(c).astype(F) + F(0.5)) * (F(2.0) / F(size)) - F(1.0)
        p = uv * F(scale) / F(view)
        return (F(1.0) * (p + F(1.0))) / F(2.0)


def tap_fx16(u, n):
    """NEAREST + CLAMP_TO_EDGE on an 8-bit-per-channel texture of n texels, as the captured run did it: the coordinate clamped
    to [0, 1) (a NaN: 0), truncated to 16 fractional bits, texel = (coord16 * n) >> 16"""
    u = np.asarray(u, F)
    with np.errstate(invalid="ignore"):
        c = np.where(u > 0, u, F(0.0))
        c = np.where(c > F(65535.0 / 65536.0), F(65535.0 / 65536.0), c).astype(F)
    return ((c * F(65536.0)).astype(F).astype(np.int64) * int(n)) >> 16


def taps(case):
    """per axis, the three tap texel indices of every output column / row: dict(x=(minus, centre, plus), y=...), and the
    coordinates before the clamp, for the tests that ask whether a tap clamped"""
    (fw, fh), (ow, oh), un = case["frame"], case["out"], case["uniforms"]
    o = F(un["offset"])
    out = {}
    for axis, (n, size) in enumerate(((fw, ow), (fh, oh))):
        s = frame_uv(np.arange(size), size, un["scaleUV"][axis], un["viewSize"][axis])
        coords = ((s - o).astype(F), s, (s + o).astype(F))
        out["xy"[axis]] = tuple(tap_fx16(c, n) for c in coords)
        out["xy"[axis] + "_coord"] = coords
    return out


# ---- which path a workgroup takes -----------------------------------------------------------------------------------------------
def classify(case):
    """Every workgroup tile of the launch, row-major: a list of dict(x0, x1, y0, y1 = its output texels, half-open;
    box = (bx0, bx1, by0, by1) inclusive frame texels by the kernel's rule - the three taps of the tile's first and last
    column / row; reach = the same from every column and row of the tile; texels = the box's size; staged)."""
    ow, oh = case["out"]
    t = taps(case)
    tiles = []
    for y0 in range(0, oh, TILE_H):
        for x0 in range(0, ow, TILE_W):
            x1, y1 = min(x0 + TILE_W, ow), min(y0 + TILE_H, oh)
            ex = [int(k[c]) for k in t["x"] for c in (x0, x1 - 1)]
            ey = [int(k[r]) for k in t["y"] for r in (y0, y1 - 1)]
            box = (min(ex), max(ex), min(ey), max(ey))
            ax = np.concatenate([k[x0:x1] for k in t["x"]])
            ay = np.concatenate([k[y0:y1] for k in t["y"]])
            reach = (int(ax.min()), int(ax.max()), int(ay.min()), int(ay.max()))
            texels = (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
            tiles.append(dict(x0=x0, x1=x1, y0=y0, y1=y1, box=box, reach=reach, texels=texels, staged=texels <= LDS_TEXELS))
    return tiles


def clamped_edges(case, tiles, path):
    """the frame edges ("x0", "x1", "y0", "y1") at which some tap of a workgroup on `path` ("staged", "direct", "any") was
    clamped: its coordinate lay outside [0, 1) before the clamp"""
    t = taps(case)
    edges = set()
    for tile in tiles:
        if path != "any" and tile["staged"] != (path == "staged"):
            continue
        for axis, (a, b) in (("x", (tile["x0"], tile["x1"])), ("y", (tile["y0"], tile["y1"]))):
            c = np.concatenate([k[a:b] for k in t[axis + "_coord"]])
            with np.errstate(invalid="ignore"):
                if (c < 0).any():
                    edges.add(axis + "0")
                if (c >= 1).any():
                    edges.add(axis + "1")
    return edges


def tile_of(case, tiles, y, x):
    """the workgroup tile that owns output texel (y, x), and its path's name"""
    tiles_x = (case["out"][0] + TILE_W - 1) // TILE_W
    tile = tiles[(y // TILE_H) * tiles_x + x // TILE_W]
    return tile, "staged" if tile["staged"] else "direct"


def mismatch(case, got, want, same):
    """the message of a failed comparison: how many components differ, the first differing texel, its workgroup and path"""
    bad = np.argwhere(~same.all(-1))
    y, x = (int(v) for v in bad[0])
    tile, path = tile_of(case, classify(case), y, x)
    return ("%s: %d components of %d texels differ; first texel (x %d, y %d) got %s want %s, in the %s workgroup of output "
            "x %d..%d, y %d..%d (box %s, %d frame texels)" % (
                case["name"], (~same).sum(), len(bad), x, y, got[y, x], want[y, x], path.upper(), tile["x0"], tile["x1"] - 1,
                tile["y0"], tile["y1"] - 1, tile["box"], tile["texels"]))


# ---- the whole pass --------------------------------------------------------------------------------------------------------------
def gray(img):
    """texture2D on an RGBA8 texture - UNORM8 -> float as (c * 257) * (1 / 65535), what the captured run did - then
    grayScale(): dot(rgb, (0.3, 0.59, 0.11))"""
    t = ((np.ascontiguousarray(img, np.uint8)[..., :3].astype(F) * F(257.0)).astype(F) * (F(1.0) / F(65535.0))).astype(F)
    return (t[..., 0] * F(0.3) + t[..., 1] * F(0.59)) + t[..., 2] * F(0.11)


def shader(case, view, last, details=None):
    """gl_FragColor of index.frag for every texel of the case's output: [oh, ow, 4] f32 (details: a dict that receives the
    bezier parameter `t` and the alpha `a`)"""
    un = case["uniforms"]
    t = taps(case)
    (xm, xc, xp), (ym, yc, yp) = t["x"], t["y"]
    X = lambda k: k[None, :]
    Y = lambda k: k[:, None]
    gv, gl = gray(view), gray(last)
    with np.errstate(all="ignore"):
        gx = (gv[Y(yc), X(xp)] - gv[Y(yc), X(xm)]) + (gl[Y(yc), X(xp)] - gl[Y(yc), X(xm)])            # :63-64
        gy = (gv[Y(yp), X(xc)] - gv[Y(ym), X(xc)]) + (gl[Y(yp), X(xc)] - gl[Y(ym), X(xc)])            # :66-67
        mag = np.sqrt(((gx * gx) + (gy * gy)) + F(un["lambda"]))                                    # :69
        diff = gv[Y(yc), X(xc)] - gl[Y(yc), X(xc)]                                                    # :72
        vx, vy = (diff * (gx / mag)) * F(un["speed"]), (diff * (gy / mag)) * F(un["speed"])           # :78
        limit = F(un["speedLimit"])
        tt = np.sqrt(vx * vx + vy * vy) / limit
        ut = F(1.0) - tt
        bz = (F(0.0) * ut + F(0.0) * tt) * ut + (F(0.0) * ut + F(1.0) * tt) * tt                    # bezier(vec3(0, 0, 1), t)
        fx, fy = bz * vx, bz * vy
        a = np.fmin(np.sqrt(fx * fx + fy * fy) / limit, F(1.0))                                     # flow(): min(|v| / limit, 1)
    if details is not None:
        details.update(t=tt, a=a)
    out = np.empty(gx.shape + (4,), F)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = fx, fy, F(un["time"]), a
    return out


def blend(src, dst):
    """gl.blendFunc(SRC_ALPHA, ONE_MINUS_SRC_ALPHA) on the float target"""
    with np.errstate(all="ignore"):
        a = src[..., 3:4]
        return (src * a + np.asarray(dst, F) * (F(1.0) - a)).astype(F)


def expected(case, view, last, dst, details=None):
    """the flow field after one blended pass of the case over `dst`"""
    return blend(shader(case, view, last, details), dst)


def oracle_pass(oracle, case, view, last, dst):
    """the same pass by the oracle (oracle/tendrils_oracle.c: to_optical_flow)"""
    un = case["uniforms"]
    u = oracle.optical_flow_uniforms(un["time"], view_size=un["viewSize"], scaleUV=un["scaleUV"], offset=un["offset"],
                                     lambda_=un["lambda"], speed=un["speed"], speedLimit=un["speedLimit"])
    return oracle.optical_flow(u, view, last, dst, blend=True)


# ---- the sequences of passes ------------------------------------------------------------------------------------------------------
def accumulate(case, frames, dst, one_pass):
    """The accumulation sequence on three frames: upload frames[0], step, upload frames[1], render TWICE (the second pass
    starts from the first one's output), step, upload frames[2], render.  one_pass(case, view, last, dst) -> the new field;
    returns the field after each of the three passes.  (After the second step `view` is the buffer that held frames[0] until
    frames[2] overwrites it, and `last` holds frames[1]: a rotation that forgot to swap would show frames[0] as `last`.)"""
    a = one_pass(case, frames[1], frames[0], dst)
    b = one_pass(case, frames[1], frames[0], a)
    c = one_pass(case, frames[2], frames[1], b)
    return [a, b, c]


def padded(case, pad_kind_seed=977):
    """The case inside a frame of twice its size, a border of noise all round: scaleUV and offset halved - exact in fp32 -
    put every tap on the texel it had, moved by (fw / 2, fh / 2).  Returns (the padded case, embed), embed(frame) -> the
    padded frame.  Exact only where the case's own coordinates are: the caller asserts with `taps` that every tap moved by
    exactly the border."""
    from helpers import noise_frame
    fw, fh = case["frame"]
    big = dict(case, name=case["name"] + "_padded", frame=[2 * fw, 2 * fh],
               uniforms=dict(case["uniforms"], scaleUV=[v / 2 for v in case["uniforms"]["scaleUV"]],
                             offset=case["uniforms"]["offset"] / 2))

    def embed(frame, seed):
        out = noise_frame(2 * fw, 2 * fh, pad_kind_seed + seed)
        out[fh // 2:fh // 2 + fh, fw // 2:fw // 2 + fw] = frame
        return out

    return big, embed
