"""Plain numpy restatement of flow-line drawing (src/flow-line/index.vert, index.frag, TRIANGLE_STRIP, SRC_ALPHA /
ONE_MINUS_SRC_ALPHA blending) - the yardstick the HIP path (tendrils_amd/csrc/th_flowline.hip) and the reference
captures (tests/golden/flowline_*.npz) are compared with.

The raster follows the conventions of the library's GeometrySpawner triangles: clip to the view volume, snap to 1/16
texel, spans ceil(left) <= x < ceil(right) per row, either winding drawn; a triangle with a vertex that is not finite
draws nothing.  Varyings are interpolated at texel centres with barycentrics of the unclipped triangle's SNAPPED
vertices (what the captured rasteriser does: interpolating from the exact window coordinates instead puts alpha 0.01
and time tens of ms off), the barycentrics in double; everything else fp32, in the shaders' operation order."""
import numpy as np

f32 = np.float32


def vertex(p, u):
    """Vertex stage for drawn point records p (dict of f32 arrays px, py, nx, ny, miter, qx, qy, time, dt) and side s
    (0: -miter, 1: +miter).  Returns clip x, y and varyings [.., 7] for both sides: arrays [n, 2]."""
    speed, rad, speed_limit = f32(u["speed"]), f32(u["rad"]), f32(u["speedLimit"])
    vx_, vy_ = f32(u["viewSize"][0]), f32(u["viewSize"][1])
    miter = np.stack([-p["miter"], p["miter"]], 1).astype(f32)
    sdf = np.sign(miter).astype(f32)
    rate = (speed / np.maximum(p["dt"], f32(1))).astype(f32)
    vx = ((p["px"] - p["qx"]) * rate).astype(f32)
    vy = ((p["py"] - p["qy"]) * rate).astype(f32)
    ln = np.sqrt(vx * vx + vy * vy).astype(f32)
    a = np.fmin((ln / speed_limit).astype(f32), f32(1))
    r = (rad * a).astype(f32)
    with np.errstate(all="ignore"):      # (equal consecutive points: infinite miters, NaN vertices)
        cx = ((p["px"][:, None] + p["nx"][:, None] * r[:, None] * miter) * vx_).astype(f32)
        cy = ((p["py"][:, None] + p["ny"][:, None] * r[:, None] * miter) * vy_).astype(f32)
    v = np.zeros(miter.shape + (7,), f32)
    v[..., 0] = vx[:, None]
    v[..., 1] = vy[:, None]
    v[..., 2] = p["time"][:, None]
    v[..., 3] = a[:, None]
    with np.errstate(all="ignore"):
        v[..., 4] = p["nx"][:, None] * miter
        v[..., 5] = p["ny"][:, None] * miter
    v[..., 6] = sdf
    return cx, cy, v


def clip_snap(cx, cy, w, h):
    """Clip a triangle (3 clip-space vertices, w = 1) to the view volume, snap; returns (X, Y) int lists or None."""
    cx, cy = [f32(c) for c in cx], [f32(c) for c in cy]
    one = f32(1)
    for plane in range(4):
        if len(cx) < 3:
            break
        tx, ty = [], []
        n = len(cx)
        for k in range(n):
            j = 0 if k == n - 1 else k + 1
            if plane == 0:
                di, dj = one + cx[k], one + cx[j]
            elif plane == 1:
                di, dj = one - cx[k], one - cx[j]
            elif plane == 2:
                di, dj = one - cy[k], one - cy[j]
            else:
                di, dj = one + cy[k], one + cy[j]
            if di >= 0:
                tx.append(cx[k]); ty.append(cy[k])
                if dj < 0:
                    D = one / f32(dj - di)
                    tx.append(f32(f32(dj * cx[k]) - f32(di * cx[j])) * D); ty.append(f32(f32(dj * cy[k]) - f32(di * cy[j])) * D)
            elif dj > 0:
                D = one / f32(di - dj)
                tx.append(f32(f32(di * cx[j]) - f32(dj * cx[k])) * D); ty.append(f32(f32(di * cy[j]) - f32(dj * cy[k])) * D)
        cx, cy = [f32(t) for t in tx], [f32(t) for t in ty]
    if len(cx) < 3:
        return None
    wx16, wy16 = f32(8) * f32(w), f32(8) * f32(h)
    ox, oy = wx16 - f32(8), wy16 - f32(8)
    X = [int(np.rint(f32(f32(c * wx16) + ox))) for c in cx]
    Y = [int(np.rint(f32(f32(c * wy16) + oy))) for c in cy]
    n = len(X)
    area2 = sum(X[k] * Y[(k + 1) % n] - X[(k + 1) % n] * Y[k] for k in range(n))
    if area2 == 0:
        return None
    if area2 > 0:
        X, Y = X[::-1], Y[::-1]
    return X, Y


def _ceil_div(a, b):
    return -((-a) // b)


def spans(X, Y, w, h):
    """{row: (left, right)} of a snapped polygon (the library's scanline rule)."""
    n = len(X)
    out = {}
    ys = [(min(Y) + 15) >> 4, ((max(Y) + 15) >> 4) - 1]
    for y in range(max(ys[0], 0), min(ys[1], h - 1) + 1):
        left, right = w, 0
        for e in range(n):
            en = 0 if e + 1 == n else e + 1
            Xa, Ya, Xb, Yb = X[e], Y[e], X[en], Y[en]
            if Ya == Yb:
                continue
            swap = Yb < Ya
            X1, Y1, X2, Y2 = (Xb, Yb, Xa, Ya) if swap else (Xa, Ya, Xb, Yb)
            if y < ((Y1 + 15) >> 4) or y >= ((Y2 + 15) >> 4):
                continue
            DX, DY = X2 - X1, Y2 - Y1
            ex = min(max(_ceil_div(DX * ((y << 4) - Y1) + X1 * DY, 16 * DY), 0), w)
            if swap:
                right = ex
            else:
                left = ex
        if left < right:
            out[y] = (left, right)
    return out


def records(points, times, closed, attributes):
    """Per drawn point records from th_flow_line_attributes' arrays (every other vertex)."""
    a = attributes
    return {"px": a["position"][0::2, 0], "py": a["position"][0::2, 1], "nx": a["normal"][0::2, 0], "ny": a["normal"][0::2, 1],
            "miter": a["miter"][1::2], "qx": a["previous"][0::2, 0], "qy": a["previous"][0::2, 1],
            "time": a["time"][0::2], "dt": a["dt"][0::2]}


def draw(flow, lines, u, coverage=None):
    """Draws `lines` (list of attribute dicts, draw order) into flow [h, w, 4] f32 in place; coverage (optional [h, w]
    int array) counts fragments."""
    h, w = flow.shape[:2]
    wx16, wy16 = f32(8) * f32(w), f32(8) * f32(h)
    ox, oy = wx16 - f32(8), wy16 - f32(8)
    cs = f32(u["crestShape"])
    for attrs in lines:
        if len(attrs["miter"]) == 0:
            continue
        p = records(None, None, None, attrs)
        cx, cy, v = vertex(p, u)
        nv = 2 * len(p["px"])
        CX, CY, V = cx.reshape(nv), cy.reshape(nv), v.reshape(nv, 7)
        for j in range(nv - 2):
            tx, ty, tv = CX[j:j + 3], CY[j:j + 3], V[j:j + 3]
            if not (np.isfinite(tx).all() and np.isfinite(ty).all()):
                continue
            poly = clip_snap(tx, ty, w, h)
            if poly is None:
                continue
            sp = spans(poly[0], poly[1], w, h)
            if not sp:
                continue
            ys = np.concatenate([np.full(r - l, y) for y, (l, r) in sp.items()])
            xs = np.concatenate([np.arange(l, r) for y, (l, r) in sp.items()])
            with np.errstate(all="ignore"):
                SX = np.rint((tx * wx16 + ox).astype(f32)).astype(np.float64)
                SY = np.rint((ty * wy16 + oy).astype(f32)).astype(np.float64)
            e1x, e1y, e2x, e2y = SX[1] - SX[0], SY[1] - SY[0], SX[2] - SX[0], SY[2] - SY[0]
            det = e1x * e2y - e2x * e1y
            inv = 1.0 / det if det != 0 else 0.0
            dx = 16.0 * xs.astype(np.float64) - SX[0]
            dy = 16.0 * ys.astype(np.float64) - SY[0]
            l1 = ((dx * e2y - dy * e2x) * inv).astype(f32)
            l2 = ((dy * e1x - dx * e1y) * inv).astype(f32)
            d1 = (tv[1] - tv[0]).astype(f32)
            d2 = (tv[2] - tv[0]).astype(f32)
            val = (tv[0][None, :] + l1[:, None] * d1[None, :] + l2[:, None] * d2[None, :]).astype(f32)
            with np.errstate(all="ignore"):
                dd = np.abs(val[:, 6])
                spd = (np.sqrt(val[:, 0] * val[:, 0] + val[:, 1] * val[:, 1]) * (f32(1) - dd)).astype(f32)
                t = (dd * cs).astype(f32)
                mx = (val[:, 0] * (f32(1) - t) + val[:, 4] * t).astype(f32)
                my = (val[:, 1] * (f32(1) - t) + val[:, 5] * t).astype(f32)
                iv = (f32(1) / np.sqrt(mx * mx + my * my)).astype(f32)
                src = np.stack([mx * iv * spd, my * iv * spd, val[:, 2], val[:, 3] - dd], 1).astype(f32)
                sa = src[:, 3:4]
                dst = flow[ys, xs]
                flow[ys, xs] = (src * sa + dst * (f32(1) - sa)).astype(f32)
            if coverage is not None:
                coverage[ys, xs] += 1
    return flow
