"""Per-frame cost of the demo's colour-map blend at a 1920 x 1080 colour map (tendrils_amd/csrc/th_blend.hip), with the demo's
three views: two 128-bin audio textures and a 1280 x 720 RGBA8 camera frame that the context already holds.

  (a) host path   the blend in numpy on the host (float32, tap indices computed once, outside the timed window), then
                  th_colormap_upload of the w * h * 16 bytes from pageable memory: what a host had to do before the pass
                  existed.  Wall clock; th_colormap_upload returns after its copy.
  (b) device path th_texture_upload of the two audio textures, th_colormap_blend, th_sync.  Wall clock.
  kernel          th_colormap_blend alone: HIP events on the context's stream around --batch enqueued blends, per blend.
  copy floor      a device-to-device copy of the colour map's bytes (torch, its own events): the least its store stream costs.
(a) and (b) alternate in one process; medians of --reps after --warmup.  Both paths leave the same bits in the map (checked).

Usage: python tools/colormap_blend_bench.py [--reps 30] [--warmup 5] [--batch 50] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
FW, FH = 1280, 720
BINS = 128
ALPHAS = (0.1, 0.3, 0.8)
F = np.float32


def host_taps():
    """tap indices of the three views for every texel of the map (they depend on the shapes alone)"""
    uvx = ((np.arange(W, dtype=F) + F(0.5)) / F(W)).astype(F)
    uvy = ((np.arange(H, dtype=F) + F(0.5)) / F(H)).astype(F)
    ax = np.clip(np.floor((uvx * F(BINS)).astype(F)), 0, BINS - 1).astype(np.intp)

    def fx16(u, n):
        c = np.clip(u, F(0.0), F(65535.0 / 65536.0)).astype(F)
        return ((c * F(65536.0)).astype(F).astype(np.int64) * n) >> 16
    return ax, fx16(uvx, FW).astype(np.intp), fx16(uvy, FH).astype(np.intp)


def host_blend(mic, track, frame, taps, gl_blend=True):
    """the blend of the three views, float32, the shader's operation order (as tests/blend_restatement.py)"""
    ax, vx, vy = taps
    total = np.zeros((H, W, 4), F)
    for lum, alpha in ((mic, ALPHAS[0]), (track, ALPHAS[1])):
        row = lum[ax]                                       # (L, L, L, 1): a = 1 * alpha
        a = F(1.0) * F(alpha)
        total[..., :3] += (row * a)[None, :, None]
        total[..., 3] += a
    c = frame[vy[:, None], vx[None, :]].astype(F)
    c = (c * F(257.0)) * (F(1.0) / F(65535.0))
    a = c[..., 3] * F(ALPHAS[2])
    total[..., :3] += c[..., :3] * a[..., None]
    total[..., 3] += a
    if gl_blend:
        sa = total[..., 3:4]
        total = total * sa + np.zeros_like(total) * (F(1.0) - sa)
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("colormap_blend_bench: no GPU - nothing is measured without one")
    import tendrils_amd as ta
    from tendrils_amd import _capi
    from tendrils_amd._capi import call
    from tendrils_amd.tendrils import View

    rng = np.random.default_rng(7)
    t = ta.Tendrils(View(W, H))
    t.resize()
    t.setup(16)
    ctx = t.particles._ctx
    frame = rng.integers(0, 256, (FH, FW, 4), dtype=np.uint8)
    call("th_frames_resize", ctx, FW, FH)
    call("th_frames_upload", ctx, frame.ctypes.data_as(C.POINTER(C.c_uint8)))
    call("th_colormap_resize", ctx, W, H)
    views = (_capi.BlendView * 3)()
    for i, (source, index) in enumerate(((_capi.VIEW_TEXTURE, 0), (_capi.VIEW_TEXTURE, 1), (_capi.VIEW_FRAMES, 0))):
        views[i].source, views[i].index, views[i].alpha = source, index, ALPHAS[i]
    taps = host_taps()
    audio = [(rng.integers(0, 256, BINS).astype(F) / F(256.0)).astype(F) for _ in range(2 * (a.reps + a.warmup))]

    def device_path(mic, track):
        call("th_texture_upload", ctx, 0, _capi.TEX_L32F, mic.ctypes.data_as(C.c_void_p), BINS, 1)
        call("th_texture_upload", ctx, 1, _capi.TEX_L32F, track.ctypes.data_as(C.c_void_p), BINS, 1)
        call("th_colormap_blend", ctx, views, 3, 1, 1)
        call("th_sync", ctx)

    def read():
        out = np.empty((H, W, 4), F)
        call("th_colormap_download", ctx, out.ctypes.data_as(_capi._fp))
        return out

    # the two paths leave the same map
    device_path(audio[0], audio[1])
    on_device = read()
    on_host = host_blend(audio[0], audio[1], frame, taps)
    call("th_colormap_upload", ctx, on_host.ctypes.data_as(_capi._fp), W, H)
    same = bool((read().view(np.uint32) == on_device.view(np.uint32)).all())

    host_ms, upload_ms, device_ms = [], [], []
    for k in range(a.warmup + a.reps):
        mic, track = audio[2 * k], audio[2 * k + 1]
        t0 = time.perf_counter()
        blended = host_blend(mic, track, frame, taps)
        t1 = time.perf_counter()
        call("th_colormap_upload", ctx, blended.ctypes.data_as(_capi._fp), W, H)
        t2 = time.perf_counter()
        device_path(mic, track)
        t3 = time.perf_counter()
        if k >= a.warmup:
            host_ms.append((t1 - t0) * 1e3)
            upload_ms.append((t2 - t1) * 1e3)
            device_ms.append((t3 - t2) * 1e3)

    kernel_ms = []
    ms = C.c_float()
    for k in range(a.warmup + a.reps):
        call("th_timer_start", ctx)
        for _ in range(a.batch):
            call("th_colormap_blend", ctx, views, 3, 1, 1)
        call("th_timer_stop", ctx, C.byref(ms))
        if k >= a.warmup:
            kernel_ms.append(ms.value / a.batch)

    src = torch.empty(H * W * 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy_ms = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        if k >= a.warmup:
            copy_ms.append(e0.elapsed_time(e1) / a.batch)
    t.dispose()

    def med(v):
        return float(np.median(v))

    def spread(v):
        return [float(np.min(v)), float(np.max(v))]
    map_bytes = W * H * 16
    tap_bytes = W * H * (4 + 4 + 4)                       # what the lanes load: one float per audio view, one RGBA8 texel
    res = dict(map=[W, H], frame=[FW, FH], bins=BINS, reps=a.reps, warmup=a.warmup, batch=a.batch, same_bits=same,
               host_blend_ms=med(host_ms), host_upload_ms=med(upload_ms), host_path_ms=med(np.add(host_ms, upload_ms)),
               host_path_minmax_ms=spread(np.add(host_ms, upload_ms)),
               device_path_ms=med(device_ms), device_path_minmax_ms=spread(device_ms),
               kernel_ms=med(kernel_ms), kernel_minmax_ms=spread(kernel_ms), copy_ms=med(copy_ms), copy_minmax_ms=spread(copy_ms),
               map_bytes=map_bytes, kernel_store_gbs=map_bytes / med(kernel_ms) / 1e6,
               kernel_store_and_tap_gbs=(map_bytes + tap_bytes) / med(kernel_ms) / 1e6,
               copy_gbs_read_plus_write=2 * map_bytes / med(copy_ms) / 1e6)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
