"""Times mesh extraction and prints ONE JSON line: one 8-view gs_tsdf_integrate launch against eight
one-view launches of the same kernel, and the plan and emit calls, on a 256^3 volume with 8 views of 800 x 800 looking at an
analytic sphere.  Device events around each form, the two forms alternating, after warm-up; median, min and max over the repeats.
Bytes are what the kernel must move, computed from the shapes and from how many voxels the views touch.

Every timed window holds --inner calls (a window of a fraction of a millisecond would measure the clock), reported per call.

    python tools/tsdf_time.py [--res 256] [--size 800] [--reps 20] [--inner 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussiansplattingmlx_amd import _lib  # noqa: E402
from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w  # noqa: E402
from gaussiansplattingmlx_amd.mesh import TSDFVolume, camera_view  # noqa: E402
from gaussiansplattingmlx_amd.renderer import GaussianRenderer, _p  # noqa: E402


def sphere_depth(cam, radius, device):
    """View-space z of the pixel centres' first hit with the sphere |p| = radius (float64 on the device), 0 where they miss."""
    W, H = cam.imageWidth, cam.imageHeight
    view = torch.as_tensor(np.asarray(cam.worldViewTransform, np.float64), device=device)
    c = view[3, :3]                                     # the origin in view space
    v, u = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64) + 0.5,
                          torch.arange(W, device=device, dtype=torch.float64) + 0.5, indexing="ij")
    d = torch.stack([(u - cam.principalX) / float(cam.focalX), (v - cam.principalY) / float(cam.focalY), torch.ones_like(u)], -1)
    A, B, Cc = (d * d).sum(-1), -2.0 * (d @ c), float(c @ c) - radius * radius
    disc = B * B - 4 * A * Cc
    z = torch.where(disc > 0, (-B - torch.sqrt(disc.clamp(min=0))) / (2 * A), torch.zeros_like(A))
    return torch.where(z > 0, z, torch.zeros_like(z)).float().contiguous()


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_time: needs a GPU (a time taken anywhere else says nothing)")
    r = GaussianRenderer(4, 64, 64)                     # (the context; nothing is rendered)
    n = a.res ** 3
    voxel = 2.0 / (a.res - 1)
    vol = TSDFVolume(r, (-1.0, -1.0, -1.0), voxel, (a.res,) * 3, 4.0 * voxel)
    cams = []
    for k in range(8):
        ang = 2 * np.pi * k / 8 + 0.1
        cams.append(Camera(a.size, a.size, 1.1 * a.size, 1.1 * a.size, look_at_c2w((3.0 * np.cos(ang), 3.0 * np.sin(ang), 0.7 * (k % 3 - 1)))))
    depths = [sphere_depth(c, 0.7, r.device) for c in cams]
    colors = [torch.rand(a.size, a.size, 3, device=r.device) for _ in cams]
    views = (_lib.gs_tsdf_view * 8)(*[camera_view(c, d, col) for c, d, col in zip(cams, depths, colors)])
    ones = [(_lib.gs_tsdf_view * 1)(views[k]) for k in range(8)]
    args = (_p(vol.tsdf), _p(vol.weight), _p(vol.rgb), _p(vol.cweight))

    def batched():
        r._check(r.lib.gs_tsdf_integrate(r.ctx, C.byref(vol.grid), 8, views, *args))

    def one_by_one():
        for k in range(8):
            r._check(r.lib.gs_tsdf_integrate(r.ctx, C.byref(vol.grid), 1, ones[k], *args))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for _ in range(a.warmup):
        batched()
        one_by_one()
    torch.cuda.synchronize()
    tb, to = [], []
    for _ in range(a.reps):
        tb.append(timed(batched))
        to.append(timed(one_by_one))
    # what one pass over the volume must move: 24 B read per voxel, 8 B written per touched voxel, 16 B more per coloured one;
    # a one-view launch touches its own view's voxels only
    w0 = vol.weight.clone()
    c0 = vol.cweight.clone()
    batched()
    touched, coloured = int((vol.weight != w0).sum()), int((vol.cweight != c0).sum())
    per_view_touched = per_view_coloured = 0
    for k in range(8):
        w0.copy_(vol.weight)
        c0.copy_(vol.cweight)
        r._check(r.lib.gs_tsdf_integrate(r.ctx, C.byref(vol.grid), 1, ones[k], *args))
        per_view_touched += int((vol.weight != w0).sum())
        per_view_coloured += int((vol.cweight != c0).sum())
    bytes_batched = 24 * n + 8 * touched + 16 * coloured
    bytes_single = 8 * 24 * n + 8 * per_view_touched + 16 * per_view_coloured
    out = dict(tool="tsdf_time", device=torch.cuda.get_device_name(0), res=a.res, views=8, image=a.size, reps=a.reps, inner=a.inner, warmup=a.warmup,
               integrate_8_views_one_launch=dict(stats(tb), volume_bytes=bytes_batched),
               integrate_8_views_eight_launches=dict(stats(to), volume_bytes=bytes_single),
               touched_voxels=touched, coloured_voxels=coloured)
    for k in ("integrate_8_views_one_launch", "integrate_8_views_eight_launches"):
        out[k]["volume_gb_per_s"] = out[k]["volume_bytes"] / (out[k]["median_ms"] * 1e-3) / 1e9
    # plan (ends in a host synchronisation: a host clock) and emit (device events) on the fused volume
    nbytes = int(r.lib.gs_tsdf_mesh_workspace_bytes(C.byref(vol.grid)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
    counts = (C.c_longlong * 2)()
    tp, te = [], []
    for i in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            r._check(r.lib.gs_tsdf_mesh_plan(r.ctx, C.byref(vol.grid), _p(vol.tsdf), _p(vol.weight), C.c_float(1.0), _p(ws), nbytes, counts))
        t1 = time.perf_counter()
        V, F = int(counts[0]), int(counts[1])
        vert, cols, faces = r._empty(V, 3), r._empty(V, 3), r._empty(F, 3, dtype=torch.int32)
        ms = timed(lambda: r._check(r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(vol.grid), _p(vol.tsdf), _p(vol.weight), _p(vol.rgb),
                                                            _p(vol.cweight), C.c_float(1.0), _p(ws), _p(vert), _p(cols), _p(faces))))
        if i >= a.warmup:
            tp.append((t1 - t0) * 1e3 / a.inner)
            te.append(ms)
    # plan: memset 7 n, mark reads 8 n and writes the flags it sets + 4 n, compact reads 7 n and writes 5 n, two scans read 4 n twice
    # and write 4 n each; emit: vertices reads 5 n (+ per vertex), faces reads 8 n + 9 n of masks and offsets (cached neighbours)
    out["mesh_plan"] = dict(stats(tp), workspace_bytes=nbytes, min_bytes=(7 + 8 + 4 + 7 + 5 + 24) * n)
    out["mesh_emit"] = dict(stats(te), vertices=V, faces=F, min_bytes=(5 + 8 + 9) * n + 24 * V + 12 * F)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
