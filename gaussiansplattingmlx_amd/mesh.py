"""Mesh extraction (include/gsplat.h gs_tsdf_*): depth rendered from the training cameras is fused into a
truncated signed distance volume and the iso-surface is taken by marching tetrahedra -- the last step 2DGS, GOF, PGSR and
RaDe-GS all ship.  Both halves run in csrc/tsdf.hip; tests/tsdf_numpy.py restates them.

    mesh = extract_mesh(renderer, model.getParams(), cameras)        # a trainer user: trainer.gaussRender, its model
    write_mesh_ply("scene.ply", *mesh.cpu())

A model trained with filter_3d renders its surface only with the filter applied: pass BAKED parameters
(renderer.bakeFilter3D(params)), which any renderer shows as the filtered model.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .renderer import _p


class Mesh(namedtuple("Mesh", ["vertices", "faces", "colors"])):
    """vertices [V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 in 0 .. 1 or None; device tensors from extract()."""

    def cpu(self):
        return Mesh(*(None if t is None else t.detach().cpu().numpy() for t in self))


def _check_dims(dims):
    d = tuple(int(x) for x in dims)
    if len(d) != 3 or any(x < 2 or x > _lib.TSDF_MAX_DIM for x in d):
        raise ValueError(f"TSDFVolume: dims are three sizes in 2 .. {_lib.TSDF_MAX_DIM}, not {tuple(dims)}")
    if d[0] * d[1] * d[2] > _lib.TSDF_MAX_POINTS:
        raise ValueError(f"TSDFVolume: at most 2^28 lattice points, not {d[0] * d[1] * d[2]}")
    return d


def camera_view(camera, depth, color=None) -> _lib.gs_tsdf_view:
    """The gs_tsdf_view of a pinhole Camera and its device images: [R | t] out of worldViewTransform (p_view = [p, 1] @ view),
    the focal lengths and the principal point (the image centre for a camera without one)."""
    if getattr(camera, "model", "pinhole") != "pinhole":
        raise ValueError("TSDF integration maps lattice points through the pinhole model: a fisheye camera's depth cannot be "
                         "fused (undistort to a pinhole view first)")
    view = np.asarray(camera.worldViewTransform, np.float32).reshape(4, 4)
    v = _lib.gs_tsdf_view()
    for i, x in enumerate(np.ascontiguousarray(view.T[:3, :]).reshape(12)):
        v.Rt[i] = float(x)
    W, H = int(camera.imageWidth), int(camera.imageHeight)
    v.fx, v.fy = float(camera.focalX), float(camera.focalY)
    v.cx, v.cy = float(getattr(camera, "principalX", W / 2.0)), float(getattr(camera, "principalY", H / 2.0))
    v.width, v.height = W, H
    if depth.numel() != W * H or (color is not None and color.numel() != 3 * W * H):
        raise ValueError("TSDF integration: a depth image is [H, W] and a colour image [H, W, 3] of its camera's size")
    v.depth, v.color = depth.data_ptr(), (None if color is None else color.data_ptr())
    return v


class TSDFVolume:
    """A dense truncated signed distance volume on the renderer's device: lattice point (i, j, k) at origin + voxel (i, j, k),
    dims = (nx, ny, nz) lattice points (2 .. 1024 each, at most 2^28 together), trunc the truncation distance in world units.
    24 bytes per lattice point (tsdf, weight, rgb, colour weight), 16 of them without color."""

    def __init__(self, renderer, origin, voxel: float, dims, trunc: float, color: bool = True):
        self.dims = _check_dims(dims)
        if not (np.isfinite(voxel) and voxel > 0 and np.isfinite(trunc) and trunc > 0) or not np.isfinite(np.asarray(origin, np.float64)).all():
            raise ValueError("TSDFVolume: voxel and trunc are finite and > 0, the origin finite")
        self.r = renderer
        self.grid = _lib.gs_tsdf_grid()
        for i, x in enumerate(np.asarray(origin, np.float32).reshape(3)):
            self.grid.origin[i] = float(x)
        self.grid.voxel, self.grid.trunc = float(voxel), float(trunc)
        self.grid.nx, self.grid.ny, self.grid.nz = self.dims
        n = self.dims[0] * self.dims[1] * self.dims[2]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=renderer.device)      # noqa: E731
        self.tsdf, self.weight = z(n), z(n)
        self.rgb, self.cweight = (z(n, 3), z(n)) if color else (None, None)

    def integrate(self, cameras, depths, colors=None):
        """Fuses the views in order, GS_TSDF_MAX_VIEWS per launch (the volume is read and written once per launch): depths are
        [H, W] (or [H, W, 1]) view-space z images, 0 or non-finite = hole; colors, if given, [H, W, 3] per view."""
        r = self.r
        cams, depths = list(cameras), list(depths)
        colors = [None] * len(cams) if colors is None else list(colors)
        if len(depths) != len(cams) or len(colors) != len(cams):
            raise ValueError("TSDFVolume.integrate: one depth (and colour) image per camera")
        for at in range(0, len(cams), _lib.GS_TSDF_MAX_VIEWS):
            held = []          # (the device tensors whose addresses the views carry)
            views = (_lib.gs_tsdf_view * _lib.GS_TSDF_MAX_VIEWS)()
            k = 0
            for cam, d, c in zip(cams[at:at + 8], depths[at:at + 8], colors[at:at + 8]):
                d = r._t(d)
                c = None if c is None else r._t(c)
                held.append((d, c))
                views[k] = camera_view(cam, d, c)
                k += 1
            r._check(r.lib.gs_tsdf_integrate(r.ctx, C.byref(self.grid), k, views, _p(self.tsdf), _p(self.weight), _p(self.rgb),
                                             _p(self.cweight)))
        return self

    def extract(self, min_weight: float = 1) -> Mesh:
        """Marching tetrahedra over the cells whose corners all have weight >= min_weight: Mesh(vertices, faces, colors) as
        device tensors (colors None for a volume without color).  One host synchronisation (the counts)."""
        r = self.r
        nbytes = int(r.lib.gs_tsdf_mesh_workspace_bytes(C.byref(self.grid)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
        counts = (C.c_longlong * 2)()
        r._check(r.lib.gs_tsdf_mesh_plan(r.ctx, C.byref(self.grid), _p(self.tsdf), _p(self.weight), C.c_float(min_weight), _p(ws),
                                         nbytes, counts))
        V, F = int(counts[0]), int(counts[1])
        vertices = r._empty(V, 3)
        faces = r._empty(F, 3, dtype=torch.int32)
        colors = r._empty(V, 3) if self.rgb is not None else None
        r._check(r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(self.grid), _p(self.tsdf), _p(self.weight), _p(self.rgb), _p(self.cweight),
                                         C.c_float(min_weight), _p(ws), _p(vertices), _p(colors), _p(faces)))
        return Mesh(vertices, faces, colors)


def default_bounds(params):
    """(lo [3], hi [3]): the 1 % .. 99 % box of the means of the Gaussians with opacity above 0.5, padded by 5 % of its size."""
    xyz = torch.as_tensor(params["xyz"]).detach().float().reshape(-1, 3)
    op = torch.sigmoid(torch.as_tensor(params["opacity"]).detach().float().reshape(-1)).to(xyz.device)
    xyz = xyz[op > 0.5]
    n = int(xyz.shape[0])
    if n == 0:
        raise ValueError("extract_mesh: no Gaussian has opacity above 0.5; pass bounds=(lo, hi)")
    s = torch.sort(xyz, dim=0).values
    lo = s[int(np.floor(0.01 * (n - 1)))].cpu().numpy().astype(np.float64)
    hi = s[int(np.ceil(0.99 * (n - 1)))].cpu().numpy().astype(np.float64)
    pad = 0.05 * (hi - lo)
    return lo - pad, hi + pad


def volume_layout(bounds, resolution: int):
    """(origin, voxel, dims): `resolution` lattice points along the box's longest side, cubic voxels, every side covered."""
    lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError("extract_mesh: bounds are (lo, hi) with hi > lo on every axis")
    if int(resolution) < 2:
        raise ValueError("extract_mesh: resolution is at least 2")
    voxel = float((hi - lo).max()) / (int(resolution) - 1)
    dims = tuple(int(max(2, np.ceil((hi[a] - lo[a]) / voxel - 1e-9) + 1)) for a in range(3))
    return lo, voxel, dims


def extract_mesh(renderer, params, cameras, bounds=None, resolution: int = 256, trunc_voxels: float = 4.0, alpha_min: float = 0.5,
                 depth_max=None, min_weight=1, color: bool = True) -> Mesh:
    """The mesh of a Gaussian scene: every camera is rendered (renderForward(wantDepth=True)), its expected depth D / a where
    a >= alpha_min (expectedDepth; elsewhere, and beyond depth_max, a hole) is fused with its colour into a volume over `bounds`
    -- (lo, hi), None = default_bounds(params) -- of `resolution` lattice points along the longest side, truncated at
    trunc_voxels voxels, and marching tetrahedra extracts the cells seen min_weight times.  Cameras are pinhole (a fisheye camera
    is refused) and of the renderer's size.  The renderer's camera model is put back whatever happens."""
    cams = list(cameras)
    for cam in cams:
        if getattr(cam, "model", "pinhole") != "pinhole":
            raise ValueError("extract_mesh: TSDF integration maps lattice points through the pinhole model, so a fisheye camera's "
                             "depth cannot be fused (render pinhole views of the scene instead)")
    if not cams:
        raise ValueError("extract_mesh: no cameras")
    for cam in cams:
        if (int(cam.imageWidth), int(cam.imageHeight)) != (renderer.W, renderer.H):
            raise ValueError(f"extract_mesh: every camera is of the renderer's size {renderer.W} x {renderer.H}")
    origin, voxel, dims = volume_layout(default_bounds(params) if bounds is None else bounds, resolution)
    vol = TSDFVolume(renderer, origin, voxel, dims, float(trunc_voxels) * voxel, color=color)
    was = renderer.cameraModel
    try:
        batch = []
        for i, cam in enumerate(cams):
            res = renderer.renderForward(params, cam, wantDepth=True)
            d = renderer.expectedDepth(res, alpha_min)           # (a new tensor; the render's buffers are the next forward's)
            if depth_max is not None:
                d = torch.where(d > float(depth_max), torch.zeros_like(d), d)
            batch.append((cam, d, res.render.clone() if color else None))
            if len(batch) == _lib.GS_TSDF_MAX_VIEWS or i == len(cams) - 1:
                vol.integrate([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch] if color else None)
                batch = []
        return vol.extract(min_weight)
    finally:
        if renderer.cameraModel != was:
            renderer.setCameraModel(was)
