"""Host-side mirror of Data/PlyWriter.swift over the C ABI: the reference's static methods, same names.

Tensors are device tensors (or anything the renderer can move to the device); the interleave / de-interleave runs on
the GPU and the file bytes are those of the reference writer.

write_mesh_ply / read_mesh_ply are the triangle-mesh file of mesh.extract_mesh, written on the host."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from .renderer import GaussianRenderer, _p


_MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_mesh_ply(path, vertices, faces, colors=None):
    """A triangle mesh (mesh.Mesh.cpu(), or any arrays / tensors) as a binary little-endian PLY: per vertex x, y, z float32 and
    red, green, blue uchar (colors in 0 .. 1, clamped and rounded to nearest; mid grey without), per face a `uchar int` list."""
    v, f, c = (None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
               for t in (vertices, faces, colors))
    v, f = v.reshape(-1, 3), f.reshape(-1, 3)
    if c is not None and c.reshape(-1, 3).shape[0] != v.shape[0]:
        raise ValueError("write_mesh_ply: one colour per vertex")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("write_mesh_ply: a face index outside the vertices")
    rows = np.zeros(v.shape[0], _MESH_VERTEX)
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    rgb = np.full((v.shape[0], 3), 128, np.uint8) if c is None else \
        np.floor(np.clip(np.nan_to_num(c.reshape(-1, 3).astype(np.float64)), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    tris = np.zeros(f.shape[0], _MESH_FACE)
    tris["n"], tris["v"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(os.fspath(path), "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(tris.tobytes())


def read_mesh_ply(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, colors [V, 3] uint8) of a file write_mesh_ply wrote."""
    with open(os.fspath(path), "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("read_mesh_ply: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_mesh_ply: binary little-endian PLY only")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    want = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
            "property uchar blue", "property list uchar int vertex_indices"]
    if props != want or list(counts) != ["vertex", "face"]:
        raise ValueError("read_mesh_ply: not the layout write_mesh_ply writes")
    body = end + len(b"end_header\n")
    V, F = counts["vertex"], counts["face"]
    if len(data) != body + V * _MESH_VERTEX.itemsize + F * _MESH_FACE.itemsize:
        raise ValueError("read_mesh_ply: truncated or oversized file")
    rows = np.frombuffer(data, _MESH_VERTEX, V, body)
    tris = np.frombuffer(data, _MESH_FACE, F, body + V * _MESH_VERTEX.itemsize)
    if F and not (tris["n"] == 3).all():
        raise ValueError("read_mesh_ply: triangles only")
    return (np.stack([rows["x"], rows["y"], rows["z"]], 1).astype(np.float32).reshape(-1, 3), tris["v"].astype(np.int32).reshape(-1, 3),
            np.stack([rows["red"], rows["green"], rows["blue"]], 1).reshape(-1, 3))


class PlyWriter:
    def __init__(self, renderer: GaussianRenderer):
        self.r = renderer

    def writeGaussianBinary(self, positions, features_dc, features_rest, opacities, scales, rotations, to):
        """PlyWriter.writeGaussianBinary(positions:features_dc:features_rest:opacities:scales:rotations:to:)
        (Data/PlyWriter.swift:116-146).  features_rest must be [N, M, 3] (the reference's precondition, :131)."""
        r = self.r
        t = [r._t(x) for x in (positions, features_dc, features_rest, opacities, scales, rotations)]
        N = int(t[0].shape[0])
        if t[2].dim() != 3 or t[2].shape[2] != 3:
            raise ValueError("features_rest must be [N, M, 3]")
        sizes = [3, 3, 3 * int(t[2].shape[1]), 1, 3, 4]
        for x, n in zip(t, sizes):
            if x.numel() != N * n:
                raise ValueError("Attribute array size mismatch")          # PlyWriter.swift:34-43
        K = int(t[2].shape[1]) + 1
        r._check(r.lib.gs_ply_write(r.ctx, os.fsencode(os.fspath(to)), N, K, *[_p(x) for x in t]))

    def probe(self, url):
        n, m, d = C.c_longlong(), C.c_int(), C.c_int()
        r = self.r
        r._check(r.lib.gs_ply_probe(r.ctx, os.fsencode(os.fspath(url)), C.byref(n), C.byref(m), C.byref(d)))
        return int(n.value), int(m.value), int(d.value)

    def loadGaussianBinaryPLYAsMLX(self, url):
        """PlyWriter.loadGaussianBinaryPLYAsMLX (Data/PlyWriter.swift:235-265): the six tensors, on the device, in
        the reference's shapes -- positions [N,3], features_dc [N,1,3], features_rest [N,M,3], opacities [N,1],
        scales [N,3], rotations [N,4]."""
        r = self.r
        N, M, D = self.probe(url)
        out = dict(positions=r._empty(N, 3), features_dc=r._empty(N, 1, 3), features_rest=r._empty(N, M, 3),
                   opacities=r._empty(N, 1), scales=r._empty(N, 3), rotations=r._empty(N, 4))
        if D != 3:
            raise ValueError("features_rest_shape must be M 3")
        r._check(r.lib.gs_ply_load(r.ctx, os.fsencode(os.fspath(url)), N, M + 1, _p(out["positions"]),
                                   _p(out["features_dc"]), _p(out["features_rest"]), _p(out["opacities"]),
                                   _p(out["scales"]), _p(out["rotations"])))
        return out

    def packRows(self, positions, features_dc, features_rest, opacities, scales, rotations) -> torch.Tensor:
        r = self.r
        t = [r._t(x) for x in (positions, features_dc, features_rest, opacities, scales, rotations)]
        N, K = int(t[0].shape[0]), int(t[2].shape[1]) + 1
        rows = r._empty(N, 14 + 3 * (K - 1))
        r._check(r.lib.gs_ply_pack_rows(r.ctx, N, K, *[_p(x) for x in t], _p(rows)))
        return rows
