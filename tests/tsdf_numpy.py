"""Vectorised numpy restatement of mesh extraction (include/gsplat.h gs_tsdf_*): TSDF fusion of depth
images and marching tetrahedra on the Kuhn split.  dtype=np.float32 follows the kernels' written order of operations and is
what the GPU is compared with bit for bit; dtype=np.float64 is the same arithmetic in double.  It is the specification of the
case table (the winding and the 2-2 quad split), which is derived here from the stated rules, never typed in.

Lattice point (i, j, k) lies at origin + voxel (i, j, k) and has linear index i + nx (j + ny k).
"""
from __future__ import annotations

import numpy as np

# ---- the Kuhn split -----------------------------------------------------------------------------------------------------------
# tetrahedron t is the path (0,0,0) -> (1,1,1) adding the axes in the t-th permutation, lexicographic order; a corner is a 3-bit
# code (x = 1, y = 2, z = 4).  Its orientation det[v1 - v0, v2 - v0, v3 - v0] is the permutation's sign.
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
TET_CORNERS = np.array([[0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7] for p in PERMS])          # [6, 4] corner codes


def _even(p):
    p = list(p)
    return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) % 2 == 0


TET_NEGATIVE = np.array([not _even(p) for p in PERMS])                                       # tetrahedra 1, 2, 5
# the 7 edges a lattice point owns, towards ...; slot of an edge = SLOT_OF_BITS[code_b ^ code_a] (a the lower endpoint)
EDGE_DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
SLOT_OF_BITS = np.array([-1, 0, 1, 3, 2, 4, 5, 6])
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]      # a tetrahedron's six edges as pairs of path corners, a < b
_EID = {e: i for i, e in enumerate(TET_EDGES)}


def _e(a, b):
    return _EID[(min(a, b), max(a, b))]


def case_table():
    """(ntri[16], tri[16, 2, 3]) for a POSITIVE tetrahedron: bit c of the case = path corner c is inside (tsdf < 0); a negative
    tetrahedron takes the complemented case (which lists the same triangles reversed).  Triangles are triples of edge ids and
    are counter-clockwise seen from the outside (tsdf >= 0):
      one corner i inside: the edges (i, a), (i, b), (i, c) with (i, a, b, c) an even permutation of (0, 1, 2, 3), a the lowest;
      one corner i outside: those, reversed: (i, c), (i, b), (i, a);
      two inside p < q, two outside r < s: the quad pr, ps, qs, qr -- walked the other way round from pr (pr, qr, qs, ps) when
        (p, r, s, q) is an odd permutation -- cut along the diagonal from its first vertex: (c0, c1, c2), (c0, c2, c3).  The
        diagonal always joins the edge (lower inside, lower outside) to the edge (higher inside, higher outside)."""
    ntri = np.zeros(16, np.int64)
    tri = -np.ones((16, 2, 3), np.int64)
    for m in range(1, 15):
        ins = [c for c in range(4) if (m >> c) & 1]
        out = [c for c in range(4) if not (m >> c) & 1]
        if len(ins) == 2:
            (p, q), (r, s) = ins, out
            c = [_e(p, r), _e(p, s), _e(q, s), _e(q, r)]
            if not _even((p, r, s, q)):
                c = [c[0], c[3], c[2], c[1]]
            ntri[m] = 2
            tri[m] = [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
            continue
        i, (a, b, c) = (ins[0], out) if len(ins) == 1 else (out[0], ins)
        if not _even((i, a, b, c)):
            b, c = c, b
        t = [_e(i, a), _e(i, b), _e(i, c)]
        ntri[m] = 1
        tri[m, 0] = t if len(ins) == 1 else t[::-1]
    return ntri, tri


NTRI, TRI = case_table()


def make_grid(origin, voxel, dims, trunc):
    return dict(origin=np.asarray(origin, np.float32), voxel=np.float32(voxel), dims=tuple(int(d) for d in dims),
                trunc=np.float32(trunc))


def lattice_points(grid, dtype=np.float32):
    """[n, 3] positions origin + voxel (i, j, k), x fastest."""
    nx, ny, nz = grid["dims"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(dtype)
    return grid["origin"].astype(dtype)[None, :] + dtype(grid["voxel"]) * ijk


def empty_volume(grid, color=True, dtype=np.float32):
    n = int(np.prod(grid["dims"]))
    return dict(tsdf=np.zeros(n, dtype), weight=np.zeros(n, dtype), rgb=np.zeros((n, 3), dtype) if color else None,
                cweight=np.zeros(n, dtype) if color else None)


def integrate(grid, views, vol, dtype=np.float32, decisions=None):
    """Fuses `views` in order into vol (in place; arrays of `dtype`).  A view: dict(Rt [3, 4], fx, fy, cx, cy, depth [H, W],
    color [H, W, 3] or None).  decisions: a list that receives, per view, (pixel index or -1, s >= -trunc, s <= trunc) per
    voxel -- the integer decisions taken from float arithmetic."""
    T = dtype
    p = lattice_points(grid, T)
    trunc = T(grid["trunc"])
    tsdf, w, rgb, cw = vol["tsdf"], vol["weight"], vol["rgb"], vol["cweight"]
    with np.errstate(all="ignore"):
        for vw in views:
            Rt = np.asarray(vw["Rt"], np.float32).astype(T)
            fx, fy, cx, cy = (T(np.float32(vw[k])) for k in ("fx", "fy", "cx", "cy"))
            depth = np.asarray(vw["depth"], np.float32)
            H, W = depth.shape
            x, y, z = (((Rt[r, 0] * p[:, 0] + Rt[r, 1] * p[:, 1]) + Rt[r, 2] * p[:, 2]) + Rt[r, 3] for r in range(3))
            ok = (z > 0) & np.isfinite(z)
            u = fx * (x / z) + cx
            v = fy * (y / z) + cy
            fu, fv = np.floor(u), np.floor(v)
            ok &= (fu >= 0) & (fu <= T(W - 1)) & (fv >= 0) & (fv <= T(H - 1))
            pix = np.where(ok, fv, 0).astype(np.int64) * W + np.where(ok, fu, 0).astype(np.int64)
            d = depth.ravel()[pix].astype(T)
            ok &= (d > 0) & np.isfinite(d)
            s = d - z
            near = ok & ~(s < -trunc)
            f = np.minimum(T(1), s / trunc)
            tsdf[near] = ((tsdf * w + f) / (w + T(1)))[near]
            w[near] = (w + T(1))[near]
            col = near & (s <= trunc)
            if rgb is not None and vw.get("color") is not None:
                c = np.asarray(vw["color"], np.float32).reshape(-1, 3)[pix].astype(T)
                rgb[col] = ((rgb * cw[:, None] + c) / (cw[:, None] + T(1)))[col]
                cw[col] = (cw + T(1))[col]
            if decisions is not None:
                decisions.append((np.where(ok, pix, -1), near.copy(), col.copy()))
    return vol


def extract(grid, tsdf, weight, min_weight=1.0, rgb=None, cweight=None, dtype=np.float32):
    """Marching tetrahedra: (vertices [V, 3], faces [F, 3] int32, colors [V, 3] or None).  Vertices ascend in (owner's linear
    index * 7 + edge slot), triangles in (cell's linear index, tetrahedron, triangle)."""
    T = dtype
    nx, ny, nz = grid["dims"]
    f = np.asarray(tsdf).reshape(-1)
    wt = np.asarray(weight).reshape(-1)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = (i + nx * (j + ny * k)).ravel().astype(np.int64)                    # ascending: the cell order
    code_off = np.array([(c & 1) + nx * (((c >> 1) & 1) + ny * ((c >> 2) & 1)) for c in range(8)], np.int64)
    inside = f < 0
    with np.errstate(invalid="ignore"):
        seen = wt >= np.float32(min_weight)
    order_keys, tri_keys = [], []
    for t in range(6):
        codes = TET_CORNERS[t]
        idx = base[:, None] + code_off[codes][None, :]                         # [cells, 4] lattice indices of the path corners
        valid = seen[idx].all(1)
        m = (inside[idx] * (1 << np.arange(4))[None, :]).sum(1)
        if TET_NEGATIVE[t]:
            m = 15 - m
        nt = np.where(valid, NTRI[m], 0)
        for q in range(2):
            rows = np.nonzero(nt > q)[0]
            if rows.size == 0:
                continue
            e = TRI[m[rows], q]                                                # [rows, 3] edge ids
            a, b = np.array(TET_EDGES)[e, 0], np.array(TET_EDGES)[e, 1]        # path corners of each edge
            owner = np.take_along_axis(idx[rows], a, 1)
            slot = SLOT_OF_BITS[codes[b] ^ codes[a]]
            tri_keys.append(owner * 7 + slot)
            order_keys.append((base[rows] * 6 + t) * 2 + q)
    if not tri_keys:
        return np.zeros((0, 3), T), np.zeros((0, 3), np.int32), (None if rgb is None else np.zeros((0, 3), T))
    tri_keys = np.concatenate(tri_keys, 0)
    tri_keys = tri_keys[np.argsort(np.concatenate(order_keys), kind="stable")]
    keys, inv = np.unique(tri_keys.ravel(), return_inverse=True)
    faces = inv.reshape(-1, 3).astype(np.int32)
    owner, slot = keys // 7, keys % 7
    ia = np.stack([owner % nx, (owner // nx) % ny, owner // (nx * ny)], 1)
    ib = ia + EDGE_DIRS[slot]
    other = ib[:, 0] + nx * (ib[:, 1] + ny * ib[:, 2])
    org, vox = grid["origin"].astype(T)[None, :], T(grid["voxel"])
    pa, pb = org + vox * ia.astype(T), org + vox * ib.astype(T)
    fa, fb = f[owner].astype(T), f[other].astype(T)
    tt = fa / (fa - fb)
    vertices = pa + tt[:, None] * (pb - pa)
    colors = None
    if rgb is not None:
        ca, cb = np.asarray(rgb).reshape(-1, 3)[owner].astype(T), np.asarray(rgb).reshape(-1, 3)[other].astype(T)
        ha, hb = np.asarray(cweight).reshape(-1)[owner] != 0, np.asarray(cweight).reshape(-1)[other] != 0
        colors = ca + tt[:, None] * (cb - ca)
        colors = np.where((ha & ~hb)[:, None], ca, colors)
        colors = np.where((~ha & hb)[:, None], cb, colors)
        colors = np.where((~ha & ~hb)[:, None], T(0.5), colors)
    return vertices.astype(T), faces, colors


# ---- what a test asks of a mesh -------------------------------------------------------------------------------------------------
def mesh_invariants(faces, n_vertices):
    """dict: V, E, F, euler, max / min triangles per undirected edge, directed edges that occur twice, directed edges without
    their reverse, triangles that repeat an index, unreferenced vertices."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    dk = d[:, 0] * (n_vertices + 1) + d[:, 1]
    rk = d[:, 1] * (n_vertices + 1) + d[:, 0]
    _, dcount = np.unique(dk, return_counts=True)
    u = np.sort(d, 1)
    _, ucount = np.unique(u[:, 0] * (n_vertices + 1) + u[:, 1], return_counts=True)
    rep = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    used = np.zeros(n_vertices, bool)
    used[faces.ravel()] = True
    E = int(ucount.size)
    return dict(V=int(n_vertices), E=E, F=int(faces.shape[0]), euler=int(n_vertices) - E + int(faces.shape[0]),
                edge_max=int(ucount.max()) if E else 0, edge_min=int(ucount.min()) if E else 0,
                directed_repeats=int((dcount > 1).sum()), unpaired=int((~np.isin(dk, rk)).sum()),
                degenerate_index=int(rep.sum()), unreferenced=int((~used).sum()))


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- the analytic grids and the integrate scene the CPU and GPU tests share ------------------------------------------------------
def analytic_grid(kind):
    """(grid, tsdf float32 [n], weight float32 [n]) of the named case."""
    if kind in ("sphere", "torus", "half"):
        n, lo, hi = 12, -1.0, 1.0
    elif kind == "zeros":
        n, lo, hi = 9, -1.0, 1.0
    elif kind == "offcentre":
        grid = make_grid((-0.9, -0.7, -0.5), 0.1, (20, 17, 13), 0.3)
        p = lattice_points(grid, np.float64)
        d = np.linalg.norm(p - np.array([0.12, 0.05, 0.07]), axis=1) - 0.45
        return grid, np.clip(d, -0.3, 0.3).astype(np.float32), np.ones(p.shape[0], np.float32)
    else:
        raise ValueError(kind)
    voxel = (hi - lo) / (n - 1)
    grid = make_grid((lo, lo, lo), voxel, (n, n, n), 3 * voxel)
    p = lattice_points(grid, np.float64)             # (the 9^3 grid's voxel is 0.25: its lattice points are exact)
    if kind == "torus":
        d = np.hypot(np.hypot(p[:, 0], p[:, 1]) - 0.6, p[:, 2]) - 0.25
    else:
        d = np.linalg.norm(p, axis=1) - (0.5 if kind == "zeros" else 0.6)
    w = np.ones(p.shape[0], np.float32)
    if kind == "half":
        w[p[:, 0] < 0.05] = 0.0
    return grid, np.clip(d, -3 * voxel, 3 * voxel).astype(np.float32), w


def look_at_Rt(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Row-major 3 x 4 world-to-view [R | t] of an OpenCV camera (x right, y down, z forward) at `eye`."""
    eye = np.asarray(eye, np.float64)
    fwd = np.asarray(target, np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], 0)
    return np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32)


def sphere_depth(Rt, fx, fy, cx, cy, W, H, centre, radius):
    """View-space z of the first hit of the pixel centres' rays with a sphere (float64 -> float32), 0 where they miss."""
    R, t = np.asarray(Rt, np.float64)[:, :3], np.asarray(Rt, np.float64)[:, 3]
    c = R @ np.asarray(centre, np.float64) + t
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)                      # z = 1 along the ray
    A, B, C = (d * d).sum(-1), -2.0 * (d @ c), c @ c - radius * radius
    disc = B * B - 4 * A * C
    z = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 0.0)
    return np.where(z > 0, z, 0.0).astype(np.float32)


def integrate_scene(n_views=3):
    """The integrate parity scene: a 20 x 17 x 13 grid, `n_views` views of 96 x 80 with off-centre principal points looking at an
    analytic sphere; view 0's depth carries a block of zeros and one NaN pixel; every view has a colour image."""
    grid = make_grid((-0.95, -0.8, -0.6), 0.1, (20, 17, 13), 0.3)
    W, H = 96, 80
    views = []
    rng = np.random.default_rng(7)
    for i in range(n_views):
        a = 0.7 + 2.0 * np.pi * i / max(n_views, 3)
        eye = (3.0 * np.cos(a), 3.0 * np.sin(a), 0.8 + 0.3 * (i % 3))
        Rt = look_at_Rt(eye, target=(0.02, -0.03, 0.01))
        fx, fy, cx, cy = 118.0 + i, 121.0 - i, 44.3 + 1.7 * (i % 4), 43.6 - 1.3 * (i % 3)
        depth = sphere_depth(Rt, fx, fy, cx, cy, W, H, (0.05, 0.0, 0.02), 0.55)
        if i == 0:
            depth[30:40, 40:52] = 0.0
            depth[45, 47] = np.nan
        color = rng.random((H, W, 3)).astype(np.float32)
        views.append(dict(Rt=Rt, fx=np.float32(fx), fy=np.float32(fy), cx=np.float32(cx), cy=np.float32(cy), depth=depth,
                          color=color))
    return grid, views
