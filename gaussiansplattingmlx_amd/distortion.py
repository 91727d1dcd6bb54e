"""The depth distortion loss (include/gsplat.h gs_blend_distortion / gs_render_distortion): 2DGS's eq. 13,
gsplat's `distloss`, the term GOF, PGSR and RaDe-GS train their surfaces with as well.

It pulls the blend weights of a ray together in depth.  Per pixel, over the entries i of its list up to its stop, with the blend
weights of contrib_prune.py (w_i = T alpha, T <- T (1 - alpha), clamp 0.99, a pixel stops after the entry with T < 1e-4) and the
mapped depth m_i = map(z_i) of the record's depth (column 10 of the packed record):

    D = sum_{i<j} w_i w_j (m_i - m_j)^2  =  A S,     A = sum w_i,  mu = sum w_i m_i / A,  S = sum w_i (m_i - mu)^2

2DGS's convention: every unordered pair once, the weights not normalised.  (A, mu, S) are carried with the weighted Welford
update  A' = A + w,  mu' = mu + (w / A') (m - mu),  S' = S + w (m - mu) (m - mu'),  which cancels nothing on thin distributions;
A M2 - M1^2 and 2DGS's running prefix form both do, in float32 (moments_form below is the former, kept to show it).  The update
runs on m - c, c the m of the pixel's first weighted entry, so that the running mean is as small as the deviations it is
subtracted from; the reported mean is c + mu.  With the pixel's totals

    dD/dw_i = g_i = A (m_i - mu)^2 + S,    dD/dm_i = 2 w_i A (m_i - mu),
    dD/dalpha_i = T_i g_i - R_i / (1 - alpha_i),    R_i = sum_{j>i} g_j w_j = 2 D - sum_{j<=i} g_j w_j,

and from alpha_i into mean, conic and opacity with the blend backward's derivatives (the clamp passes the gradient iff raw <= 0.99,
the floor of 1 - alpha is 1e-6), from m_i into the depth through map'(z).  Maps: "ndc", m = far / (far - near) (1 - near / z),
2DGS's with its near 0.2 and far 1000, and "linear", m = z, gsplat's.

The step's loss gains  weight (1 / (H W)) sum_p v_p D_p,  v_p the step's loss-mask weight (v / 255) where a loss mask is set,
else 1: divided by all pixels, as the masked colour loss is.

tile_distortion / tile_distortion_vjp are the host-side statements of what csrc/distortion.hip computes in float32, for tests
and tools -- float64 by default; with dtype=np.float32 they follow the kernels' operation order.  DistortionConfig holds the
trainer's settings: GaussianTrainer(distortion=DistortionConfig(...)).

Not here: median depth, normals from the Gaussians' own axes, normalised (Mip-NeRF 360) weights,
data-parallel and multi-view steps, fisheye cameras.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .contrib_prune import ALPHA_MAX, T_STOP

MAPS = ("ndc", "linear")          # GS_DISTORTION_NDC, GS_DISTORTION_LINEAR
ONE_MINUS_ALPHA_MIN = 1e-6        # the floor of 1 - alpha in dD/dalpha (blend.hip bwd_step)
GRAD_COLUMNS = (0, 1, 2, 3, 4, 5, 9, 10)      # the packed columns the term has a gradient in: mean, conic, opacity, depth


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


@dataclass
class DistortionConfig:
    """weight: the term's weight in the step's loss (2DGS: 100 on bounded scenes, 1000 .. 10000 on unbounded ones with the "ndc"
    map).  start: the first iteration that runs the term (2DGS: 3000); before it the step is the step without distortion=.
    map: "ndc" (2DGS: m = far / (far - near) (1 - near / z)) or "linear" (gsplat: m = z).  near, far: the "ndc" map's planes."""
    weight: float = 100.0
    start: int = 3000
    map: str = "ndc"
    near: float = 0.2
    far: float = 1000.0

    def validate(self):
        if not _number(self.weight) or not (math.isfinite(self.weight) and self.weight >= 0.0):
            raise ValueError("DistortionConfig: weight is finite and >= 0")
        if isinstance(self.start, bool) or not isinstance(self.start, int) or self.start < 0:
            raise ValueError("DistortionConfig: start is an integer >= 0")
        if self.map not in MAPS:
            raise ValueError(f"DistortionConfig: map is one of {', '.join(repr(m) for m in MAPS)}")
        if not (_number(self.near) and _number(self.far) and math.isfinite(self.near) and math.isfinite(self.far)
                and 0.0 < self.near < self.far):
            raise ValueError("DistortionConfig: near and far are finite with 0 < near < far")
        return self

    def params(self):
        """The term's gs_distortion_params."""
        from . import _lib
        return _lib.gs_distortion_params(MAPS.index(self.map), float(self.near), float(self.far))


def map_depth(z, map="ndc", near=0.2, far=1000.0, dtype=np.float64):
    """(m, dm/dz) of the depths z in `dtype`; near and far are rounded to float32 first, as the library takes them."""
    dtype = np.dtype(dtype).type
    if map not in MAPS:
        raise ValueError(f"map is one of {', '.join(repr(m) for m in MAPS)}")
    z = np.asarray(z, dtype)
    if map == "linear":
        return z, np.ones_like(z)
    near, far = np.float32(near), np.float32(far)
    scale = dtype(far / (far - near))             # (formed in float32 on the host, as the launcher does)
    near = dtype(near)
    with np.errstate(divide="ignore", invalid="ignore"):
        return scale * (dtype(1.0) - near / z), scale * near / (z * z)


def _tiles(packed, sortedIdx, tileRanges, W, H, tileW, tileH, dtype):
    """Per tile with a list: (rows, columns, the pixel coordinates as `dtype` grids, the list's Gaussian indices)."""
    idx = np.asarray(sortedIdx).astype(np.int64).reshape(-1)
    ranges = np.asarray(tileRanges).astype(np.int64).reshape(-1, 2)
    gridW = (W + tileW - 1) // tileW
    for tile in range(ranges.shape[0]):
        s, e = ranges[tile]
        if e <= s:
            continue
        ty, tx = divmod(tile, gridW)
        ys, xs = np.arange(ty * tileH, min(H, (ty + 1) * tileH)), np.arange(tx * tileW, min(W, (tx + 1) * tileW))
        if ys.size == 0 or xs.size == 0:
            continue
        py, px = (a.astype(dtype) for a in np.meshgrid(ys, xs, indexing="ij"))
        yield ys, xs, py, px, idx[s:e]


def _alpha(r, px, py, dtype):
    """contrib_prune.blend_weights' alpha of the record r on the pixels, with the terms the backward needs again."""
    dx, dy = px - r[0], py - r[1]
    dxdy = dx * dy
    q = -dtype(0.5) * (dx * dx * r[2] + dy * dy * r[5] + dxdy * r[3] + dxdy * r[4])
    ex = np.exp(q)
    raw = ex * r[9]
    return dx, dy, dxdy, ex, raw, np.minimum(raw, dtype(ALPHA_MAX))


def tile_distortion(packed, sortedIdx, tileRanges, W, H, tileW, tileH, map="ndc", near=0.2, far=1000.0, dtype=np.float64):
    """(D [H, W], totals [H, W, 3] = (A, mu, S)) of one view from its packed records [N, 11] and tile lists, in `dtype`: the
    Welford sweep of the module's docstring in list order.  Pixels with nothing blended are zeros."""
    dtype = np.dtype(dtype).type
    P = np.asarray(packed, dtype).reshape(-1, 11)
    m_all, _ = map_depth(P[:, 10], map, near, far, dtype)
    one, stop, zero = dtype(1.0), dtype(T_STOP), dtype(0.0)
    totals = np.zeros((H, W, 3), dtype)
    for ys, xs, py, px, gs in _tiles(P, sortedIdx, tileRanges, W, H, tileW, tileH, dtype):
        T = np.ones(py.shape, dtype)
        live = np.ones(py.shape, bool)
        A, mu, S, c = (np.zeros(py.shape, dtype) for _ in range(4))      # mu: of m - c
        for g in gs:
            if not live.any():
                break
            alpha = _alpha(P[g], px, py, dtype)[5]
            w = np.where(live, T * alpha, zero)
            pos = w > zero                       # (w = 0 changes nothing, and A' could still be 0)
            c = np.where(pos & (A == zero), m_all[g], c)     # the pixel's first weighted entry: the origin of the rest
            e = m_all[g] - c
            An = A + w
            d = e - mu
            mun = mu + (w / np.where(pos, An, one)) * d
            S = np.where(pos, S + (w * d) * (e - mun), S)
            A, mu = np.where(pos, An, A), np.where(pos, mun, mu)
            T = np.where(live, T * (one - alpha), T)
            live &= ~(T < stop)
        totals[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = np.stack([A, c + mu, S], axis=-1)
    return totals[..., 0] * totals[..., 2], totals


def tile_distortion_vjp(packed, sortedIdx, tileRanges, W, H, tileW, tileH, cot, map="ndc", near=0.2, far=1000.0,
                        dtype=np.float64, totals=None, N=None):
    """The gradient rows [N, 11] (packed column order; the colour columns stay 0) of sum_p cot[p] D[p] for the cotangent image
    cot [H, W], in `dtype`: a second front-to-back sweep with the prefix of g_j w_j beside T, R_i as 2 D minus it.  totals:
    tile_distortion(...)[1] of the same view in the same dtype, if at hand.  Rows of Gaussians that weigh on no pixel are exactly 0."""
    dtype = np.dtype(dtype).type
    P = np.asarray(packed, dtype).reshape(-1, 11)
    if N is None:
        N = P.shape[0]
    if totals is None:
        totals = tile_distortion(P, sortedIdx, tileRanges, W, H, tileW, tileH, map, near, far, dtype)[1]
    ct = np.asarray(cot, dtype).reshape(H, W)
    m_all, dm_all = map_depth(P[:, 10], map, near, far, dtype)
    one, two, half, stop, zero = dtype(1.0), dtype(2.0), dtype(0.5), dtype(T_STOP), dtype(0.0)
    amax, floor = dtype(ALPHA_MAX), dtype(ONE_MINUS_ALPHA_MIN)
    rows = np.zeros((N, 11), dtype)
    for ys, xs, py, px, gs in _tiles(P, sortedIdx, tileRanges, W, H, tileW, tileH, dtype):
        sl = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
        cp, A, mu, S = ct[sl], totals[sl + (0,)], totals[sl + (1,)], totals[sl + (2,)]
        twoD = two * (A * S)
        T = np.ones(py.shape, dtype)
        Pfx = np.zeros(py.shape, dtype)
        live = cp != zero                        # (a pixel the loss does not see adds zeros: it is done from the start)
        for g in gs:
            if not live.any():
                break
            r = P[g]
            dx, dy, dxdy, ex, raw, alpha = _alpha(r, px, py, dtype)
            w = T * alpha
            d = m_all[g] - mu
            Ad = A * d
            gi = Ad * d + S
            Pfx = np.where(live, Pfx + gi * w, Pfx)
            R = twoD - Pfx
            denom = np.maximum(one - alpha, floor)
            dAlpha = cp * (T * gi - R * (one / denom))
            S32 = np.where(raw > amax, zero, dAlpha)
            exS = ex * S32
            S36 = -half * (r[9] * exS)
            S39 = dy * (r[5] * S36)
            S41 = dx * (r[2] * S36)
            S42 = r[4] * S36 + r[3] * S36
            c01 = dxdy * S36
            vals = (-(S41 + S41 + dy * S42), -(S39 + S39 + dx * S42), dx * dx * S36, c01, c01, dy * dy * S36, exS,
                    cp * ((two * w) * Ad) * dm_all[g])
            for col, v in zip(GRAD_COLUMNS, vals):
                rows[g, col] += np.where(live, v, zero).sum(dtype=dtype)
            T = np.where(live, T * (one - alpha), T)
            live &= ~(T < stop)
    return rows


def moments_form(w, m, dtype=np.float32):
    """D of one pixel as A M2 - M1^2 (A = sum w, M1 = sum w m, M2 = sum w m^2) in `dtype`, in list order: the form the kernels do
    NOT use.  On a thin distribution the two products agree in their leading digits and the difference is rounding noise."""
    dtype = np.dtype(dtype).type
    w, m = np.asarray(w, dtype), np.asarray(m, dtype)
    A = M1 = M2 = dtype(0.0)
    for wi, mi in zip(w, m):
        A = dtype(A + wi)
        M1 = dtype(M1 + wi * mi)
        M2 = dtype(M2 + (wi * mi) * mi)
    return dtype(A * M2 - M1 * M1)


def welford_form(w, m, dtype=np.float32, shift=True):
    """(A, mu, S) of one pixel by the kernels' weighted Welford update in `dtype`, in list order; D = A S.  shift=False: the
    update on m itself instead of on m - c, c the first weighted entry's m -- not what the kernels do either: its running mean
    is rounded to an ulp of m, which on a thin distribution is a visible fraction of every deviation."""
    dtype = np.dtype(dtype).type
    w, m = np.asarray(w, dtype), np.asarray(m, dtype)
    A = mu = S = c = dtype(0.0)
    for wi, mi in zip(w, m):
        if not wi > 0:
            continue
        if shift and A == 0:
            c = mi
        e = dtype(mi - c)
        An = dtype(A + wi)
        d = dtype(e - mu)
        mun = dtype(mu + dtype(wi / An) * d)
        S = dtype(S + dtype(wi * d) * dtype(e - mun))
        A, mu = An, mun
    return A, dtype(c + mu), S


def loss_and_cotangent(D, weight, mask=None, dtype=np.float64):
    """(L, dL/dD) of gs_distortion_loss: L = weight (1 / (H W)) sum_p v_p D_p, v = mask / 255 of an optional uint8 mask."""
    dtype = np.dtype(dtype).type
    D = np.asarray(D, dtype)
    v = np.ones(D.shape, dtype) if mask is None else np.asarray(mask).astype(dtype).reshape(D.shape) / dtype(255.0)
    n = dtype(D.size)
    return dtype(weight) * (v * D).sum(dtype=dtype) / n, dtype(weight) * v / n
