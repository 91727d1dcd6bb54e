"""AbsGS densification: the per-pixel absolute 2-D gradient statistic (include/gsplat.h gs_set_absgrad).

The reference densifies a Gaussian when the accumulated norm of its signed xyz gradient, over the step count, exceeds a
threshold.  A signed gradient is a sum over pixels; on a large blurry Gaussian that covers fine detail the pixels pull in
opposite directions and cancel (the "gradient collision" of AbsGS, Ye et al. 2024).  The remedy, gsplat's absgrad=True and
Mip-Splatting's code: sum the per-pixel ABSOLUTE values of the 2-D mean gradient and densify on those.  For a pixel p and the
i-th entry g of its tile's depth-ordered list, with d = p - mean, c the conic and the blend's own quantities

    raw = exp(-1/2 d^T c d) opacity,   alpha = min(raw, 0.99),   S_i = cot . sample_i (colour, and depth when given),
    T = 1, R = 0 in front of the list,   K = cot . final - cotAlpha (1 - outAlpha),
    R += T alpha S_i,   dalpha = T S_i - (K - R) / (1 - alpha),   h = dalpha raw (0 where raw > 0.99),   T *= 1 - alpha,

for the entries in front of the pixel's stop (lastContrib), the two terms of the mean's gradient are

    g_x = h (c00 dx + 1/2 (c01 + c10) dy),     g_y = h (c11 dy + 1/2 (c01 + c10) dx),

and per Gaussian   S = (sum g_x, sum g_y)  is what the backward has always produced,  A = (sum |g_x|, sum |g_y|)  is new.
(K: cot . final covers a white background, whose T_n sum(cot) is part of the final colour; the alpha cotangent's term is the
cotangent -cotAlpha of the final transmittance T_n = 1 - outAlpha, which every entry of the list scales.)  The statistic the
trainer accumulates is hypot(W/2 Ax, H/2 Ay), gsplat's and Inria's NDC scaling of the screen-space gradient.

blend_absgrad / absgrad_statistic are the host-side statements of what csrc/blend_v2.hip (ABSGRAD) and csrc/densify.hip
compute in float32, for tests and tools; GaussianTrainer(absgrad=AbsGradConfig()) trains with the criterion.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

ALPHA_MAX = 0.99            # the blend's clamp; an entry with raw above it has no gradient


@dataclass
class AbsGradConfig:
    # gsplat's documented grow_grad2d for absgrad=True.  gsplat divides the accumulated statistic by a per-Gaussian visibility
    # count; this project keeps the reference's global step count as the denominator, so the value is a starting point that
    # nobody has tuned here
    threshold: float = 0.0008

    def validate(self) -> "AbsGradConfig":
        """Raises ValueError for a setting the trainer does not take; returns self."""
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, (int, float, np.floating, np.integer)) or not math.isfinite(t) or t <= 0:
            raise ValueError(f"AbsGradConfig.threshold must be a finite number > 0, got {t!r}")
        return self


def blend_absgrad(packed, sortedIdx, tileRanges, W, H, tileW, tileH, cotColor, outColor, lastContrib, cotDepth=None,
                  outDepth=None, cotAlpha=None, outAlpha=None, dtype=np.float64):
    """(A [N, 2], S [N, 2]): the absolute and the signed sums over the pixels of (g_x, g_y) of one view, in pixel units, from
    its packed records [N, 11] (means2d, conic, colour, opacity, depth), tile lists (sortedIdx [M], tileRanges [T, 2]), the
    forward's outputs (outColor [H, W, 3], lastContrib [H, W]; outDepth / outAlpha with their cotangents) and the cotangents,
    in `dtype`.  One forward sweep per tile, vectorised over the tile's pixels."""
    if (cotDepth is None) != (outDepth is None):
        raise ValueError("blend_absgrad: cotDepth and outDepth come together")
    if (cotAlpha is None) != (outAlpha is None):
        raise ValueError("blend_absgrad: cotAlpha and outAlpha come together")
    P = np.asarray(packed, dtype).reshape(-1, 11)
    idx = np.asarray(sortedIdx).astype(np.int64).reshape(-1)
    ranges = np.asarray(tileRanges).astype(np.int64).reshape(-1, 2)
    cot = np.asarray(cotColor, dtype).reshape(H, W, 3)
    K = (cot * np.asarray(outColor, dtype).reshape(H, W, 3)).sum(axis=2)
    cotD = None
    if cotDepth is not None:
        cotD = np.asarray(cotDepth, dtype).reshape(H, W)
        K = K + cotD * np.asarray(outDepth, dtype).reshape(H, W)
    if cotAlpha is not None:
        K = K - np.asarray(cotAlpha, dtype).reshape(H, W) * (dtype(1.0) - np.asarray(outAlpha, dtype).reshape(H, W))
    last = np.asarray(lastContrib).astype(np.int64).reshape(H, W)
    N = P.shape[0]
    A, S = np.zeros((N, 2), dtype), np.zeros((N, 2), dtype)
    gridW = (W + tileW - 1) // tileW
    half, one, amax, zero = dtype(0.5), dtype(1.0), dtype(ALPHA_MAX), dtype(0.0)
    for tile in range(ranges.shape[0]):
        s, e = ranges[tile]
        if e <= s:
            continue
        ty, tx = divmod(tile, gridW)
        y0, y1, x0, x1 = ty * tileH, min(H, (ty + 1) * tileH), tx * tileW, min(W, (tx + 1) * tileW)
        if y1 <= y0 or x1 <= x0:
            continue
        py, px = (a.astype(dtype) for a in np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij"))
        c = cot[y0:y1, x0:x1]
        cd = None if cotD is None else cotD[y0:y1, x0:x1]
        n = np.minimum(last[y0:y1, x0:x1], e - s)
        Kt = K[y0:y1, x0:x1]
        T = np.ones(py.shape, dtype)
        R = np.zeros(py.shape, dtype)
        for i, g in enumerate(idx[s:s + int(n.max())]):
            r = P[g]
            dx, dy = px - r[0], py - r[1]
            dxdy = dx * dy
            q = -half * (dx * dx * r[2] + dy * dy * r[5] + dxdy * r[3] + dxdy * r[4])
            raw = np.exp(q) * r[9]
            live = i < n
            alpha = np.where(live, np.minimum(raw, amax), zero)
            Si = c[..., 0] * r[6] + c[..., 1] * r[7] + c[..., 2] * r[8]
            if cd is not None:
                Si = Si + cd * r[10]
            R = R + T * alpha * Si
            dalpha = T * Si - (Kt - R) / (one - alpha)
            h = np.where(live & ~(raw > amax), dalpha * raw, zero)
            T = T * (one - alpha)
            cs = half * (r[3] + r[4])
            gx, gy = h * (r[2] * dx + cs * dy), h * (r[5] * dy + cs * dx)
            A[g, 0] += np.abs(gx).sum()
            A[g, 1] += np.abs(gy).sum()
            S[g, 0] += gx.sum()
            S[g, 1] += gy.sum()
    return A, S


def absgrad_statistic(A, W, H):
    """What one step adds to the densification accumulator: hypot(W/2 Ax, H/2 Ay) [N] of A [N, 2]."""
    A = np.asarray(A)
    return np.hypot(0.5 * W * A[..., 0], 0.5 * H * A[..., 1])
