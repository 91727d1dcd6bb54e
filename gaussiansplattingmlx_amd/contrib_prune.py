"""Contribution-based pruning: per-Gaussian blend weight scores (include/gsplat.h gs_blend_contrib).

For a view, a pixel p and the j-th entry g of its tile's depth-ordered list the blend computes, T = 1 in front of the list,

    raw = exp(-1/2 d^T conic d) opacity_g,   alpha = min(raw, 0.99),   w(p, g) = T alpha,   T <- T (1 - alpha),

and the pixel stops after the entry that brings T below 1e-4 (later entries: w = 0).  The scores of a Gaussian are

    max_w[g] = max over the pixels of all views of w(p, g)     RadSplat (Niemeyer et al. 2024): prune below 0.01
    sum_w[g] = sum over the pixels of all views of w(p, g)     LightGaussian / Mini-Splatting: importance for compaction

and a Gaussian whose score lies below the threshold is pruned (action 3, count 0 of gs_classify_gaussians; else 0 and 1).
blend_weights / contrib_actions are the host-side statements of what csrc/contrib.hip computes in float32, for tests and
tools; GaussianTrainer(contrib_prune=ContribPruneConfig(...)) runs the prune during training.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

ALPHA_MAX = 0.99            # the blend's clamp
T_STOP = 1e-4               # a pixel stops after the entry that brings its transmittance below this


@dataclass
class ContribPruneConfig:
    threshold: float = 0.01             # a Gaussian whose score is below it is pruned
    at: tuple = (16000, 24000)          # the iterations behind which the event runs (RadSplat's, of 30 000)
    cameras: list | None = None         # the training cameras the score is taken over
    score: str = "max"                  # "max" (RadSplat) or "sum" (LightGaussian / Mini-Splatting)

    def validate(self) -> "ContribPruneConfig":
        """Raises ValueError for a setting the event does not take; returns self."""
        if self.score not in ("max", "sum"):
            raise ValueError(f"ContribPruneConfig.score must be \"max\" or \"sum\", got {self.score!r}")
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, (int, float, np.floating, np.integer)) or not math.isfinite(t) or t <= 0:
            raise ValueError(f"ContribPruneConfig.threshold must be a finite number > 0, got {t!r}")
        if self.score == "max" and t > 1:
            raise ValueError(f"ContribPruneConfig.threshold must be in (0, 1] for score=\"max\" (a weight never exceeds 1), got {t!r}")
        try:
            at = tuple(self.at)
        except TypeError:
            raise ValueError(f"ContribPruneConfig.at must be a sequence of iterations, got {self.at!r}") from None
        for v in at:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"ContribPruneConfig.at must hold positive integers, got {v!r}")
        if any(b <= a for a, b in zip(at, at[1:])):
            raise ValueError(f"ContribPruneConfig.at must be strictly increasing, got {self.at!r}")
        try:
            n = len(self.cameras) if self.cameras is not None else 0
        except TypeError:
            n = 0
        if n < 1:
            raise ValueError("ContribPruneConfig.cameras must be a non-empty list (the training cameras)")
        return self

    def is_event(self, t: int) -> bool:
        """Does the event run behind step t?"""
        return int(t) in tuple(self.at)


def blend_weights(packed, sortedIdx, tileRanges, W, H, tileW, tileH, dtype=np.float64, per_pixel: bool = False):
    """(max_w [N], sum_w [N]) of one view from its packed records [N, 11] (means2d, conic, colour, opacity, depth) and tile
    lists (sortedIdx [M], tileRanges [T, 2]), in `dtype`.  per_pixel=True: also the [H, W] image of sum over g of w(p, g)."""
    P = np.asarray(packed, dtype).reshape(-1, 11)
    idx = np.asarray(sortedIdx).astype(np.int64).reshape(-1)
    ranges = np.asarray(tileRanges).astype(np.int64).reshape(-1, 2)
    N = P.shape[0]
    max_w, sum_w = np.zeros(N, dtype), np.zeros(N, dtype)
    image = np.zeros((H, W), dtype)
    gridW = (W + tileW - 1) // tileW
    half, one, amax, stop = dtype(0.5), dtype(1.0), dtype(ALPHA_MAX), dtype(T_STOP)
    for tile in range(ranges.shape[0]):
        s, e = ranges[tile]
        if e <= s:
            continue
        ty, tx = divmod(tile, gridW)
        ys, xs = np.arange(ty * tileH, min(H, (ty + 1) * tileH)), np.arange(tx * tileW, min(W, (tx + 1) * tileW))
        if ys.size == 0 or xs.size == 0:
            continue
        py, px = (a.astype(dtype) for a in np.meshgrid(ys, xs, indexing="ij"))
        T = np.ones(py.shape, dtype)
        live = np.ones(py.shape, bool)
        acc = np.zeros(py.shape, dtype)
        for g in idx[s:e]:
            if not live.any():
                break
            r = P[g]
            dx, dy = px - r[0], py - r[1]
            dxdy = dx * dy
            q = -half * (dx * dx * r[2] + dy * dy * r[5] + dxdy * r[3] + dxdy * r[4])
            alpha = np.minimum(np.exp(q) * r[9], amax)
            w = np.where(live, T * alpha, dtype(0.0))
            T = np.where(live, T * (one - alpha), T)
            live &= ~(T < stop)
            acc += w
            m = w.max()
            if m > max_w[g]:
                max_w[g] = m
            sum_w[g] += w.sum()
        image[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = acc
    return (max_w, sum_w, image) if per_pixel else (max_w, sum_w)


def contrib_actions(score, threshold):
    """(actions [N] int32, counts [N] int32): prune (3, 0) where score < threshold, else keep (0, 1)."""
    prune = np.asarray(score) < threshold
    return np.where(prune, 3, 0).astype(np.int32), np.where(prune, 0, 1).astype(np.int32)
