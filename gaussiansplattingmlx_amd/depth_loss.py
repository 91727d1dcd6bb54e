"""Depth-supervised training (include/gsplat.h gs_depth_loss; the reference's depth term,
GaussianTrainer.swift:689-714 and :949, Inria's depth regularisation, gsplat's depth_loss).

A depth prior fixes what colour cannot: floaters and wrong surfaces on textureless regions.  With D the render's accumulated
depth sum T alpha z, a its alpha and t = scale * target + offset, the step adds weight * Ld to the loss,

    Ld = sum_valid |x - t| / max(#valid, 1e-6)

    mode            x        a pixel is valid iff its mask is set and      the target is
    "accumulated"   D        --                                            a metric depth (the reference's term: right where
                                                                           the render is opaque)
    "expected"      D / a    a >= alpha_min (and a > 0)                    a metric depth
    "disparity"     a / D    a >= alpha_min (and a > 0), D > 0             an inverse depth (gsplat's depth_loss; Inria's
                                                                           prior with its depth_params.json scale / offset)

and hands the blend backward the cotangents of D and a.  This module holds the trainer's settings; tests/depth_loss_numpy.py
restates the kernel in numpy.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

MODES = ("accumulated", "expected", "disparity")      # GS_DEPTH_ACCUMULATED, GS_DEPTH_EXPECTED, GS_DEPTH_DISPARITY


@dataclass
class DepthConfig:
    """mode: one of MODES.  weight: the depth term's weight, a float, or (init, final) decayed log-linearly over the trainer's
    iterationCount as exposureLearningRate decays its rate (Inria's pair is (1.0, 0.01)).  alpha_min: in the expected and
    disparity modes a pixel whose render alpha is below it takes no part.

    Nobody has tuned alpha_min = 0.05 or any weight here: the defaults are starting points, not recommendations."""
    mode: str = "accumulated"
    weight: object = 1.0
    alpha_min: float = 0.05

    def _pair(self):
        """The weight as a float, or as a tuple (init, final)."""
        w, bad = self.weight, ValueError("DepthConfig: weight is a float or (init, final)")
        number = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
        if isinstance(w, (tuple, list)):
            if len(w) != 2 or not all(number(x) for x in w):
                raise bad
            if not all(math.isfinite(x) and x > 0.0 for x in w):
                raise ValueError("DepthConfig: a decayed weight (init, final) is positive and finite at both ends")
            return (float(w[0]), float(w[1]))
        if not number(w):
            raise bad
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError("DepthConfig: weight is finite and >= 0")
        return float(w)

    def validate(self):
        if self.mode not in MODES:
            raise ValueError(f"DepthConfig: unknown mode {self.mode!r} (one of {', '.join(MODES)})")
        self._pair()
        try:
            a = float(self.alpha_min)
        except (TypeError, ValueError):
            a = float("nan")
        if isinstance(self.alpha_min, bool) or not (math.isfinite(a) and 0.0 <= a <= 1.0):
            raise ValueError("DepthConfig: alpha_min lies in [0, 1]")
        return self

    def weight_at(self, t: int, total: int) -> float:
        """The weight of step t of total: the constant, or log-linear from init to final, held at final from `total` on."""
        w = self._pair()
        if not isinstance(w, tuple):
            return w
        s = min(float(t) / float(total), 1.0) if total > 0 else 1.0
        return math.exp((1.0 - s) * math.log(w[0]) + s * math.log(w[1]))

    @property
    def mode_id(self) -> int:
        return MODES.index(self.mode)
