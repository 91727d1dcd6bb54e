"""Adaptive density control: the densification of the original 3DGS (include/gsplat.h gs_set_adc_stats, DESIGN.md section 26;
Kerbl et al. 2023 -- Inria's densify_and_prune and reset_opacity --, gsplat's DefaultStrategy).

The rule every 3DGS paper and data set is tuned for, beside the reference's (strategy="reference") and the MCMC strategy:

  statistic   every step, for each Gaussian the view saw (radius > 0): gradSum += hypot(W/2 gx, H/2 gy) of the gradient of
              its 2-D mean (the absolute sums under absgrad), count += 1, maxRadius = max(maxRadius, radius);
  event       every densify_interval steps in [densify_from, densify_until], per Gaussian, the first that holds:
                sigmoid(opacity) < min_opacity                                                      prune
                N < maxGaussians and gradSum / count >= grad_threshold     clone if max exp(scale) <= percent_dense x extent,
                                                                           split otherwise
                after the first reset: maxRadius > max_screen_size or max exp(scale) > prune_world x extent     prune
              a split replaces the Gaussian by two children at xyz + R(q) (exp(scale) * z), z ~ N(0, I) per child, their scales
              divided by 1.6; a clone adds an exact copy.  The Adam moments of kept Gaussians and of a clone's original survive
              the event, children and copies start at zero; the three accumulators are zeroed.
  reset       every opacity_reset_interval steps (up to densify_until): opacity = min(opacity, reset_value), the opacity
              segment's moments zeroed -- what removes floaters.

GaussianTrainer(strategy="adc", adc=ADCConfig(scene_extent=scene_extent(cameras))) trains with it; csrc/adc.hip holds the
kernels, tests/adc_numpy.py restates them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float, np.floating, np.integer)) and math.isfinite(x)


def _integer(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


@dataclass
class ADCConfig:
    # Inria's and gsplat's defaults (densify_grad_threshold, percent_dense, the 0.005 of densify_and_prune, size_threshold 20,
    # the 0.1 x extent of prune_big_points); nobody has tuned them here
    grad_threshold: float = 0.0002
    percent_dense: float = 0.01
    min_opacity: float = 0.005
    max_screen_size: float = 20.0       # pixels; <= 0: no screen-size test (gsplat's default)
    prune_world: float = 0.1
    scene_extent: float = None          # scene_extent(cameras): required
    densify_from: int = 500
    densify_until: int = 15000
    densify_interval: int = 100
    opacity_reset_interval: int = 3000
    reset_value: float = 0.01
    revised_opacity: bool = False

    def validate(self) -> "ADCConfig":
        """Raises ValueError for a setting the trainer does not take; returns self."""
        for name in ("grad_threshold", "percent_dense", "prune_world", "scene_extent"):
            v = getattr(self, name)
            if not _number(v) or v <= 0:
                hint = " (adc.scene_extent(cameras))" if name == "scene_extent" else ""
                raise ValueError(f"ADCConfig.{name} must be a finite number > 0, got {v!r}{hint}")
        for name in ("min_opacity", "reset_value"):
            v = getattr(self, name)
            if not _number(v) or not 0 < v < 1:
                raise ValueError(f"ADCConfig.{name} must lie in (0, 1), got {v!r}")
        if not _number(self.max_screen_size):
            raise ValueError(f"ADCConfig.max_screen_size must be a finite number (<= 0: no screen test), got {self.max_screen_size!r}")
        for name, low in (("densify_from", 0), ("densify_until", 0), ("densify_interval", 1), ("opacity_reset_interval", 1)):
            v = getattr(self, name)
            if not _integer(v) or v < low:
                raise ValueError(f"ADCConfig.{name} must be an integer >= {low}, got {v!r}")
        if self.densify_until < self.densify_from:
            raise ValueError(f"ADCConfig.densify_until = {self.densify_until} is below densify_from = {self.densify_from}")
        if not isinstance(self.revised_opacity, (bool, np.bool_)):
            raise ValueError("ADCConfig.revised_opacity is True or False")
        return self

    def is_event(self, it: int) -> bool:
        """Does a densify event run behind step `it`?"""
        return self.densify_from <= it <= self.densify_until and it % self.densify_interval == 0

    def is_reset(self, it: int) -> bool:
        """Does an opacity reset run behind step `it`?  (Not behind step 0: nothing has been learnt that a reset could undo.)"""
        return 0 < it <= self.densify_until and it % self.opacity_reset_interval == 0


def scene_extent(cameras) -> float:
    """Inria's cameras_extent: 1.1 x the largest distance of a camera centre from the centres' mean.  cameras: objects with a
    cameraCenter, or centres [n, 3]."""
    cams = list(cameras) if not isinstance(cameras, np.ndarray) else cameras
    if len(cams) < 1:
        raise ValueError("scene_extent: no cameras")
    c = np.stack([np.asarray(getattr(cam, "cameraCenter", cam), np.float64).reshape(-1) for cam in cams])
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("scene_extent: camera centres have three components")
    if not np.isfinite(c).all():
        raise ValueError("scene_extent: a camera centre is not finite")
    extent = 1.1 * float(np.linalg.norm(c - c.mean(axis=0), axis=1).max())
    if not extent > 0:
        raise ValueError("scene_extent: the cameras' centres coincide (the extent would be 0)")
    return extent
