"""Training on RGBA views over a background colour (include/gsplat.h gs_set_background / gs_composite_target, DESIGN.md
section 18; Inria's --random_background, gsplat's backgrounds= / random_bkgd).

On a fixed black background nothing tells an empty pixel from a black surface, on a white one nothing tells it from a white
surface, and a semi-transparent floater of the background's colour costs no loss.  With a colour that changes every step only a
truly empty pixel matches its target every time.  This module holds the trainer's settings, the step's colour as a pure function
of (seed, iteration), and the statements in numpy that the tests hold the kernels to:

    target      composite(rgb, a, b)              = a rgb + (1 - a) b
    forward     with_background(colour_black, alpha, b) = colour_black + (1 - alpha) b
    backward    the gradient for cotangents (g, cD, cA) under b is the black backward's for (g, cD, shifted_cot_alpha(g, cA, b)),
                shifted_cot_alpha = cA - g . b:  the colour enters only through T = 1 - alpha, d colour_c / dT = b_c.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np


@dataclass
class BackgroundConfig:
    """mode "random": step t composites over background_for(seed, t); mode "fixed": every step over `color` (three finite
    floats).  `color` is needed when mode is "fixed" and refused otherwise."""
    mode: str = "random"
    seed: int = 0
    color: object = None

    def validate(self):
        if self.mode not in ("random", "fixed"):
            raise ValueError(f"BackgroundConfig: unknown mode {self.mode!r} (\"random\" or \"fixed\")")
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or int(self.seed) < 0:
            raise ValueError("BackgroundConfig: seed is an integer >= 0")
        if self.mode == "random":
            if self.color is not None:
                raise ValueError("BackgroundConfig: color belongs to mode=\"fixed\" (a random background takes its colours from seed)")
            return self
        if self.color is None:
            raise ValueError("BackgroundConfig: mode=\"fixed\" needs color = (r, g, b)")
        try:
            c = [float(x) for x in self.color]
        except (TypeError, ValueError):
            c = []
        if len(c) != 3 or not all(math.isfinite(x) for x in c):
            raise ValueError("BackgroundConfig: color is three finite floats")
        return self

    def color_at(self, iteration: int) -> np.ndarray:
        """The step's colour, float32 [3]."""
        if self.mode == "fixed":
            return np.asarray([float(x) for x in self.color], np.float32)
        return background_for(self.seed, iteration)


def background_for(seed: int, iteration: int) -> np.ndarray:
    """The random background of step `iteration`: float32 [3] in [0, 1), np.random.default_rng([seed, iteration]).  A pure
    function of its two arguments: a reload or a restart sees the same colours, in whatever order they are asked for."""
    seed, iteration = int(seed), int(iteration)
    if seed < 0 or iteration < 0:
        raise ValueError("background_for: seed and iteration are >= 0")
    return np.random.default_rng([seed, iteration]).random(3, dtype=np.float32)


def composite(rgb, alpha, bg):
    """a rgb + (1 - a) b per pixel: rgb [..., 3] straight (un-premultiplied), alpha [...], in float64."""
    rgb, alpha, bg = np.asarray(rgb, np.float64), np.asarray(alpha, np.float64), np.asarray(bg, np.float64).reshape(3)
    return alpha[..., None] * rgb + (1.0 - alpha[..., None]) * bg


def with_background(color_black, alpha, bg):
    """A render over bg from the render over black and its alpha: colour_black + (1 - alpha) b, in the inputs' float type
    (float64 unless both are float32)."""
    color_black, alpha = np.asarray(color_black), np.asarray(alpha)
    dt = np.float32 if color_black.dtype == np.float32 and alpha.dtype == np.float32 else np.float64
    bg = np.asarray(bg, dt).reshape(3)
    return color_black.astype(dt) + (dt(1) - alpha.astype(dt))[..., None] * bg


def shifted_cot_alpha(cotColor, cotAlpha, bg):
    """cA - g . b per pixel: the alpha cotangent under which the BLACK backward returns the gradient under b (the channels are
    added in order, in the inputs' float type: with b = (1, 1, 1) this is the white backward's own -cA + (gx + gy + gz))."""
    cotColor, cotAlpha = np.asarray(cotColor), np.asarray(cotAlpha)
    dt = np.float32 if cotColor.dtype == np.float32 and cotAlpha.dtype == np.float32 else np.float64
    g, bg = cotColor.astype(dt).reshape(-1, 3), np.asarray(bg, dt).reshape(3)
    dot = (g[:, 0] * bg[0] + g[:, 1] * bg[1]) + g[:, 2] * bg[2]
    return (cotAlpha.astype(dt).reshape(-1) - dot).reshape(cotAlpha.shape)
