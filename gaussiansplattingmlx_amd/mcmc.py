"""The MCMC densification strategy's settings (include/gsplat.h gs_set_mcmc).

"3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024), gsplat's MCMCStrategy: dead Gaussians are
relocated onto live ones, the count grows by at most grow_rate per event up to cap_max, every step adds position noise and
two regularisers.  The defaults are gsplat's.  GaussianTrainer(strategy="mcmc", mcmc=MCMCConfig(...)) runs it.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np


@dataclass
class MCMCConfig:
    cap_max: int = 1_000_000        # the budget: N never exceeds it
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    min_opacity: float = 0.005      # a Gaussian with sigmoid(opacity) <= min_opacity (or not finite) is dead
    refine_start: int = 500         # events at refine_start < t < refine_stop, t % refine_every == 0
    refine_stop: int = 25_000
    refine_every: int = 100
    grow_rate: float = 0.05
    n_max: int = 51                 # the relocation formula's largest n
    seed: int | None = None         # None: the trainer's noise_seed

    def validate(self) -> "MCMCConfig":
        """Raises ValueError for a setting the kernels do not take; returns self."""
        def finite_nonneg(name):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"MCMCConfig.{name} must be a finite number >= 0, got {v!r}")
        for name in ("noise_lr", "opacity_reg", "scale_reg"):
            finite_nonneg(name)
        if not (isinstance(self.min_opacity, (int, float)) and 0.0 < self.min_opacity < 1.0):
            raise ValueError(f"MCMCConfig.min_opacity must be in (0, 1), got {self.min_opacity!r}")
        if not (isinstance(self.grow_rate, (int, float)) and 0.0 <= self.grow_rate <= 1.0):
            raise ValueError(f"MCMCConfig.grow_rate must be in [0, 1], got {self.grow_rate!r}")
        for name, lo, hi in (("cap_max", 1, 2 ** 31 - 1), ("n_max", 1, 51), ("refine_every", 1, 2 ** 31 - 1),
                             ("refine_start", 0, 2 ** 31 - 1), ("refine_stop", 0, 2 ** 31 - 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"MCMCConfig.{name} must be an integer in [{lo}, {hi}], got {v!r}")
        if self.seed is not None and (isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer))
                                      or not 0 <= self.seed < 2 ** 64):
            raise ValueError(f"MCMCConfig.seed must be None or an integer in [0, 2^64), got {self.seed!r}")
        return self

    def is_event(self, t: int) -> bool:
        """Does the event run behind step t?"""
        return self.refine_start < t < self.refine_stop and t % self.refine_every == 0

    def params(self, iteration: int, seed: int):
        """The ctypes gs_mcmc_params of step `iteration` (seed: used when self.seed is None)."""
        from ._lib import gs_mcmc_params
        p = gs_mcmc_params()
        p.noise_lr, p.opacity_reg, p.scale_reg = float(self.noise_lr), float(self.opacity_reg), float(self.scale_reg)
        p.min_opacity, p.grow_rate = float(self.min_opacity), float(self.grow_rate)
        p.cap_max, p.n_max, p.iteration = int(self.cap_max), int(self.n_max), int(iteration)
        p.seed = C.c_ulonglong(int(seed if self.seed is None else self.seed)).value
        return p


def grown_count(N: int, cap_max: int, grow_rate: float) -> int:
    """The count after a growth event: min(cap_max, floor((1 + grow_rate) N)), never below N."""
    return max(int(N), min(int(cap_max), int(math.floor((1.0 + float(grow_rate)) * int(N)))))


def relocation_formula(o, n, min_opacity: float = 0.005, n_max: int = 51):
    """The relocation's opacity and scale factor in float64 for sources of opacity o drawn n - 1 times (n clamped to n_max):
    o' = clamp(1 - (1 - o)^(1/n), min_opacity, 1 - 2^-23), and s'/s = o / sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k
    o'^(k+1) / sqrt(k+1).  What csrc/mcmc.hip mcmc_formula_kernel computes, in the same order.

    Accuracy: against the same expression at 60 decimal digits (tests/test_mcmc_cpu.py) both results are within 2.5e-10
    relative for raw opacities in [-5.2, 30] and n up to 51 (the alternating sum's cancellation; 1e-9 up to raw 36.5).
    Float64 loses it from raw >= 37 on, where o = sigmoid(raw) rounds to 1.0 and o' sits at its upper clamp: the sum's terms
    then reach C(50, 25), and s'/s is off by 1.8e-7 at n = 35 and 1.3e-3 at n = 51."""
    o = np.asarray(o, np.float64)
    n = np.minimum(np.broadcast_to(np.asarray(n, np.int64), o.shape), int(n_max))
    on = np.clip(1.0 - np.power(1.0 - o, 1.0 / n), float(min_opacity), 1.0 - 2.0 ** -23)
    den = np.zeros(o.shape, np.float64)
    for idx in np.ndindex(o.shape):
        d, x = 0.0, float(on[idx])
        for a in range(1, int(n[idx]) + 1):
            binom, pw = 1.0, x
            for k in range(a):
                term = binom * pw / math.sqrt(k + 1)
                d += -term if k & 1 else term
                binom = binom * (a - 1 - k) / (k + 1)
                pw *= x
        den[idx] = d
    return on, o / den
