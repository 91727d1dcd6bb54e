"""Normal regularisation from the rendered depth (include/gsplat.h gs_normal_loss; the normal terms of
DN-Splatter, MonoSDF and VCR-GauS on the normals of the depth image, the smoothness term 2DGS, GOF, PGSR and RaDe-GS train
their surfaces with).

mesh.extract_mesh fuses every camera's expected depth D / a; a mesh made that way is only as good as those depth images.  The
step takes the normals n of the expected depth image (a cross product of the back-projected neighbours, header) and adds

    l1_weight  sum_Vp |n - Nt|_1 / #Vp  +  cos_weight  sum_Vp (1 - n . Nt) / #Vp  +  smooth_weight  sum_pairs w_pq (1 - n_p . n_q) / #pairs

to the loss: Nt a normal prior in camera space (OpenCV axes, facing the camera; trainStep's targetNormal, TrainData.normalArray),
the pairs the adjacent pixels that both have a normal, w_pq = exp(-edge_gamma mean_c |I_p - I_q|) on the step's target colour.
It hands the blend backward the cotangents of D and a.  This module holds the trainer's settings; tests/normal_loss_numpy.py
restates the kernels in numpy.

Not here: normals rendered from the Gaussians' own axes and 2DGS's consistency between them and the depth
normals, median depth, fisheye cameras, data-parallel and multi-view steps.  The depth distortion loss these methods train with
beside it is distortion.py's (GaussianTrainer(distortion=DistortionConfig(...))).
"""
from __future__ import annotations

import math
from dataclasses import dataclass


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


@dataclass
class NormalConfig:
    """l1_weight, cos_weight: the weights of the two prior terms (they need trainStep's targetNormal; a step without one runs
    the smoothness term alone).  smooth_weight: the weight of the smoothness term.  Each is a float, or (init, final) decayed
    log-linearly over the trainer's iterationCount as DepthConfig.weight is.  alpha_min: a pixel whose render alpha is below
    it has no expected depth and gives its neighbours no normal.  max_jump: with a value > 0 a pixel whose neighbours' depths
    differ by more than max_jump times its own depth has no normal (depth edges); 0 keeps every pixel.  edge_gamma: the
    smoothness pairs are weighted by exp(-edge_gamma mean_c |I_p - I_q|) of the step's target colour; 0 weights every pair 1.
    start: the first iteration that runs the term; before it the step is the step without normal=.

    Nobody has tuned any default here: every weight is 0 (the term does nothing until one is set), and alpha_min = 0.05,
    max_jump = 0, edge_gamma = 0 and start = 0 are starting points, not recommendations."""
    l1_weight: object = 0.0
    cos_weight: object = 0.0
    smooth_weight: object = 0.0
    alpha_min: float = 0.05
    max_jump: float = 0.0
    edge_gamma: float = 0.0
    start: int = 0

    @staticmethod
    def _pair(w, name):
        """A weight as a float, or as a tuple (init, final)."""
        bad = ValueError(f"NormalConfig: {name} is a float or (init, final)")
        if isinstance(w, (tuple, list)):
            if len(w) != 2 or not all(_number(x) for x in w):
                raise bad
            if not all(math.isfinite(x) and x > 0.0 for x in w):
                raise ValueError(f"NormalConfig: a decayed {name} (init, final) is positive and finite at both ends")
            return (float(w[0]), float(w[1]))
        if not _number(w):
            raise bad
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"NormalConfig: {name} is finite and >= 0")
        return float(w)

    def validate(self):
        for name in ("l1_weight", "cos_weight", "smooth_weight"):
            self._pair(getattr(self, name), name)
        for name, hi in (("alpha_min", 1.0), ("max_jump", math.inf), ("edge_gamma", math.inf)):
            x = getattr(self, name)
            if not _number(x) or not (math.isfinite(x) and 0.0 <= x <= hi):
                raise ValueError(f"NormalConfig: {name} " + ("lies in [0, 1]" if hi == 1.0 else "is finite and >= 0"))
        if isinstance(self.start, bool) or not isinstance(self.start, int) or self.start < 0:
            raise ValueError("NormalConfig: start is an integer >= 0")
        return self

    def weights_at(self, t: int, total: int):
        """(l1, cos, smooth) at step t of total: each the constant, or log-linear from init to final, held at final from `total`."""
        s = min(float(t) / float(total), 1.0) if total > 0 else 1.0
        out = []
        for name in ("l1_weight", "cos_weight", "smooth_weight"):
            w = self._pair(getattr(self, name), name)
            out.append(w if not isinstance(w, tuple) else math.exp((1.0 - s) * math.log(w[0]) + s * math.log(w[1])))
        return tuple(out)

    @property
    def wants_prior(self) -> bool:
        """Does any prior term have a weight?"""
        return any(self._pair(getattr(self, n), n) != 0.0 for n in ("l1_weight", "cos_weight"))
