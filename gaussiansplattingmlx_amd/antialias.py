"""The anti-aliased mode's opacity compensation in float64 (include/gsplat.h gs_set_antialiasing).

    rho = sqrt(det Sigma / det Sigma_b),  Sigma = Sigma_b - 0.3 I

Sigma_b is the blurred 2-D covariance the projection returns (the reference's + 0.3 on the diagonal); the fused kernels blend
sigma(o) rho instead of sigma(o).  A splat whose det Sigma is not > 0 (or not finite) gets rho = 0: invisible, zero gradient.
These are the host-side statements of what csrc/gs_math.h aa_opacity_scale computes in float32, for tests and tools that
compose the mode from the reference's ops.
"""
from __future__ import annotations

import numpy as np

BLUR = 0.3


def _unblurred(cov2d):
    c = np.asarray(cov2d, np.float64).reshape(-1, 2, 2)
    return c - BLUR * np.eye(2)[None], c


def _det(a):
    return a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]


def opacity_scale(cov2d):
    """rho per splat from the blurred covariances cov2d [..., 2, 2] (four independent entries); 0 where det Sigma is not
    > 0 or not finite."""
    u, b = _unblurred(cov2d)
    du, db = _det(u), _det(b)
    ok = (du > 0) & np.isfinite(du) & (db > 0) & np.isfinite(db)
    rho = np.zeros(du.shape, np.float64)
    rho[ok] = np.sqrt(du[ok] / db[ok])
    return rho.reshape(np.shape(cov2d)[:-2])


def opacity_scale_vjp(cov2d, cot):
    """The cotangent of Sigma_b, [..., 2, 2] in the four-independent-entries convention, for cotangent `cot` of rho:
    cot (rho / 2) (Sigma^-T - Sigma_b^-T); 0 where rho is."""
    u, b = _unblurred(cov2d)
    rho = opacity_scale(cov2d).reshape(-1)
    cot = np.broadcast_to(np.asarray(cot, np.float64).reshape(-1), rho.shape)
    out = np.zeros(u.shape, np.float64)
    ok = rho > 0
    if ok.any():
        iu = np.linalg.inv(u[ok]).transpose(0, 2, 1)
        ib = np.linalg.inv(b[ok]).transpose(0, 2, 1)
        out[ok] = (cot[ok] * rho[ok] * 0.5)[:, None, None] * (iu - ib)
    return out.reshape(np.shape(cov2d))
