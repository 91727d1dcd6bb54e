"""Exposure compensation restated in numpy (include/gsplat.h gs_set_exposure), composed with the oracle's loss.

M is [A | b] row-major 3 x 4 (12 floats).  The loss of an exposed render is the oracle's loss_forward_backward of A r + b; its
VJP is dL/dr = A^T g, dL/dA = sum_p g_p r_p^T, dL/db = sum_p g_p with g the oracle's colour cotangent.  Sums in float64."""
import numpy as np

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)


def apply(M, img, dtype=np.float64):
    """A img + b over the last axis of img, computed in float64 and rounded to `dtype`."""
    M = np.asarray(M, np.float64).reshape(3, 4)
    x = np.asarray(img, np.float64)
    return (x @ M[:, :3].T + M[:, 3]).astype(dtype)


def vjp(M, g, render):
    """(dL/dr [.., 3], dL/dM [12]) from g = dL/d(A r + b), in float64."""
    M = np.asarray(M, np.float64).reshape(3, 4)
    g64 = np.asarray(g, np.float64).reshape(-1, 3)
    r64 = np.asarray(render, np.float64).reshape(-1, 3)
    dM = np.empty((3, 4))
    dM[:, :3] = g64.T @ r64
    dM[:, 3] = g64.sum(0)
    return (g64 @ M[:, :3]).reshape(np.shape(g)), dM.reshape(12)


def composed(o, render, target, M, lam=0.2, **depth):
    """The oracle `o`'s loss of the exposed render at the oracle's precision: (loss, dL/dr, dL/dM, g)."""
    c = apply(M, render, o.dtype)
    loss, g, _, _, _ = o.loss_forward_backward(c, target, lam, **depth)
    dr, dM = vjp(M, g, render)
    return loss, dr, dM, g


def random_exposure(rng):
    """diag in [0.6, 1.4], off-diagonals in [-0.15, 0.15], biases in [-0.1, 0.1]."""
    A = rng.uniform(-0.15, 0.15, (3, 3))
    A[np.diag_indices(3)] = rng.uniform(0.6, 1.4, 3)
    return np.concatenate([A, rng.uniform(-0.1, 0.1, (3, 1))], 1).astype(np.float32).reshape(12)


def adam(p, g, m, v, lr, b1=0.9, b2=0.999, eps=1e-15):
    """The project's Adam (no bias correction) in float32, in place."""
    f = np.float32
    m[:] = f(b1) * m + (f(1) - f(b1)) * g
    v[:] = f(b2) * v + (f(1) - f(b2)) * g * g
    p[:] = p - (f(lr) * m) / (np.sqrt(v) + f(eps))
