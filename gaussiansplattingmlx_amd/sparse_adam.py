"""Sparse Adam: the step updates only the Gaussians its view saw (include/gsplat.h gs_set_sparse_adam, DESIGN.md section 17;
Taming 3DGS, Mallick et al. 2024 -- Inria's --optimizer_type sparse_adam, gsplat's visible_adam / SelectiveAdam).

The rule in numpy float32, as the tests state dense Adam: the project's Adam (beta = (0.9, 0.999), eps = 1e-15, (1 - beta) formed
in float32, no bias correction) on the elements of the visible rows, every other element returned as it came.  And the map from
an arena element to its Gaussian for a GaussModel layout, packed or capacity-strided: what gs_adam_step_visible computes per
element on the device.
"""
from __future__ import annotations

import numpy as np


def element_rows(seg_end, seg_row_floats, n=None) -> np.ndarray:
    """Row of every arena element: element e of segment s (elements seg_end[s-1] .. seg_end[s] - 1, the first segment from 0)
    belongs to row (e - start_s) // seg_row_floats[s].  The pads behind a segment's rows get the row numbers that follow the
    last row that fits, so `row < N` tells an element of a Gaussian from a pad or from the tail of a capacity-strided segment."""
    seg_end = [int(x) for x in seg_end]
    widths = [int(x) for x in seg_row_floats]
    if len(seg_end) != len(widths) or any(w < 1 for w in widths):
        raise ValueError("element_rows: one row width >= 1 per segment")
    n = seg_end[-1] if n is None else int(n)
    if n != seg_end[-1] or any(b < a for a, b in zip([0] + seg_end[:-1], seg_end)):
        raise ValueError("element_rows: ascending segment ends that cover the arena")
    rows = np.empty(n, np.int64)
    start = 0
    for end, w in zip(seg_end, widths):
        rows[start:end] = np.arange(end - start, dtype=np.int64) // w
        start = end
    return rows


def model_row_floats(model) -> list:
    """seg_row_floats of a GaussModel: the floats per Gaussian of its six tensors, in arena order (1 for a tensor without
    elements -- features_rest at K = 1 --, whose segment is empty whatever its width)."""
    from .trainer import ARENA_ORDER
    return [max(int(model._per[k]), 1) for k in ARENA_ORDER]


def model_element_rows(model) -> np.ndarray:
    """element_rows of a GaussModel's current layout (packed: stride == N; strided: stride >= N rows per segment)."""
    return element_rows(model.seg_end, model_row_floats(model), model.numel)


def element_mask(visible, seg_end, seg_row_floats, N=None) -> np.ndarray:
    """Which arena elements a sparse step moves: those of rows < N whose mask entry is non-zero."""
    visible = np.asarray(visible).astype(bool).reshape(-1)
    N = visible.shape[0] if N is None else int(N)
    rows = element_rows(seg_end, seg_row_floats)
    on = rows < N
    on[on] = visible[rows[on]]
    return on


def adam_dense(p, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-15, grad_scale=1.0):
    """One step of the project's Adam in float32 (lr: a scalar or one rate per element): returns (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    lr = np.asarray(lr, np.float32)
    one = np.float32(1)
    b1, b2 = np.float32(beta1), np.float32(beta2)
    gs = g * np.float32(grad_scale)
    m2 = b1 * m + (one - b1) * gs
    v2 = b2 * v + (one - b2) * gs * gs
    p2 = p - lr * m2 / (np.sqrt(v2) + np.float32(eps))
    return p2.astype(np.float32), m2.astype(np.float32), v2.astype(np.float32)


def adam_visible(p, g, m, v, lr, on, beta1=0.9, beta2=0.999, eps=1e-15, grad_scale=1.0):
    """The sparse rule: adam_dense on the elements where `on` (element_mask) is set; every other element of p, m and v comes
    back bit for bit."""
    p, m, v = (np.asarray(a, np.float32) for a in (p, m, v))
    on = np.asarray(on, bool)
    p2, m2, v2 = adam_dense(p, g, m, v, lr, beta1, beta2, eps, grad_scale)
    return np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)


def adam_visible_rows(p, g, m, v, lr, visible, beta1=0.9, beta2=0.999, eps=1e-15, grad_scale=1.0):
    """The rule on one [N, ...] tensor: rows whose mask entry is set take the step, the others keep every bit."""
    p = np.asarray(p, np.float32)
    vis = np.asarray(visible).astype(bool).reshape((-1,) + (1,) * (p.ndim - 1))
    return adam_visible(p, g, m, v, lr, np.broadcast_to(vis, p.shape), beta1, beta2, eps, grad_scale)
