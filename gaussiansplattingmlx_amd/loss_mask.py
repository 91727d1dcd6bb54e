"""Per-pixel loss masks restated in numpy (include/gsplat.h gs_set_loss_mask).

A mask is a uint8 image [H, W]: pixel weight w = v / 255 in float32, one correctly rounded division, so 255 is exactly
1.0 (keep), 0 exactly 0.0 (ignore) and the values between are soft weights (an anti-aliased matte edge).  A bool mask means
0 / 255.  White means keep: nothing is inverted or thresholded.  With a mask bound the colour loss is the plain loss of
the weighted images w R and w G; both sums and the divisor still run over all pixels (no re-normalisation by sum w, as in
gsplat and Inria's 3DGS), and the cotangent is w * dL/d(w R).  tests/loss_mask_numpy.py builds the mirror of the loss from
these weights and the oracle's loss.
"""
from __future__ import annotations

import numpy as np

_DTYPES = ("uint8", "bool", "torch.uint8", "torch.bool")


def validate(mask, H: int, W: int, who: str = "loss mask"):
    """Raises ValueError unless mask (a numpy array or a torch tensor) is uint8 or bool of shape (H, W)."""
    dtype, shape = getattr(mask, "dtype", None), getattr(mask, "shape", None)
    if dtype is None or shape is None or str(dtype) not in _DTYPES:
        raise ValueError(f"{who}: a uint8 or bool image, not {dtype if dtype is not None else type(mask).__name__}")
    if tuple(shape) != (int(H), int(W)):
        raise ValueError(f"{who}: shape (H, W) = ({int(H)}, {int(W)}), not {tuple(shape)}")


def as_uint8(mask) -> np.ndarray:
    """The uint8 form of a host mask: a bool mask becomes 0 / 255, a uint8 mask is itself."""
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        return m.astype(np.uint8) * np.uint8(255)
    if m.dtype != np.uint8:
        raise ValueError(f"loss mask: a uint8 or bool image, not {m.dtype}")
    return m


def weights(mask) -> np.ndarray:
    """float32 pixel weights of a uint8 or bool mask: (float)v / 255.0f."""
    m = as_uint8(mask)
    if m.ndim != 2:
        raise ValueError(f"loss mask: an (H, W) image, not shape {m.shape}")
    return m.astype(np.float32) / np.float32(255.0)
