"""The masked loss restated in numpy (include/gsplat.h gs_set_loss_mask), composed with the oracle's loss.

The weight of mask value v is w = v / 255 (gaussiansplattingmlx_amd.loss_mask.weights).  The loss under a mask is the oracle's
loss_forward_backward of the weighted images w R and w G at the oracle's precision -- both sums still divided by all 3 H W
elements -- and its cotangent with respect to R is w times that call's cotangent (the chain rule through R -> w R)."""
import numpy as np

from gaussiansplattingmlx_amd.loss_mask import weights


def masked_loss(oracle, render, target, mask, lambda_dssim=0.2):
    """(loss, cot, l1, ssim) of `render` against `target` under `mask` (uint8 or bool [H, W]), at the oracle's precision."""
    w = weights(mask).astype(oracle.dtype)[..., None]          # (v / 255 in float32 is exact to widen)
    rw = np.asarray(render, oracle.dtype) * w
    gw = np.asarray(target, oracle.dtype) * w
    loss, cot, _, l1, ssim = oracle.loss_forward_backward(rw, gw, lambda_dssim)
    return loss, cot * w, l1, ssim
