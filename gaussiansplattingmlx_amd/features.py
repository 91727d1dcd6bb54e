"""N-channel per-Gaussian feature rendering (include/gsplat.h gs_blend_features / gs_render_features).

Any per-Gaussian vector f[g, 0..C) -- semantic or language features (Feature-3DGS, LangSplat, LEGaussians), segmentation
identities, normals, albedo -- is blended over the same splats as the colours, with the blend weights of contrib_prune.py,

    out[p, c]    = sum over the entries g of p's list of  w(p, g) f[g, c]          w(p, g) = T alpha,  T <- T (1 - alpha),
    grad_f[g, c] = sum over the pixels p of               w(p, g) cot[p, c]        a pixel stops after the entry with T < 1e-4,

without a background term.  The geometry is frozen: a field is distilled into a trained scene, there is no gradient into
opacity, conic or mean.  tile_weights / blend_features / blend_features_vjp are the host-side statements of what
csrc/features.hip computes in float32, for tests and tools; FeatureField holds a field on the device and trains it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .contrib_prune import ALPHA_MAX, T_STOP

CHANNEL_GROUP = 16          # channels per sweep of the lists (csrc/features.hip GS_FEATURE_GROUP, gs_feature_channel_group())
MAX_CHANNELS = 256          # GS_MAX_FEATURE_CHANNELS
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-15      # the trainer's Adam (gs_adam_step): no bias correction


def tile_weights(packed, sortedIdx, tileRanges, W, H, tileW, tileH, dtype=np.float64):
    """The blend weights of one view, tile by tile: a list of (ys, xs, g, w) with the tile's pixel rows and columns, the
    Gaussian indices g [n] of the entries up to the one behind which every pixel has stopped, and w [n, len(ys), len(xs)] in
    `dtype`.  contrib_prune.blend_weights' arithmetic in its order; computed once, it serves any number of blend_features /
    blend_features_vjp calls on the same (frozen) geometry."""
    P = np.asarray(packed, dtype).reshape(-1, 11)
    idx = np.asarray(sortedIdx).astype(np.int64).reshape(-1)
    ranges = np.asarray(tileRanges).astype(np.int64).reshape(-1, 2)
    gridW = (W + tileW - 1) // tileW
    half, one, amax, stop = dtype(0.5), dtype(1.0), dtype(ALPHA_MAX), dtype(T_STOP)
    tiles = []
    for tile in range(ranges.shape[0]):
        s, e = ranges[tile]
        if e <= s:
            continue
        ty, tx = divmod(tile, gridW)
        ys, xs = np.arange(ty * tileH, min(H, (ty + 1) * tileH)), np.arange(tx * tileW, min(W, (tx + 1) * tileW))
        if ys.size == 0 or xs.size == 0:
            continue
        py, px = (a.astype(dtype) for a in np.meshgrid(ys, xs, indexing="ij"))
        T = np.ones(py.shape, dtype)
        live = np.ones(py.shape, bool)
        ws = []
        for g in idx[s:e]:
            if not live.any():
                break
            r = P[g]
            dx, dy = px - r[0], py - r[1]
            dxdy = dx * dy
            q = -half * (dx * dx * r[2] + dy * dy * r[5] + dxdy * r[3] + dxdy * r[4])
            alpha = np.minimum(np.exp(q) * r[9], amax)
            ws.append(np.where(live, T * alpha, dtype(0.0)))
            T = np.where(live, T * (one - alpha), T)
            live &= ~(T < stop)
        tiles.append((ys, xs, idx[s:s + len(ws)], np.stack(ws)))
    return tiles


def blend_features(packed, sortedIdx, tileRanges, W, H, tileW, tileH, features, dtype=np.float64, weights=None):
    """The feature image [H, W, C] of one view from its packed records [N, 11], tile lists and features [N, C], in `dtype`;
    a pixel's sum runs in list order.  weights: tile_weights(...) of the same view, if they are at hand."""
    f = np.asarray(features, dtype)
    f = f.reshape(f.shape[0], -1)
    if weights is None:
        weights = tile_weights(packed, sortedIdx, tileRanges, W, H, tileW, tileH, dtype)
    out = np.zeros((H, W, f.shape[1]), dtype)
    for ys, xs, g, w in weights:
        acc = np.zeros((ys.size, xs.size, f.shape[1]), dtype)
        for j in range(g.size):
            acc += w[j][:, :, None] * f[g[j]]
        out[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = acc
    return out


def blend_features_vjp(packed, sortedIdx, tileRanges, W, H, tileW, tileH, cot, dtype=np.float64, weights=None, N=None):
    """The gradient [N, C] of blend_features with respect to the features for the cotangent image cot [H, W, C].  N: the
    number of Gaussians (default: the rows of packed).  Rows of Gaussians that weigh on no pixel are exactly 0."""
    ct = np.asarray(cot, dtype).reshape(H, W, -1)
    if N is None:
        N = np.asarray(packed).reshape(-1, 11).shape[0]
    if weights is None:
        weights = tile_weights(packed, sortedIdx, tileRanges, W, H, tileW, tileH, dtype)
    grad = np.zeros((N, ct.shape[2]), dtype)
    for ys, xs, g, w in weights:
        c = ct[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        rows = np.einsum("jyx,yxc->jc", w, c)
        touched = w.reshape(g.size, -1).any(axis=1)          # (an entry of weight 0 everywhere adds nothing, not even 0.0 * cot)
        np.add.at(grad, g[touched], rows[touched])
    return grad


def loss_and_cotangent(image, target, mask=None, loss="l1", xp=np):
    """(loss, dloss/dimage) of FeatureField.trainStep on a feature image [H, W, C]: the mean over all H W C elements of
    |d| ("l1") or d^2 ("l2"), d = w (image - target), w = mask / 255 of an optional uint8 mask [H, W] (no re-normalisation by
    coverage, as the loss masks).  xp: numpy or torch."""
    if loss not in ("l1", "l2"):
        raise ValueError(f"loss must be \"l1\" or \"l2\", got {loss!r}")
    d = image - target
    w = None
    if mask is not None:
        w = (mask.astype(d.dtype) if xp is np else mask.to(d.dtype))[..., None] / 255
        d = d * w
    n = d.size if xp is np else d.numel()
    if loss == "l1":
        value, cot = xp.abs(d).sum() / n, xp.sign(d) / n
    else:
        value, cot = (d * d).sum() / n, 2 * d / n
    return value, cot if w is None else cot * w


def adam_reference(f, g, m, v, lr, dtype=np.float64):
    """One step of the trainer's Adam (gs_adam_step) on the host, in place, in `dtype`."""
    b1, b2, eps, lr = dtype(ADAM_BETA1), dtype(ADAM_BETA2), dtype(ADAM_EPS), dtype(lr)
    m[...] = b1 * m + (dtype(1) - b1) * g
    v[...] = b2 * v + (dtype(1) - b2) * g * g
    f[...] = f - lr * m / (np.sqrt(v) + eps)


class FeatureField:
    """A C-channel feature field on the Gaussians of a trained scene: features [N, C] and two Adam moments on the device.
    lr: Feature-3DGS's semantic-feature rate.  The field does not follow densify or prune events: N is fixed."""

    def __init__(self, renderer, N: int, C: int, lr: float = 1e-3, init=None):
        import torch
        N, C = int(N), int(C)
        if N < 1 or not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"FeatureField: N >= 1 and 1 <= C <= {MAX_CHANNELS}, got N = {N}, C = {C}")
        self.renderer, self.N, self.C, self.lr = renderer, N, C, float(lr)
        self.features = torch.zeros((N, C), dtype=torch.float32, device=renderer.device)
        if init is not None:
            init = torch.as_tensor(init, dtype=torch.float32)
            if tuple(init.shape) != (N, C):
                raise ValueError(f"FeatureField: init must be [{N}, {C}], got {tuple(init.shape)}")
            self.features.copy_(init)
        self.m, self.v, self.grad = (torch.zeros_like(self.features) for _ in range(3))

    def _forward(self, who, params, camera, viewKey):
        n = int(params["xyz"].shape[0])
        if n != self.N:
            raise ValueError(f"{who}: the field holds {self.N} Gaussians, params has {n}")
        self.renderer.renderChecked(params, camera, viewKey=viewKey, wantDepth=False)

    def render(self, params, camera, viewKey=None):
        """The feature image [H, W, C] of the scene `params` from `camera`."""
        self._forward("FeatureField.render", params, camera, viewKey)
        return self.renderer.renderFeatures(self.features)

    def trainStep(self, params, camera, target, mask=None, loss: str = "l1", viewKey=None):
        """One Adam step of the features towards the feature image target [H, W, C] (mask: optional uint8 [H, W], weight
        v / 255); returns the loss before the step as a 0-dim device tensor."""
        import torch
        r = self.renderer
        if loss not in ("l1", "l2"):
            raise ValueError(f"FeatureField.trainStep: loss must be \"l1\" or \"l2\", got {loss!r}")
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (r.H, r.W, self.C):
            raise ValueError(f"FeatureField.trainStep: target must be a tensor [{r.H}, {r.W}, {self.C}]")
        if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (r.H, r.W)):
            raise ValueError(f"FeatureField.trainStep: mask must be a uint8 tensor [{r.H}, {r.W}]")
        self._forward("FeatureField.trainStep", params, camera, viewKey)
        image = r.renderFeatures(self.features)
        value, cot = loss_and_cotangent(image, target.to(image), None if mask is None else mask.to(image.device), loss, xp=torch)
        r.renderFeaturesVJP(cot.contiguous(), self.grad.zero_())
        n = self.N * self.C
        r._check(r.lib.gs_adam_step(r.ctx, n, ctypes.c_void_p(self.features.data_ptr()), ctypes.c_void_p(self.grad.data_ptr()),
                                    ctypes.c_void_p(self.m.data_ptr()), ctypes.c_void_p(self.v.data_ptr()), 1, (ctypes.c_longlong * 1)(n),
                                    (ctypes.c_float * 1)(self.lr), ctypes.c_float(ADAM_BETA1), ctypes.c_float(ADAM_BETA2), ctypes.c_float(ADAM_EPS),
                                    ctypes.c_float(1.0)))
        return value
