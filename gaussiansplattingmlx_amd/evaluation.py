"""Held-out evaluation (include/gsplat.h gs_image_metrics / gs_colour_moments): the view split, the
host half of the metrics and the result container.  Pure numpy; tests/metrics_numpy.py restates the device half.

    psnr = -10 log10(sse / (3 wsum))        inf for identical images, nan where nothing is weighted in
    ssim = ssim_sum / (3 wsum)              Inria's loss_utils.ssim: the CENTRED 11 x 11 window (centred_window), not the
                                            off-centre one the training loss inherits from the reference app
    cc_*   the same two of M p against the target, M = [A | b] the least-squares affine colour transform of the render onto
           the target (fit_affine_colour, from the 22 moment sums of gs_colour_moments): what gsplat reports when a per-view
           appearance is trained, because a held-out view has no learnt exposure or grid

split_views is the Mip-NeRF 360 / Inria `llffhold` convention: every test_every-th view is held out.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np


def centred_window(K: int = 11, sigma: float = 1.5) -> np.ndarray:
    """Inria's create_window: float32 [K, K], the outer product of the normalised taps exp(-(i - K // 2)^2 / (2 sigma^2)),
    each step in float32 as gs_image_metrics forms its eleven."""
    d = (np.arange(K) - K // 2).astype(np.float32)
    g = np.exp(-(d * d) / np.float32(2.0 * sigma * sigma)).astype(np.float32)
    g = g / g.sum(dtype=np.float32)
    return np.outer(g, g).astype(np.float32)


def split_views(n: int, test_every: int = 8, offset: int = 0):
    """(train_idx, test_idx), int64: view i is held out iff i % test_every == offset; test_every <= 0 holds out nothing."""
    idx = np.arange(int(n), dtype=np.int64)
    if test_every <= 0:
        return idx, idx[:0]
    held = idx % int(test_every) == int(offset)
    return idx[~held], idx[held]


def split_train_data(trainData, test_every: int = 8, offset: int = 0):
    """(train, test): two TrainData with every per-view array sliced by split_views; a field that is None stays None."""
    tr, te = split_views(len(trainData.Hs), test_every, offset)

    models = getattr(trainData, "cameraModelArray", None)       # (attributes beside the fields: data.TrainData)
    normals = getattr(trainData, "normalArray", None)

    def take(idx):
        return trainData.replace(cameraModelArray=None if models is None else np.asarray(models)[idx],
                                 normalArray=None if normals is None else np.asarray(normals)[idx],
                                 **{f.name: (None if getattr(trainData, f.name) is None else np.asarray(getattr(trainData, f.name))[idx])
                                    for f in dataclasses.fields(trainData)})
    return take(tr), take(te)


_TRIU = [(i, j) for i in range(4) for j in range(i, 4)]


def fit_affine_colour(moments) -> np.ndarray:
    """M = [A | b], float32 [3, 4] as gs_apply_exposure takes it, from the 22 moments of gs_colour_moments (S's upper triangle
    by rows, then T [4, 3]): M^T = lstsq(S, T) in float64.  A constant or blank render makes S singular; the minimum-norm
    solution is the answer then."""
    m = np.asarray(moments, np.float64).reshape(22)
    S = np.zeros((4, 4))
    for k, (i, j) in enumerate(_TRIU):
        S[i, j] = S[j, i] = m[k]
    T = m[10:].reshape(4, 3)
    Mt = np.linalg.lstsq(S, T, rcond=None)[0]
    return np.ascontiguousarray(Mt.T, np.float32)


def metrics_from_sums(sums):
    """(psnr, ssim, weight) from gs_image_metrics' {sse, ssim_sum, wsum, 3 wsum}, one view [4] or many [V, 4], float64: psnr
    is inf where the error is zero, both are nan where wsum is."""
    s = np.asarray(sums, np.float64)
    sse, ssum, wsum, w3 = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = -10.0 * np.log10(sse / w3)
        ssim = ssum / w3
    return psnr, ssim, wsum


_METRICS = ("psnr", "ssim", "cc_psnr", "cc_ssim")


@dataclass
class EvalResult:
    """Per-view arrays (float64 [V]; cc_* None without colour correction; weight = the view's sum of mask weights), their
    means over the views whose value is finite (mean_psnr, ... : nan where no view is), and how many views each mean left out
    (skipped["psnr"], ...: a fully masked view is nan, identical images are inf)."""
    psnr: np.ndarray
    ssim: np.ndarray
    cc_psnr: np.ndarray | None
    cc_ssim: np.ndarray | None
    weight: np.ndarray

    def _finite(self, name):
        v = getattr(self, name)
        return None if v is None else np.asarray(v, np.float64)[np.isfinite(v)]

    def mean(self, name: str) -> float:
        v = self._finite(name)
        return float("nan") if v is None or v.size == 0 else float(v.mean())

    @property
    def skipped(self) -> dict:
        return {k: (0 if getattr(self, k) is None else int(len(getattr(self, k)) - self._finite(k).size)) for k in _METRICS}

    mean_psnr = property(lambda self: self.mean("psnr"))
    mean_ssim = property(lambda self: self.mean("ssim"))
    mean_cc_psnr = property(lambda self: self.mean("cc_psnr"))
    mean_cc_ssim = property(lambda self: self.mean("cc_ssim"))

    @classmethod
    def from_sums(cls, sums, cc_sums=None):
        psnr, ssim, weight = metrics_from_sums(np.asarray(sums, np.float64).reshape(-1, 4))
        cc = (None, None) if cc_sums is None else metrics_from_sums(np.asarray(cc_sums, np.float64).reshape(-1, 4))[:2]
        return cls(psnr, ssim, cc[0], cc[1], weight)
