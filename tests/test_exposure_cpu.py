"""Exposure compensation without a device: the numpy restatement's VJP against central differences of the float64 composed
loss (tests/exposure_numpy.py), the trainer's learning-rate schedule and refusals, and the header's declarations
(include/gsplat.h gs_set_exposure, gs_apply_exposure)."""
import importlib.util
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_expoc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


en = _load("exposure_numpy")


def test_identity_is_the_image():
    rng = np.random.default_rng(1)
    img = rng.uniform(0, 1, (7, 5, 3)).astype(np.float32)
    assert np.array_equal(en.apply(en.IDENTITY, img, np.float32), img)
    g = rng.normal(0, 1, img.shape)
    dr, _ = en.vjp(en.IDENTITY, g, img)
    assert np.array_equal(dr, g)


@pytest.mark.parametrize("depth", [False, True])
def test_vjp_against_central_differences(oracle64, depth):
    """The restated VJP against central differences of the float64 composed loss, all 12 components.  h = 1e-5 on a loss of
    O(0.1) leaves a rounding error of ~1e-16 / 1e-5 = 1e-11 and a truncation error of O(h^2); the loss is smooth in M away
    from the L1 kink, which a random image meets with probability ~0.  Bar: 1e-6 of the gradient's largest component."""
    H, W = 24, 30
    rng = np.random.default_rng(11)
    ren = rng.uniform(0, 1, (H, W, 3))
    tgt = np.clip(ren + rng.normal(0, 0.15, ren.shape), 0, 1)
    kw = {}
    if depth:
        kw = dict(renderDepth=rng.uniform(1, 4, (H, W)), targetDepth=rng.uniform(1, 4, (H, W)),
                  depthMask=rng.uniform(size=(H, W)) > 0.5, lambdaDepth=0.3)
    M = en.random_exposure(rng).astype(np.float64)
    _, dr, dM, g = en.composed(oracle64, ren, tgt, M, 0.2, **kw)
    h = 1e-5
    fd = np.empty(12)
    for k in range(12):
        Mp, Mm = M.copy(), M.copy()
        Mp[k] += h
        Mm[k] -= h
        fd[k] = (en.composed(oracle64, ren, tgt, Mp, 0.2, **kw)[0] - en.composed(oracle64, ren, tgt, Mm, 0.2, **kw)[0]) / (2 * h)
    assert np.abs(fd - dM).max() <= 1e-6 * np.abs(dM).max(), (fd, dM)
    # dL/dr: the render's own cotangent is A^T g (one pixel, one channel, by differences)
    p, j = (5, 7), 1
    rp, rm = ren.copy(), ren.copy()
    rp[p][j] += h
    rm[p][j] -= h
    fdr = (en.composed(oracle64, rp, tgt, M, 0.2, **kw)[0] - en.composed(oracle64, rm, tgt, M, 0.2, **kw)[0]) / (2 * h)
    assert abs(fdr - dr[p][j]) <= 1e-6 * np.abs(dr).max(), (fdr, dr[p][j])


def test_learning_rate_schedule():
    from gaussiansplattingmlx_amd.trainer import exposureLearningRate
    T = 30000
    assert math.isclose(exposureLearningRate(0, T), 0.01, rel_tol=1e-12)
    assert math.isclose(exposureLearningRate(T, T), 0.001, rel_tol=1e-12)
    assert math.isclose(exposureLearningRate(T // 2, T), math.sqrt(1e-5), rel_tol=1e-12)
    assert math.isclose(exposureLearningRate(3 * T, T), 0.001, rel_tol=1e-12)         # held at the final rate
    assert math.isclose(exposureLearningRate(0, T, (0.02, 0.002)), 0.02, rel_tol=1e-12)
    lrs = [exposureLearningRate(t, T) for t in range(0, T + 1, 1000)]
    assert all(a > b for a, b in zip(lrs, lrs[1:]))


@pytest.mark.parametrize("kw", [dict(views_per_rank=2), dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)),
                                dict(exchange_impl="native"), dict(n_views=None), dict(n_views=0), dict(n_views=2.5),
                                dict(n_views=-1), dict(exposure_lr=(0.01,)), dict(exposure_lr=(0.01, 0.0)),
                                dict(exposure_lr=(0.01, float("nan"))), dict(exposure_lr="fast"), dict(exposure_lr=None)])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(exposure_opt=True, n_views=4)
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_header_declares_and_library_exports_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "int gs_set_exposure(gs_ctx* ctx, const float* M" in src
    assert "int gs_apply_exposure(gs_ctx* ctx, long long n_pixels, const float* M" in src
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import _lib
    assert {"gs_set_exposure", "gs_apply_exposure"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert hasattr(lib, "gs_set_exposure") and hasattr(lib, "gs_apply_exposure")


def test_hip_source_is_built_without_contraction():
    from gaussiansplattingmlx_amd import build
    assert build.SOURCES["exposure.hip"] == ["-ffp-contract=off"]
