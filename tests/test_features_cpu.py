"""N-channel feature rendering without a device (gaussiansplattingmlx_amd/features.py, include/gsplat.h gs_blend_features,
DESIGN.md section 31): the numpy statement of the feature forward against the oracle's blend and against
contrib_prune.blend_weights, on the oracle's own tile lists; the adjoint identity that is the whole derivative check of a map
linear in the features; the rows of occluded and off-screen Gaussians; the entry points' declaration; and the host form of
the training loop the GPU test repeats on the device (train_case / host_loop).

Bars.  Against the float64 oracle and between the two float64 host statements 1e-12: the same arithmetic in the same order
(exp from two libraries, an ulp per entry over lists of a few hundred entries).  The adjoint identity 1e-12 relative to
sum |cot out|: two orders of summation of the same float64 products.  The training case's float32 / float64 distance: 1e-3
(a condition on the chosen case, see host_loop).
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import contrib_prune as cp
from gaussiansplattingmlx_amd import features as ft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = ("gs_blend_features", "gs_blend_features_backward", "gs_render_features", "gs_render_features_backward",
           "gs_feature_channel_group")


def _load(name):
    spec = importlib.util.spec_from_file_location("_ftc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_contrib_prune_cpu")
CASES = [(48, 40, (16, 16), 300), (64, 64, (32, 32), 500), (50, 38, (25, 19), 200)]
_cache = {}


def _case(oracle64, W, H, tile, N):
    key = (W, H, tile, N)
    if key not in _cache:
        s = cpu.op_scene(W, H, N, seed=5)
        bn = oracle64.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], W, H, tile[0], tile[1])
        lists = (s["packed"], bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1])
        _cache[key] = (s, bn, lists, ft.tile_weights(*lists))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. the model against the oracle
@pytest.mark.parametrize("W,H,tile,N", CASES)
def test_model_matches_the_oracles_colour_and_the_weight_image(oracle64, W, H, tile, N):
    s, bn, lists, weights = _case(oracle64, W, H, tile, N)
    color = oracle64.blend_forward(s["packed"], bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], False)[0]
    got = ft.blend_features(*lists, s["packed"][:, 6:9], weights=weights)
    assert got.shape == (H, W, 3) and got.dtype == np.float64
    assert np.abs(got.reshape(-1, 3) - color).max() <= 1e-12
    image = cp.blend_weights(*lists, per_pixel=True)[2]
    ones = ft.blend_features(*lists, np.ones((N, 1)))            # (the weights recomputed: the argument is optional)
    assert np.abs(ones[:, :, 0] - image).max() <= 1e-12
    # and the sums over the pixels are contrib_prune's per-Gaussian sums
    sum_w = cp.blend_weights(*lists)[1]
    assert np.abs(ft.blend_features_vjp(*lists, np.ones((H, W, 1)), weights=weights)[:, 0] - sum_w).max() <= 1e-12 * W * H


# --------------------------------------------------------------------------------------------------------- 2. adjoint identity
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("W,H,tile,N", CASES)
def test_adjoint_identity(oracle64, W, H, tile, N, C):
    s, bn, lists, weights = _case(oracle64, W, H, tile, N)
    rng = np.random.default_rng(100 + C)
    f, cot = rng.uniform(-1, 1, (N, C)), rng.uniform(-1, 1, (H, W, C))
    out = ft.blend_features(*lists, f, weights=weights)
    grad = ft.blend_features_vjp(*lists, cot, weights=weights)
    assert grad.shape == (N, C)
    lhs, rhs = (cot * out).sum(), (grad * f).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(cot * out).sum()
    assert np.abs(cot * out).sum() > 1.0


# --------------------------------------------------------------------------------------------------------------- 3. VJP rows
@pytest.mark.parametrize("W,H,tile,N", CASES)
def test_vjp_rows_of_unseen_gaussians_are_zero(oracle64, W, H, tile, N):
    s, bn, lists, weights = _case(oracle64, W, H, tile, N)
    cot = np.random.default_rng(3).uniform(-1, 1, (H, W, 4))
    grad = ft.blend_features_vjp(*lists, cot, weights=weights)
    assert not grad[s["occluded"]].any() and not grad[s["offscreen"]].any()
    assert np.abs(grad[s["spanning"]]).max() > 0


# -------------------------------------------------------------------------------------------------------------- 4. entry points
def test_header_binding_and_group_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "#define GSPLAT_ABI_VERSION 6" in src and "#define GS_MAX_FEATURE_CHANNELS 256" in src
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
    assert "features.hip" in __import__("gaussiansplattingmlx_amd.build", fromlist=["SOURCES"]).SOURCES
    assert ft.MAX_CHANNELS == _lib.MAX_FEATURE_CHANNELS == 256
    kernel = open(os.path.join(ROOT, "gaussiansplattingmlx_amd", "csrc", "features.hip")).read()
    assert re.search(r"#define GS_FEATURE_GROUP (\d+)", kernel).group(1) == str(ft.CHANNEL_GROUP)
    import gaussiansplattingmlx_amd
    assert gaussiansplattingmlx_amd.FeatureField is ft.FeatureField


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_blend_features(None, 0, 1, None, None, None) == 1
    assert lib.gs_blend_features_backward(None, 0, 1, None, None, None) == 1
    assert lib.gs_render_features(None, 1, None, None) == 1
    assert lib.gs_render_features_backward(None, 1, None, None) == 1
    assert lib.gs_feature_channel_group() == ft.CHANNEL_GROUP


def test_loss_and_cotangent_is_the_derivative():
    rng = np.random.default_rng(9)
    img, tgt = rng.uniform(-1, 1, (6, 5, 3)), rng.uniform(-1, 1, (6, 5, 3))
    mask = rng.integers(0, 256, (6, 5)).astype(np.uint8)
    for loss in ("l1", "l2"):
        for m in (None, mask):
            v, cot = ft.loss_and_cotangent(img, tgt, m, loss)
            d = rng.uniform(-1, 1, img.shape) * 1e-7
            v2 = ft.loss_and_cotangent(img + d, tgt, m, loss)[0]
            assert abs((v2 - v) - (cot * d).sum()) <= 1e-12, (loss, m is None)
    with pytest.raises(ValueError):
        ft.loss_and_cotangent(img, tgt, None, "huber")


# ------------------------------------------------------------------------------------------------------- 5. the training loop
TRAIN = dict(W=64, H=48, N=400, seed=17, C=8, loss="l2", lr=1e-3, steps=5, fseed=23)


def train_case(oracle64):
    """The scene, lists and target of the training test: op_scene(64, 48, 400, seed=17), C = 8, the target the float64 render
    of a seeded f*."""
    t = TRAIN
    s = cpu.op_scene(t["W"], t["H"], t["N"], seed=t["seed"])
    bn = oracle64.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], t["W"], t["H"], 16, 16)
    lists = (s["packed"], bn.sortedIdx, bn.tileRanges, t["W"], t["H"], 16, 16)
    fstar = np.random.default_rng(t["fseed"]).uniform(-1, 1, (t["N"], t["C"]))
    target = ft.blend_features(*lists, fstar)
    return s, bn, lists, target


def host_loop(lists, target, N, C, dtype, steps=TRAIN["steps"], lr=TRAIN["lr"], loss=TRAIN["loss"]):
    """FeatureField.trainStep on the host in `dtype` from zeros: the per-step losses.  The weights are computed once (the
    geometry is frozen)."""
    weights = ft.tile_weights(*lists, dtype=dtype)
    f, m, v = (np.zeros((N, C), dtype) for _ in range(3))
    tgt = np.asarray(target, dtype)
    losses = []
    for _ in range(steps):
        img = ft.blend_features(*lists, f, dtype=dtype, weights=weights)
        value, cot = ft.loss_and_cotangent(img, tgt, None, loss)
        losses.append(float(value))
        g = ft.blend_features_vjp(*lists, cot.astype(dtype), dtype=dtype, weights=weights, N=N)
        ft.adam_reference(f, g, m, v, lr, dtype)
    return np.array(losses)


def relative_distance(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.abs(b)


def test_training_loop_on_the_host(oracle64):
    s, bn, lists, target = train_case(oracle64)
    l64 = host_loop(lists, target, TRAIN["N"], TRAIN["C"], np.float64)
    l32 = host_loop(lists, target, TRAIN["N"], TRAIN["C"], np.float32)
    d32 = relative_distance(l32, l64)
    print("float64 losses", l64, "d32", d32)
    assert (np.diff(l64) < 0).all()
    assert d32.max() < 1e-3
