"""Contribution-based pruning without a device (gaussiansplattingmlx_amd/contrib_prune.py, include/gsplat.h gs_blend_contrib,
DESIGN.md section 15): the numpy statement of the blend weight scores against the oracle it restates, on the oracle's own tile
lists; hand-built occluded and off-screen Gaussians; the action rule; the settings' validation; the trainer's refusals; the
entry points' declaration.  Also the scenes the GPU tests of the op-level kernel use (op_scene).

The identity the first test rests on: w(p, g) = T alpha = T - T (1 - alpha), so the weights of a pixel telescope to
sum over g of w = 1 - T_final, which is the blend's alpha image; with every colour set to 1 the blend's red channel is that
sum term by term.  (T_final = 1 - alpha: the transmittance is what 1 - sum of w equals.)

Bars.  Against the float64 oracle 1e-12: the same arithmetic in the same order, exp from two libraries (an ulp, 1e-16, per
entry over lists of a few hundred entries).  Against the float32 oracle the project's image bar, 1e-4.
"""
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import contrib_prune as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gs_blend_contrib", "gs_render_contrib", "gs_contrib_actions")


# ---------------------------------------------------------------------------------------------------------------- scenes
def op_scene(W, H, N, seed, layer_depth=10.0, radius=(3.0, 12.0)):
    """Packed records [N, 11] float32 and rects for an op-level binning, built in screen space:
      rows [0, n)          random splats, depths in (2, 9), means up to 5 px outside the image
      row  n               one faint splat spanning every tile, in front of everything (depth 0.5)
      rows n+1 .. n+6      a full-image opaque layer at `layer_depth`: six flat splats of opacity 0.95 -- T = 0.05^k falls
                           below 1e-4 at the fourth in any precision (1.25e-4, then 6.25e-6: nowhere near the threshold)
      rows n+7 .. n+16     ten splats behind the layer (depth 20+): fully occluded
      the last eight rows  off-screen: four with rects outside the image, four with radius 0
    Returns dict(packed, rectMin, rectMax, radii, depths, occluded, offscreen, spanning)."""
    rng = np.random.default_rng(seed)
    n = N - 25
    assert n > 0
    packed = np.zeros((N, 11), np.float32)
    rad = np.zeros(N, np.float32)
    packed[:n, 0] = rng.uniform(-5, W + 5, n); packed[:n, 1] = rng.uniform(-5, H + 5, n)
    r = rng.uniform(radius[0], radius[1], n)
    sx, sy = r / 3 * rng.uniform(0.5, 1.0, n), r / 3 * rng.uniform(0.5, 1.0, n)
    rho = rng.uniform(-0.6, 0.6, n)
    det = (sx * sy) ** 2 * (1 - rho ** 2)
    packed[:n, 2] = sy ** 2 / det; packed[:n, 5] = sx ** 2 / det
    packed[:n, 3] = packed[:n, 4] = -rho * sx * sy / det
    packed[:n, 9] = rng.uniform(0.05, 0.9, n)
    packed[:n, 10] = rng.uniform(2.0, 9.0, n)
    rad[:n] = r
    # the spanning splat
    packed[n, 0:2] = (W / 2, H / 2); packed[n, 2] = packed[n, 5] = 1e-4; packed[n, 9] = 0.1; packed[n, 10] = 0.5
    rad[n] = 4 * max(W, H)
    # the opaque layer
    lay = slice(n + 1, n + 7)
    packed[lay, 0] = W / 2; packed[lay, 1] = H / 2; packed[lay, 2] = packed[lay, 5] = 1e-9; packed[lay, 9] = 0.95
    packed[lay, 10] = layer_depth + 0.05 * np.arange(6)
    rad[lay] = 4 * max(W, H)
    # behind it
    occ = slice(n + 7, n + 17)
    packed[occ, 0] = rng.uniform(4, W - 4, 10); packed[occ, 1] = rng.uniform(4, H - 4, 10)
    packed[occ, 2] = packed[occ, 5] = 0.02; packed[occ, 9] = 0.8; packed[occ, 10] = layer_depth + 10 + rng.uniform(0, 5, 10)
    rad[occ] = 12.0
    # off-screen
    off = slice(N - 8, N)
    packed[off, 0] = (-300, W + 300, W / 2, -250, W / 2, 3, W - 3, W / 3); packed[off, 1] = (H / 2, H / 2, H + 400, -250, H / 2, 3, H - 3, H / 3)
    packed[off, 2] = packed[off, 5] = 0.02; packed[off, 9] = 0.9; packed[off, 10] = 1.0
    rad[off] = (9.0, 9.0, 9.0, 9.0, 0.0, 0.0, 0.0, 0.0)
    packed[:, 6:9] = rng.uniform(0, 1, (N, 3))
    rmin = (packed[:, 0:2] - rad[:, None]).astype(np.float32)
    rmax = (packed[:, 0:2] + rad[:, None]).astype(np.float32)
    occluded = np.zeros(N, bool); occluded[n + 5:n + 17] = True      # the layer's last two and everything behind it
    offscreen = np.zeros(N, bool); offscreen[off] = True
    return dict(packed=packed, rectMin=rmin, rectMax=rmax, radii=rad, depths=packed[:, 10].copy(), occluded=occluded,
                offscreen=offscreen, spanning=n)


def _lists(o, s, W, H, tile):
    return o.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], W, H, tile[0], tile[1])


# ------------------------------------------------------------------------------------------- the rule against the oracle
@pytest.mark.parametrize("W,H,tile,N", [(48, 40, (16, 16), 300), (64, 64, (32, 32), 500), (50, 38, (25, 19), 200)])
def test_weights_sum_to_the_oracles_alpha_and_unit_colour_image(oracle32, oracle64, W, H, tile, N):
    s = op_scene(W, H, N, seed=5)
    packed = s["packed"].copy()
    packed[:, 6:9] = 1.0
    bn = _lists(oracle64, s, W, H, tile)
    max_w, sum_w, image = cp.blend_weights(packed, bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], per_pixel=True)
    assert image.min() > 1.0 - 1.3e-4            # every pixel reaches the opaque layer and stops inside it (T < 1.25e-4)
    for o, bar in ((oracle64, 1e-12), (oracle32, 1e-4)):
        color, _, alpha, _ = o.blend_forward(packed, bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], False)
        assert np.abs(image.reshape(-1) - color[:, 0]).max() <= bar
        # 1 - sum of w is the final transmittance, 1 - alpha
        assert np.abs((1.0 - image.reshape(-1)) - (1.0 - alpha.astype(np.float64))).max() <= bar
    alpha64 = oracle64.blend_forward(packed, bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], False)[2]
    assert abs(sum_w.sum() - alpha64.sum()) <= 1e-12 * W * H
    assert np.all(max_w <= 0.99 + 1e-15) and np.all(max_w >= 0) and np.all(sum_w >= max_w - 1e-15)
    # occluded and off-screen: exactly 0; the spanning splat is seen by every pixel
    assert not max_w[s["occluded"]].any() and not sum_w[s["occluded"]].any()
    assert not max_w[s["offscreen"]].any() and not sum_w[s["offscreen"]].any()
    assert sum_w[s["spanning"]] > 0.05 * W * H and 0.09 < max_w[s["spanning"]] <= 0.1 + 1e-8


def test_hand_built_occlusion_and_stop(oracle64):
    """One tile of identical pixels by hand: a splat of alpha 0.3 in front of an opaque stack, one more behind it."""
    W = H = 16
    packed = np.zeros((7, 11))
    packed[:, 0:2] = 8.0
    packed[:, 2] = packed[:, 5] = 1e-12                  # flat: exp(...) = 1 to 1e-10
    packed[:, 9] = (0.3, 0.95, 0.95, 0.95, 0.95, 0.95, 0.7)
    packed[:, 10] = np.arange(1, 8)
    rmin, rmax = np.zeros((7, 2)), np.full((7, 2), 15.0)
    bn = oracle64.tile_bin(rmin, rmax, np.ones(7), packed[:, 10], W, H, 16, 16)
    assert bn.sortedIdx.tolist() == list(range(7))
    max_w, sum_w = cp.blend_weights(packed, bn.sortedIdx, bn.tileRanges, W, H, 16, 16)
    alpha = packed[:, 9]
    after = np.cumprod(1.0 - alpha)                       # T behind entry j: 0.7, 0.035, 1.75e-3, 8.75e-5, ...
    before = np.concatenate([[1.0], after[:-1]])
    stop = int(np.argmax(after < cp.T_STOP))              # the entry that brings T below 1e-4
    assert stop == 3
    want = np.where(np.arange(7) <= stop, before * alpha, 0.0)
    assert np.abs(max_w - want).max() <= 1e-9
    assert np.abs(sum_w - want * 256).max() <= 1e-7
    assert not max_w[4:].any() and not sum_w[4:].any()    # behind the stop: exactly 0


# --------------------------------------------------------------------------------------------------------- the action rule
def test_action_rule():
    score = np.array([0.0, 0.0099999, 0.01, 0.010001, 0.5, np.nan])
    actions, counts = cp.contrib_actions(score, 0.01)
    assert actions.dtype == np.int32 and counts.dtype == np.int32
    assert actions.tolist() == [3, 3, 0, 0, 0, 0] and counts.tolist() == [0, 0, 1, 1, 1, 1]      # (NaN < t is false: kept)
    assert np.array_equal(counts == 0, actions == 3)


# ----------------------------------------------------------------------------------------------------------- the settings
def test_config_defaults_and_events():
    c = cp.ContribPruneConfig(cameras=[object()]).validate()
    assert c.threshold == 0.01 and tuple(c.at) == (16000, 24000) and c.score == "max"
    assert c.is_event(16000) and c.is_event(24000) and not c.is_event(0) and not c.is_event(16001)
    assert cp.ContribPruneConfig(threshold=1.0, cameras=[1]).validate()
    assert cp.ContribPruneConfig(threshold=250.0, score="sum", cameras=[1], at=[5]).validate()


@pytest.mark.parametrize("kw", [dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=1.5), dict(threshold=float("nan")),
                                dict(threshold=float("inf"), score="sum"), dict(threshold=None), dict(threshold=True),
                                dict(threshold=0.0, score="sum"), dict(score="mean"), dict(at=(0,)), dict(at=(5, 5)),
                                dict(at=(7, 3)), dict(at=(2.5,)), dict(at=(True,)), dict(at=3), dict(cameras=None),
                                dict(cameras=[]), dict(cameras=5)])
def test_config_refuses(kw):
    args = dict(cameras=[object()])
    args.update(kw)
    with pytest.raises(ValueError):
        cp.ContribPruneConfig(**args).validate()


@pytest.mark.parametrize("kw", [dict(strategy="mcmc"), dict(process_group=object()), dict(views_per_rank=2),
                                dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(contrib_prune=dict(threshold=0.01)),
                                dict(contrib_prune=cp.ContribPruneConfig(threshold=2.0, cameras=[1]))])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(contrib_prune=cp.ContribPruneConfig(cameras=[object()]))
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "#define GSPLAT_ABI_VERSION 6" in src
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
    assert "contrib.hip" in __import__("gaussiansplattingmlx_amd.build", fromlist=["SOURCES"]).SOURCES


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_blend_contrib(None, 0, None, None, None) == 1
    assert lib.gs_render_contrib(None, None, None) == 1
    import ctypes
    assert lib.gs_contrib_actions(None, 0, None, ctypes.c_float(0.01), None, None) == 1
