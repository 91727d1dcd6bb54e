"""AbsGS densification without a device (gaussiansplattingmlx_amd/absgrad.py, include/gsplat.h gs_set_absgrad, DESIGN.md
section 16): the numpy statement of the per-pixel absolute 2-D gradient sums against the oracle it restates -- its SIGNED sums
are columns 0 and 1 of the oracle's blend backward --, the cancellation it is there to see through, its sensitivity to float32
stops, the statistic, the settings' validation, the trainer's refusals and the entry points' declaration.

The scene is the one the GPU tests use (test_gpu_trajectory._scene(71, 3000, 160, 120, 0.06), camera 0): tile lists of up to
1521 entries at 16 x 16 and 2739 at 50 x 38, far beyond the blend backward's 64-entry segments and 256-entry chunks.

Bars.  Signed sums against the float64 oracle: 1e-9 max-normalised (measured 5e-13: the same terms, the oracle sweeps a pixel's
list backwards from the final transmittance, the rule forwards from 1).  Float32 records, colours and stops fed to the float64
rule against the all-float64 result: 1e-4 (measured 1.5e-6, one pixel stopping one entry apart) -- the device bar of 1e-3 is
met by the reference alone with a wide margin.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import absgrad as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("gs_set_absgrad", "gs_get_absgrad")
W, H, N = 160, 120, 3000
TILES = ((16, 16), (50, 38))
VARIANTS = ("plain", "depth", "alpha", "white")


def _load(name):
    spec = importlib.util.spec_from_file_location("_abs_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_cache = {}


def scene():
    if "scene" not in _cache:
        _cache["scene"] = _load("test_gpu_trajectory")._scene(71, N, W, H, 0.06)
    return _cache["scene"]


def cotangents(variant):
    """(cotColor [H, W, 3], cotDepth [H, W] or None, cotAlpha [H, W] or None) in float64; the colour cotangent is the issue's."""
    cot = np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)
    cd = np.random.default_rng(4).standard_normal((H, W)) / (W * H) if variant == "depth" else None
    ca = np.random.default_rng(5).standard_normal((H, W)) / (W * H) if variant == "alpha" else None
    return cot, cd, ca


def forward(o, tile, white):
    key = ("fw", np.dtype(o.dtype).name, tile, white)
    if key not in _cache:
        p, cams = scene()
        _cache[key] = o.render_forward(p, cams[0].as_dict(), W, H, tile[0], tile[1], 4, whiteBg=white)
    return _cache[key]


def rule(fw, tile, variant):
    """blend_absgrad in float64 on a forward's records, lists and outputs."""
    cot, cd, ca = cotangents(variant)
    bn = fw["bin"]
    return ag.blend_absgrad(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], cot, fw["color"], fw["last"],
                            cotDepth=cd, outDepth=None if cd is None else fw["depth"],
                            cotAlpha=ca, outAlpha=None if ca is None else fw["alpha"])


def want(oracle64, tile, variant):
    """(A, S) of the float64 rule on the float64 oracle's forward: computed once per (tile, variant), never changed."""
    key = ("want", tile, variant)
    if key not in _cache:
        A, S = rule(forward(oracle64, tile, variant == "white"), tile, variant)
        A.setflags(write=False)
        S.setflags(write=False)
        _cache[key] = (A, S)
    return _cache[key]


def _maxnorm(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------------- the rule against the oracle
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tile", TILES)
def test_signed_sums_are_the_oracles_mean_gradient(oracle64, tile, variant):
    white = variant == "white"
    fw = forward(oracle64, tile, white)
    bn = fw["bin"]
    counts = bn.tileRanges.reshape(-1, 2).astype(np.int64)
    assert (counts[:, 1] - counts[:, 0]).max() == (1521 if tile == (16, 16) else 2739)
    cot, cd, ca = cotangents(variant)
    z = np.zeros(W * H)
    gp = oracle64.blend_backward(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], white, cot.reshape(-1, 3),
                                 z if cd is None else cd.reshape(-1), z if ca is None else ca.reshape(-1), fw["color"],
                                 fw["depth"], fw["alpha"], fw["last"])
    A, S = want(oracle64, tile, variant)
    for col in range(2):
        err = _maxnorm(S[:, col], gp[:, col])
        print(f"{tile} {variant} column {col}: signed sums against the oracle {err:.3e} (bar 1e-9)")
        assert err <= 1e-9
    if variant != "plain":          # (the cotangent, or the background, matters on this scene)
        assert _maxnorm(S, want(oracle64, tile, "plain")[1]) > 1e-3
    # A >= |S| element-wise, with no exceptions: |sum| <= sum of | | term by term, in the same order
    assert np.all(A >= np.abs(S))
    assert np.all(A >= 0)
    if variant == "plain":
        nz = int((A.sum(axis=1) > 0).sum())
        assert nz == int((np.abs(S).sum(axis=1) > 0).sum()) == (2519 if tile == (16, 16) else 2768)      # of the 3000
        ratio = A.max() / np.abs(S).max()
        print(f"{tile}: max A / max |S| = {ratio:.2f}")
        assert ratio >= 5.0


def test_float32_stops_move_the_sums_little(oracle32, oracle64):
    """The float32 oracle's records, colours and stops through the float64 rule: what a float32 forward can move."""
    tile = (16, 16)
    A64, S64 = want(oracle64, tile, "plain")
    fw32, fw64 = forward(oracle32, tile, False), forward(oracle64, tile, False)
    assert np.array_equal(fw32["bin"].sortedIdx, fw64["bin"].sortedIdx)
    apart = int((fw32["last"] != fw64["last"]).sum())
    A32, S32 = rule(fw32, tile, "plain")
    for col in range(2):
        ea, es = _maxnorm(A32[:, col], A64[:, col]), _maxnorm(S32[:, col], S64[:, col])
        print(f"column {col}: float32 inputs move A by {ea:.3e}, S by {es:.3e} (bar 1e-4); {apart} pixels stop apart")
        assert ea <= 1e-4 and es <= 1e-4


def test_rule_wants_outputs_with_their_cotangents(oracle64):
    fw = forward(oracle64, (16, 16), False)
    bn = fw["bin"]
    cot = cotangents("plain")[0]
    for kw in (dict(cotDepth=np.zeros((H, W))), dict(outDepth=fw["depth"]), dict(cotAlpha=np.zeros((H, W))),
               dict(outAlpha=fw["alpha"])):
        with pytest.raises(ValueError):
            ag.blend_absgrad(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, 16, 16, cot, fw["color"], fw["last"], **kw)


def test_hand_built_pair_cancels_in_the_signed_sum_only():
    """One isotropic splat at the centre of a 16 x 16 tile under a constant cotangent: g_x is odd in dx, the pixels left and
    right of the mean pull against each other, S_x = 0 and A_x is the sum of the magnitudes."""
    w = h = 16
    packed = np.zeros((1, 11))
    packed[0, 0:2] = 7.5
    packed[0, 2] = packed[0, 5] = 0.05
    packed[0, 6:9] = (1.0, 0.5, 0.25)
    packed[0, 9] = 0.6
    packed[0, 10] = 1.0
    xs = np.arange(w) - 7.5
    cot = np.zeros((h, w, 3))
    cot[..., 0] = 1.0                     # dL/dalpha = cot . colour = 1 everywhere: h = raw > 0, g_x = h c00 dx is odd in dx
    dx, dy = np.meshgrid(xs, xs, indexing="xy")
    raw = 0.6 * np.exp(-0.5 * 0.05 * (dx * dx + dy * dy))
    out = (raw[..., None] * packed[0, 6:9]).reshape(h, w, 3)      # the forward: one entry, T = 1
    last = np.ones((h, w), np.uint32)
    A, S = ag.blend_absgrad(packed, np.zeros(1, np.uint32), np.array([[0, 1]], np.uint32), w, h, 16, 16, cot, out, last)
    # dalpha = T S_i - (K - R) / (1 - alpha) with K = R: dalpha = S_i = 1
    gx, gy = raw * 0.05 * dx, raw * 0.05 * dy
    assert abs(S[0, 0]) <= 1e-12 and abs(S[0, 1]) <= 1e-12
    assert abs(A[0, 0] - np.abs(gx).sum()) <= 1e-12 and abs(A[0, 1] - np.abs(gy).sum()) <= 1e-12
    assert A[0, 0] > 1.0
    # an entry at or past the pixel's stop, and one with raw > 0.99, add nothing
    A0, _ = ag.blend_absgrad(packed, np.zeros(1, np.uint32), np.array([[0, 1]], np.uint32), w, h, 16, 16, cot, out,
                             np.zeros((h, w), np.uint32))
    assert not A0.any()
    hot = packed.copy()
    hot[0, 9] = 1.0
    hot[0, 2] = hot[0, 5] = 1e-12          # raw = 1 > 0.99 at every pixel
    A1, S1 = ag.blend_absgrad(hot, np.zeros(1, np.uint32), np.array([[0, 1]], np.uint32), w, h, 16, 16, cot, out, last)
    assert not A1.any() and not S1.any()


# ----------------------------------------------------------------------------------------------------------- the statistic
def test_statistic_on_a_hand_made_input():
    A = np.array([[0.0, 0.0], [3.0 / 80, 4.0 / 60], [1.0, 0.0], [0.0, 2.0]])
    got = ag.absgrad_statistic(A, 160, 120)
    assert got.shape == (4,)
    assert np.allclose(got, [0.0, 5.0, 80.0, 120.0], rtol=1e-15, atol=0)
    assert ag.absgrad_statistic(np.float32([[0.5, 0.25]]), 4, 8)[0] == pytest.approx(np.hypot(1.0, 1.0))


# ----------------------------------------------------------------------------------------------------------- the settings
def test_config_defaults():
    c = ag.AbsGradConfig().validate()
    assert c.threshold == 0.0008
    assert ag.AbsGradConfig(threshold=0.002).validate().threshold == 0.002
    assert ag.AbsGradConfig(threshold=1).validate()


@pytest.mark.parametrize("t", [0.0, -0.1, float("nan"), float("inf"), None, True, "0.0008"])
def test_config_refuses(t):
    with pytest.raises(ValueError):
        ag.AbsGradConfig(threshold=t).validate()


@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(strategy="mcmc"), dict(densify=False),
                                dict(absgrad=dict(threshold=0.0008)), dict(absgrad=True),
                                dict(absgrad=ag.AbsGradConfig(threshold=0.0))])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(absgrad=ag.AbsGradConfig())
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
    assert "hypot(W/2 Ax, H/2 Ay)" in src        # the header states the statistic


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_set_absgrad(None, 1) == 1
    assert lib.gs_get_absgrad(None, 0, None) == 1
