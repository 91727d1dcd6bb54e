"""The depth distortion loss without a device (gaussiansplattingmlx_amd/distortion.py, include/gsplat.h gs_blend_distortion ..,
DESIGN.md section 37): the float64 numpy statement against the brute-force pair sum on the oracle's own tile lists, its VJP
against central differences, the float32 forms on thin distributions, and the host surface (declarations, binding, settings,
the trainer's refusals).

Bars.
  Brute force      1e-12 relative, per pixel: two float64 evaluations of one polynomial in the weights and depths, the Welford
                   sweep (which cancels nothing) against n^2 / 2 products summed pairwise.
  Central          1e-6 of the column's largest gradient entry: float64 central differences with a step of 1e-6 of the column's
  differences      scale carry a truncation error of step^2 f''' / 6 and a rounding error of 1e-16 |L| / step, both below 1e-8
                   of the entries on this scene; the scene keeps every pixel away from a stop (T > 1e-3) and the clamp
                   (raw <= 0.8), asserted, so the statement is smooth there.
  Thin             lists of n = 8 entries with depths spread 1e-4 relative around one value.  The float32 Welford form (on
  distributions    m - c, as the kernels) against the float64 statement: S is a sum of n non-negative terms, each with four
                   roundings of half an ulp and the running mean's own, amplified by sqrt(1 + mu_e^2 / sigma^2) <= 3 (mu_e the
                   mean of the deviations from the first entry): (n + 4) x 3 / 2 = 18 ulps of A S at the very most -- "a few".
                   A M2 - M1^2 in float32 must miss that by orders of magnitude on every one of the cases: asserted > 1e4 ulps.
"""
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import distortion as ds
from gaussiansplattingmlx_amd import features as ft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = ("gs_blend_distortion", "gs_blend_distortion_backward", "gs_render_distortion", "gs_render_distortion_backward",
           "gs_distortion_loss", "gs_arm_distortion")
MAP_KW = {"ndc": dict(map="ndc", near=0.2, far=1000.0), "linear": dict(map="linear")}


def _load(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dsc_" + name, os.path.join(HERE, name + ".py"))
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


def brute_force(lists, weights, **map_kw):
    """D [H, W] as the double sum over the pairs i < j of a pixel's entries, from features.tile_weights' weights."""
    packed, W, H = np.asarray(lists[0], np.float64), lists[3], lists[4]
    m_all = ds.map_depth(packed[:, 10], dtype=np.float64, **map_kw)[0]
    D = np.zeros((H, W))
    for ys, xs, g, w in weights:
        m = m_all[g]
        d2 = (m[:, None] - m[None, :]) ** 2
        iu = np.triu_indices(g.size, 1)
        D[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = np.einsum("kyx,kyx,k->yx", w[iu[0]], w[iu[1]], d2[iu])
    return D


# ------------------------------------------------------------------------------------------------------------ 1. brute force
@pytest.mark.parametrize("mapname", list(MAP_KW))
@pytest.mark.parametrize("W,H,tile,N", CASES)
def test_statement_is_the_pair_sum(oracle64, W, H, tile, N, mapname):
    s, bn, lists, weights = _case(oracle64, W, H, tile, N)
    D, totals = ds.tile_distortion(*lists, **MAP_KW[mapname])
    want = brute_force(lists, weights, **MAP_KW[mapname])
    assert D.shape == (H, W) and totals.shape == (H, W, 3) and D.dtype == np.float64
    err = np.abs(D - want)
    print(f"{mapname}: max D {want.max():.4e}, worst relative distance {np.max(err / np.maximum(want, 1e-300)):.3e}")
    assert want.max() > 1e-3 and (err <= 1e-12 * want).all()
    # the totals are what they are called: A the alpha image, mu the weighted mean, and D = A S
    A = sum(np.pad(w.sum(axis=0), ((ys[0], H - 1 - ys[-1]), (xs[0], W - 1 - xs[-1]))) for ys, xs, g, w in weights)
    assert np.abs(totals[..., 0] - A).max() <= 1e-12
    assert np.array_equal(D, totals[..., 0] * totals[..., 2]) and (totals[..., 2] >= 0).all()


# ---------------------------------------------------------------------------------------------------- 2. central differences
def smooth_scene(W=32, H=32, N=8, seed=3):
    """Eight broad splats over a 32 x 32 image: opacities <= 0.5, so T >= 0.5^8 = 3.9e-3 everywhere and raw <= 0.5."""
    rng = np.random.default_rng(seed)
    packed = np.zeros((N, 11))
    packed[:, 0], packed[:, 1] = rng.uniform(4, W - 4, N), rng.uniform(4, H - 4, N)
    sx, sy, rho = rng.uniform(3, 7, N), rng.uniform(3, 7, N), rng.uniform(-0.5, 0.5, N)
    det = (sx * sy) ** 2 * (1 - rho ** 2)
    packed[:, 2], packed[:, 5] = sy ** 2 / det, sx ** 2 / det
    packed[:, 3] = packed[:, 4] = -rho * sx * sy / det
    packed[:, 6:9] = rng.uniform(0, 1, (N, 3))
    packed[:, 9] = rng.uniform(0.1, 0.5, N)
    packed[:, 10] = rng.uniform(1.0, 6.0, N)
    rad = 3.0 * np.maximum(sx, sy)
    return packed, packed[:, 0:2] - rad[:, None], packed[:, 0:2] + rad[:, None], rad


@pytest.mark.parametrize("mapname", list(MAP_KW))
def test_vjp_agrees_with_central_differences(oracle64, mapname):
    W = H = 32
    packed, rmin, rmax, rad = smooth_scene(W, H)
    bn = oracle64.tile_bin(rmin, rmax, rad, packed[:, 10], W, H, 16, 16)
    lists = (bn.sortedIdx, bn.tileRanges, W, H, 16, 16)
    # no pixel near a stop or the clamp: the statement is smooth
    T_final = 1.0 - sum(np.pad(w.sum(axis=0), ((ys[0], H - 1 - ys[-1]), (xs[0], W - 1 - xs[-1])))
                        for ys, xs, g, w in ft.tile_weights(packed, *lists))
    assert packed[:, 9].max() <= 0.8 and T_final.min() > 1e-3 and T_final.max() < 0.999
    kw = MAP_KW[mapname]
    cot = np.random.default_rng(9).uniform(-1, 1, (H, W))
    rows = ds.tile_distortion_vjp(packed, *lists, cot, **kw)
    assert rows.shape == (8, 11) and not rows[:, 6:9].any()

    def L(p):
        return (cot * ds.tile_distortion(p, *lists, **kw)[0]).sum()
    for col in ds.GRAD_COLUMNS:
        h = 1e-6 * np.abs(packed[:, col]).max()
        num = np.zeros(8)
        for g in range(8):
            lo, hi = packed.copy(), packed.copy()
            lo[g, col] -= h
            hi[g, col] += h
            num[g] = (L(hi) - L(lo)) / (2 * h)
        err = np.abs(rows[:, col] - num).max() / np.abs(num).max()
        print(f"{mapname} column {col}: max |grad| {np.abs(num).max():.4e}, distance {err:.3e}")
        assert np.abs(num).max() > 0 and err <= 1e-6


def test_float32_statement_follows_the_float64_one(oracle64):
    """The dtype=np.float32 forms (the kernels' operation order) stay near the float64 ones on an ordinary scene."""
    W, H, tile, N = CASES[0]
    s, bn, lists, _ = _case(oracle64, W, H, tile, N)
    D64, t64 = ds.tile_distortion(*lists)
    D32, t32 = ds.tile_distortion(*lists, dtype=np.float32)
    assert D32.dtype == np.float32 and np.abs(D32 - D64).max() <= 1e-5 * D64.max()
    cot = np.random.default_rng(2).uniform(-1, 1, (H, W))
    r64 = ds.tile_distortion_vjp(*lists, cot, totals=t64)
    r32 = ds.tile_distortion_vjp(*lists, cot, dtype=np.float32, totals=t32)
    for col in ds.GRAD_COLUMNS:
        assert np.abs(r32[:, col] - r64[:, col]).max() <= 1e-3 * np.abs(r64[:, col]).max(), col
    for what in ("occluded", "offscreen"):
        assert not r64[s[what]].any() and not r32[s[what]].any()
    # a pixel the loss does not see gives nothing: a zero cotangent, exact zeros
    assert not ds.tile_distortion_vjp(*lists, np.zeros((H, W)), totals=t64).any()


# ------------------------------------------------------------------------------------------------------ 3. thin distributions
def test_welford_keeps_thin_distributions_and_the_moments_form_does_not():
    n, bar = 8, (8 + 4) * 3 / 2
    rng = np.random.default_rng(0)
    worst_w = worst_plain = 0.0
    best_m = np.inf
    for centre in (0.97, 5.0, 40.0):
        for _ in range(40):
            alpha = rng.uniform(0.05, 0.5, n)
            w = (np.concatenate([[1.0], np.cumprod(1 - alpha)[:-1]]) * alpha).astype(np.float32)
            m = (centre * (1 + 1e-4 * rng.uniform(-1, 1, n))).astype(np.float32)
            A, _, S = ds.welford_form(w, m, np.float64)
            D64 = A * S
            w64, m64 = w.astype(np.float64), m.astype(np.float64)
            brute = 0.5 * (w64[:, None] * w64[None, :] * (m64[:, None] - m64[None, :]) ** 2).sum()
            assert abs(D64 - brute) <= 1e-12 * brute
            ulp = float(np.spacing(np.float32(D64)))
            A32, _, S32 = ds.welford_form(w, m, np.float32)
            Ap, _, Sp = ds.welford_form(w, m, np.float32, shift=False)
            worst_w = max(worst_w, abs(float(np.float32(A32 * S32)) - D64) / ulp)
            worst_plain = max(worst_plain, abs(float(np.float32(Ap * Sp)) - D64) / ulp)
            best_m = min(best_m, abs(float(ds.moments_form(w, m, np.float32)) - D64) / ulp)
    print(f"ulps of A S from float64: Welford on m - c at most {worst_w:.1f} (bar {bar:.0f}), Welford on m itself at most "
          f"{worst_plain:.0f}, A M2 - M1^2 at least {best_m:.3g}")
    assert worst_w <= bar
    assert best_m > 1e4


# ------------------------------------------------------------------------------------------------------------ 4. host surface
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "#define GSPLAT_ABI_VERSION 6" in src
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
    assert re.search(r"typedef struct gs_distortion_params\s*\{\s*int map;\s*float near, far;\s*\}", plain)
    assert [n for n, _ in _lib.gs_distortion_params._fields_] == ["map", "near", "far"]
    assert (_lib.GS_DISTORTION_NDC, _lib.GS_DISTORTION_LINEAR) == (0, 1) == tuple(ds.MAPS.index(m) for m in ("ndc", "linear"))
    assert re.search(r"GS_DISTORTION_NDC\s*=\s*0\s*,\s*GS_DISTORTION_LINEAR\s*=\s*1", plain)
    assert "distortion.hip" in __import__("gaussiansplattingmlx_amd.build", fromlist=["SOURCES"]).SOURCES
    # every entry point's comment says what it is
    for e in ("gs_blend_distortion", "gs_render_distortion", "gs_distortion_loss", "gs_arm_distortion"):
        comment = src[:src.index("int " + e + "(")].rsplit("/*", 1)[1]
        assert "2DGS" in comment and "distloss" in comment, e
    assert "Columns 12 and 13" in src


def test_null_context_is_refused():
    import ctypes
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    p = _lib.gs_distortion_params(0, 0.2, 1000.0)
    assert lib.gs_blend_distortion(None, 0, None, ctypes.byref(p), None, None) == 1
    assert lib.gs_blend_distortion_backward(None, 0, None, ctypes.byref(p), None, None, None) == 1
    assert lib.gs_render_distortion(None, ctypes.byref(p), None, None) == 1
    assert lib.gs_render_distortion_backward(None, ctypes.byref(p), None, None, None) == 1
    assert lib.gs_distortion_loss(None, ctypes.c_float(1.0), 0, None, None, None, None) == 1
    assert lib.gs_arm_distortion(None, None, None, None) == 1


def test_config_defaults_and_validation():
    c = ds.DistortionConfig().validate()
    assert (c.weight, c.start, c.map, c.near, c.far) == (100.0, 3000, "ndc", 0.2, 1000.0)
    p = c.params()
    assert p.map == 0 and p.near == np.float32(0.2) and p.far == 1000.0
    assert ds.DistortionConfig(weight=0.0, start=0, map="linear").validate().params().map == 1


@pytest.mark.parametrize("kw", [dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=None),
                                dict(weight=True), dict(start=-1), dict(start=2.5), dict(start=True), dict(map="log"),
                                dict(map=0), dict(near=0.0), dict(near=-0.2), dict(near=5.0, far=5.0), dict(far=float("inf")),
                                dict(near=float("nan")), dict(far=None)])
def test_config_refuses(kw):
    with pytest.raises(ValueError):
        ds.DistortionConfig(**kw).validate()


@pytest.mark.parametrize("kw,match", [(dict(views_per_rank=2), "one view per step"),
                                      (dict(process_group=object()), "single-device steps only"),
                                      (dict(exchange_impl="native"), "single-device steps only"),
                                      (dict(dp_bootstrap=(b"", 0, 1)), "single-device steps only"),
                                      (dict(distortion=dict(weight=1.0)), "a DistortionConfig"),
                                      (dict(distortion=ds.DistortionConfig(map="log")), "map")])
def test_trainer_refuses(kw, match):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(distortion=ds.DistortionConfig())
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_train_step_refuses_a_fisheye_camera():
    from gaussiansplattingmlx_amd.camera import Camera
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)         # (the checks come before anything else of the trainer is touched)
    tr.background = tr.depth = tr.normal = tr.pg = None
    tr.pose_opt = tr.filter_3d = False
    tr.exchange_impl, tr.viewsPerRank = "torch", 1
    tr.distortion = ds.DistortionConfig()
    with pytest.raises(ValueError, match="distortion= takes pinhole cameras only"):
        tr.trainStep(Camera(8, 6, 7.0, 7.0, np.eye(4), model="fisheye"), None)


def test_loss_statement():
    D = np.arange(12, dtype=np.float64).reshape(3, 4)
    L, cot = ds.loss_and_cotangent(D, 2.0)
    assert L == pytest.approx(2.0 * D.mean()) and np.allclose(cot, 2.0 / 12)
    mask = np.zeros((3, 4), np.uint8)
    mask[1] = 255
    mask[2, 0] = 51
    L, cot = ds.loss_and_cotangent(D, 2.0, mask)
    assert L == pytest.approx(2.0 * (D[1].sum() + 0.2 * D[2, 0]) / 12) and cot[0, 0] == 0 and cot[1, 1] == pytest.approx(2.0 / 12)
