"""Adaptive density control without a device (gaussiansplattingmlx_amd/adc.py, include/gsplat.h gs_set_adc_stats, DESIGN.md
section 26): the numpy restatement of the kernels (tests/adc_numpy.py) on hand-built inputs -- the decision table with every
branch and priority, the split children's distribution, the revised opacity, the reset --, scene_extent, the settings'
validation, the model's staging of the moments, the trainer's refusals and the entry points' declaration.

Bars.  Split children: n draws of z ~ N(0, I) through the float64 gather give deviations d = R diag(s) z with covariance
Sigma = R diag(s^2) R^T; with the mean known, the sample moment S_ij = mean(d_i d_j) has variance (Sigma_ii Sigma_jj +
Sigma_ij^2) / n (Isserlis), and the bar is six of those standard deviations per entry (n = 200 000: 1.3 % to 1.9 % of the entry's
scale; printed).  Revised opacity: 1 - (1 - alpha')^2 = alpha to 1e-12 relative in float64 (the form has no cancellation).
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import adc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("gs_set_adc_stats", "gs_adc_accumulate", "gs_adc_classify", "gs_adc_gather", "gs_adc_gather_moments",
           "gs_adc_reset_opacity")
DTYPES = (np.float32, np.float64)


def _load(name):
    spec = importlib.util.spec_from_file_location("_adc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


az = _load("adc_numpy")
K, S, C, P = az.KEEP, az.SPLIT, az.CLONE, az.PRUNE


# ------------------------------------------------------------------------------------------------------ the statistic
@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_on_a_hand_made_input(dtype):
    rows = np.zeros((4, 16), np.float32)
    rows[0, 0:2] = (3.0 / 80, 4.0 / 60)                # hypot(80 x, 60 y) = 5
    rows[1, 0:2] = (1.0, 1.0)                          # radius 0: nothing moves
    rows[2, 0:2], rows[2, 12:14] = (1.0, 0.0), (0.0, 2.0)
    rows[3, 0:2] = (1e-25, 1e-25)
    radii = np.float32([6.0, 0.0, 9.0, 3.0])
    acc = np.float32([[1.0, 2.0, 3.0, 0.0], [7.0, 8.0, 9.0, 0.0], [3.0, 99.0, 12.0, 0.0]])
    g, n, mr = az.accumulate(rows, radii, False, 160, 120, *acc, dtype=dtype)
    assert g.dtype == dtype
    assert np.allclose(g[:3], [6.0, 2.0, 83.0], rtol=1e-6) and np.array_equal(n, [8.0, 8.0, 10.0, 1.0])
    assert np.array_equal(mr, [6.0, 99.0, 12.0, 3.0])
    assert g[3] > 0 and abs(g[3] / np.hypot(80e-25, 60e-25) - 1) < 1e-6          # the squares underflow in float32; hypot does not
    g2, n2, _ = az.accumulate(rows, radii, True, 160, 120, g, n, mr, dtype=dtype)      # the absolute columns; a second call adds
    assert np.allclose(g2[:3], [6.0, 2.0, 83.0 + 120.0], rtol=1e-6) and np.array_equal(n2, [9.0, 8.0, 11.0, 2.0])


# ------------------------------------------------------------------------------------------------------- the decision
def _table():
    """Hand-built rows under the default thresholds at extent 4: grad 2e-4, dense 0.04, world 0.4, opacity 0.005, screen 20."""
    lo, hi = -8.0, 2.0                                  # raw opacities: sigmoid 3.4e-4 and 0.88
    small, mid, huge = np.log(0.01), np.log(0.1), np.log(0.5)
    thr = np.float32(0.0002)
    rows = [
        # gradSum, count, maxRadius, log scale, raw opacity
        (1.0, 4.0, 5.0, small, lo),                     # 0 transparent AND over the gradient threshold
        (1.0, 4.0, 5.0, small, hi),                     # 1 over the threshold, small
        (1.0, 4.0, 5.0, mid, hi),                       # 2 over the threshold, above percent_dense x extent
        (1.0, 4.0, 30.0, huge, hi),                     # 3 over the threshold AND over both size bounds
        (0.0, 4.0, 30.0, small, hi),                    # 4 below the threshold, over the screen size
        (0.0, 4.0, 5.0, huge, hi),                      # 5 below the threshold, over the world size
        (0.0, 4.0, 5.0, small, hi),                     # 6 nothing applies
        (1e6, 0.0, 5.0, small, hi),                     # 7 never seen: the average is 0 whatever the sum holds
        (float(thr * np.float32(4.0)), 4.0, 5.0, small, hi),      # 8 the average IS the threshold (>=)
        (0.0, 4.0, 20.0, small, hi),                    # 9 the radius IS the screen size (>)
        (0.0, 0.0, 0.0, small, lo),                     # 10 transparent and never seen
    ]
    a = np.float32(rows)
    return a[:, 0], a[:, 1], a[:, 2], np.repeat(a[:, 3:4], 3, axis=1), a[:, 4]


@pytest.mark.parametrize("dtype", DTYPES)
def test_decision_table(dtype):
    g, n, mr, sc, op = _table()
    run = lambda allow, size, **kw: az.classify(g, n, mr, sc, op, dict(az.DEFAULTS, **kw), allow, size, dtype)      # noqa: E731
    a, c = run(True, True)
    assert list(a) == [P, C, S, S, P, P, K, K, C, K, P]         # opacity beats gradient; gradient beats size
    assert list(c) == [0, 2, 2, 2, 0, 0, 1, 1, 2, 1, 0]
    a, _ = run(True, False)                                     # sizePrune off
    assert list(a) == [P, C, S, S, K, K, K, K, C, K, P]
    a, _ = run(False, True)                                     # allowDensify off: what would have grown falls through to the size test
    assert list(a) == [P, K, K, P, P, P, K, K, K, K, P]
    a, _ = run(False, False)
    assert list(a) == [P, K, K, K, K, K, K, K, K, K, P]
    a, _ = run(True, True, max_screen_size=0.0)                 # no screen test; the world test stays
    assert list(a) == [P, C, S, S, K, P, K, K, C, K, P]
    a, _ = run(True, True, max_screen_size=-1.0)
    assert list(a) == [P, C, S, S, K, P, K, K, C, K, P]
    # the largest of the three scales decides, whichever column holds it
    sc2 = sc.copy()
    sc2[1] = (np.log(0.01), np.log(0.01), np.log(0.1))
    assert az.classify(g, n, mr, sc2, op, az.DEFAULTS, True, False, dtype)[0][1] == S


def test_shared_classify_inputs_reach_every_action_away_from_the_thresholds():
    for screen in (20.0, 0.0):
        prm = dict(az.DEFAULTS, max_screen_size=screen)
        inp = az.classify_inputs(prm)
        assert not az.near_threshold(*inp, prm).any()
        for allow in (True, False):
            for size in (True, False):
                a32, c32 = az.classify(*inp, prm, allow, size, np.float32)
                a64, c64 = az.classify(*inp, prm, allow, size, np.float64)
                assert np.array_equal(a32, a64) and np.array_equal(c32, c64)
                have = set(np.unique(a32))
                assert have == ({K, S, C, P} if allow else {K, P})
        assert (inp[1] == 0).sum() > 50


# --------------------------------------------------------------------------------------------------------- the gather
def test_split_children_are_samples_of_the_gaussian():
    n = 200_000
    rng = np.random.default_rng(41)
    q = np.float32([[0.9, -2.0, 0.7, 1.6]])                       # unnormalised on purpose
    s = np.float32([[np.log(0.3), np.log(0.05), np.log(0.12)]])
    p = dict(xyz=np.float32([[0.5, -1.0, 2.0]]), features_dc=np.zeros((1, 1, 3), np.float32),
             features_rest=np.zeros((1, 3, 3), np.float32), scales=s, rotation=q, opacity=np.float32([0.3]))
    mode = np.tile(np.int32([1, 2]), n // 2)
    out = az.gather(p, np.zeros(n, np.int32), mode, rng.standard_normal((n, 3)).astype(np.float32))
    d = out["xyz"] - p["xyz"].astype(np.float64)
    R = az.rotation_matrices(q)[0]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12
    Sigma = R @ np.diag(np.exp(s[0].astype(np.float64)) ** 2) @ R.T
    Sm = d.T @ d / n
    bar = 6.0 * np.sqrt((np.outer(np.diag(Sigma), np.diag(Sigma)) + Sigma ** 2) / n)
    print("sample covariance against R diag(s^2) R^T, in units of the six-sigma bar:\n", np.abs(Sm - Sigma) / bar)
    assert (np.abs(Sm - Sigma) <= bar).all()
    for half in (d[0::2], d[1::2]):                               # each child is its own draw: neither mirrors the other
        assert np.abs(half.mean(axis=0)).max() <= 6.0 * np.sqrt(np.diag(Sigma).max() / (n / 2))
    assert abs(np.corrcoef(d[0::2, 0], d[1::2, 0])[0, 1]) < 6.0 / np.sqrt(n / 2)
    assert np.allclose(out["scales"], s.astype(np.float64) + np.float64(az.SCALE_REDUCTION), rtol=0, atol=0)
    assert np.array_equal(out["rotation"], np.repeat(q.astype(np.float64), n, 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_clones_and_kept_rows_are_exact_copies(dtype):
    p = az.gather_params(64, 4)
    act = az.gather_actions(64)
    dz = _load("densify_numpy")
    off, st = dz.offsets(act)
    g, m = dz.output_map(act, off, st["total"])
    noise = np.random.default_rng(3).standard_normal((st["total"], 3)).astype(np.float32)
    out = az.gather(p, g, m, noise, dtype=dtype)
    same = (m == 0) | (m == 3)
    assert same.any() and (m == 3).any() and (~same).any()
    for k in az.PARAMS:
        assert np.array_equal(out[k][same].astype(np.float32), p[k][g][same]), k
    assert not np.array_equal(out["xyz"][~same].astype(np.float32), p["xyz"][g][~same])
    for k in ("features_dc", "features_rest", "rotation", "opacity"):
        assert np.array_equal(out[k].astype(np.float32), p[k][g]), k


def test_revised_opacity_identity():
    o = np.linspace(-12.0, 12.0, 97).astype(np.float32)
    raw = az.revised_opacity(o, np.float64)
    a = 1 / (1 + np.exp(-o.astype(np.float64)))
    a_new = 1 / (1 + np.exp(-raw))
    # 1 - (1 - x)^2 = x (2 - x): the left form would lose 1 / x of float64's digits to its own subtraction at x ~ 3e-6
    assert np.abs(a_new * (2 - a_new) / a - 1).max() <= 1e-12
    assert (a_new < a).all() and (a_new > 0.5 * a).all()         # two layers of alpha' composite to one of alpha
    r32 = az.revised_opacity(o, np.float32)
    assert r32.dtype == np.float32 and np.abs(r32 - raw).max() <= 1e-5 * np.abs(raw).max()
    # through the gather: split children and BOTH rows of a clone, nothing else
    p = az.gather_params(8, 4)
    act = np.int32([K, S, C, P, K, C, S, K])
    dz = _load("densify_numpy")
    off, st = dz.offsets(act)
    g, m = dz.output_map(act, off, st["total"])
    noise = np.zeros((st["total"], 3), np.float32)
    on, offp = az.gather(p, g, m, noise, revised=True), az.gather(p, g, m, noise, revised=False)
    changed = on["opacity"] != offp["opacity"]
    assert np.array_equal(changed, np.isin(act[g], (S, C)))
    assert np.allclose(on["opacity"][changed], az.revised_opacity(p["opacity"][g][changed]), rtol=0, atol=0)


def test_moments_survive_where_the_gaussian_does():
    p = az.gather_params(40, 4)
    act = az.gather_actions(40)
    dz = _load("densify_numpy")
    off, st = dz.offsets(act)
    g, m = dz.output_map(act, off, st["total"])
    out = az.gather_moments(p, g, m, act)
    kept = (m == 0) & (act[g] != S)
    assert kept.any() and (~kept).any()
    for k in az.PARAMS:
        assert np.array_equal(out[k][kept], p[k][g][kept]) and not out[k][~kept].any(), k
    assert not kept[m == 3].any() and kept[(m == 0) & (act[g] == C)].all()


# ---------------------------------------------------------------------------------------------------------- the reset
def test_reset_is_idempotent_and_never_raises_an_opacity():
    cap = az.reset_raw(0.01)
    assert abs(1 / (1 + np.exp(-np.float64(cap))) - 0.01) < 1e-8
    o = np.float32([-20.0, np.nextafter(cap, np.float32(-np.inf)), cap, np.nextafter(cap, np.float32(np.inf)), 0.0, 9.0, np.inf])
    m, v = np.ones(7, np.float32), np.full(7, 2.0, np.float32)
    o1, m1, v1 = az.reset_opacity(o, m, v, 0.01)
    assert (o1 <= o).all() and (o1 <= cap).all() and np.array_equal(o1[:3], o[:3]) and (o1[3:] == cap).all()
    assert not m1.any() and not v1.any()
    o2, _, _ = az.reset_opacity(o1, m1, v1, 0.01)
    assert np.array_equal(o2, o1)


# ------------------------------------------------------------------------------------------------------- scene_extent
def test_scene_extent_on_a_hand_built_rig():
    centres = np.array([[3.0, 0, 0], [-3.0, 0, 0], [0, 4.0, 0], [0, -4.0, 0]])        # mean 0, farthest 4
    assert adc.scene_extent(centres) == pytest.approx(4.4, rel=1e-15)
    assert adc.scene_extent(centres + [10.0, -7.0, 2.0]) == pytest.approx(4.4, rel=1e-12)      # translation invariant

    class Cam:
        def __init__(self, c):
            self.cameraCenter = np.float32(c)
    assert adc.scene_extent([Cam(c) for c in centres]) == pytest.approx(4.4, rel=1e-6)
    off = np.array([[0.0, 0, 0], [0, 0, 0], [0, 0, 0], [8.0, 0, 0]])                   # mean (2, 0, 0): farthest 6
    assert adc.scene_extent(off) == pytest.approx(6.6, rel=1e-15)
    for bad in ([], np.zeros((3, 3)), [[0.0, 0, 0]], [[np.nan, 0, 0], [1.0, 0, 0]], [[0.0, 1.0], [1.0, 0.0]]):
        with pytest.raises(ValueError):
            adc.scene_extent(bad)


# ------------------------------------------------------------------------------------------------------- the settings
def test_config_defaults():
    c = adc.ADCConfig(scene_extent=4.4).validate()
    assert (c.grad_threshold, c.percent_dense, c.min_opacity, c.max_screen_size, c.prune_world) == (0.0002, 0.01, 0.005, 20.0, 0.1)
    assert (c.densify_from, c.densify_until, c.densify_interval, c.opacity_reset_interval) == (500, 15000, 100, 3000)
    assert c.reset_value == 0.01 and c.revised_opacity is False
    assert adc.ADCConfig(scene_extent=1, max_screen_size=0, revised_opacity=True).validate()
    assert [t for t in range(0, 1300) if c.is_event(t)] == [500, 600, 700, 800, 900, 1000, 1100, 1200]
    assert not c.is_event(15100) and c.is_event(15000)
    assert [t for t in range(0, 16000) if c.is_reset(t)] == [3000, 6000, 9000, 12000, 15000]


@pytest.mark.parametrize("kw", [dict(), dict(scene_extent=0.0), dict(scene_extent=float("inf")), dict(scene_extent="4"),
                                dict(grad_threshold=0.0), dict(grad_threshold=float("nan")), dict(percent_dense=-1.0),
                                dict(min_opacity=0.0), dict(min_opacity=1.0), dict(min_opacity=True),
                                dict(max_screen_size=float("nan")), dict(max_screen_size=None), dict(prune_world=0.0),
                                dict(densify_from=-1), dict(densify_from=1.5), dict(densify_until=100, densify_from=200),
                                dict(densify_interval=0), dict(opacity_reset_interval=0), dict(opacity_reset_interval=True),
                                dict(reset_value=0.0), dict(reset_value=1.0), dict(revised_opacity=1)])
def test_config_refuses(kw):
    args = dict(scene_extent=4.4)
    if not kw:
        args = {}
    args.update(kw)
    with pytest.raises(ValueError):
        adc.ADCConfig(**args).validate()


def _contrib():
    from gaussiansplattingmlx_amd.contrib_prune import ContribPruneConfig
    return ContribPruneConfig(cameras=[object()])


@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(filter_3d=True, filter_cameras=[object()]),
                                dict(contrib_prune="config"), dict(sparse_adam=True), dict(adc=None),
                                dict(adc=dict(scene_extent=4.4)), dict(adc=adc.ADCConfig()),
                                dict(adc=adc.ADCConfig(scene_extent=4.4, reset_value=2.0)), dict(strategy="reference"),
                                dict(strategy="mcmc"), dict(mcmc=object())])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(strategy="adc", adc=adc.ADCConfig(scene_extent=4.4))
    args.update(kw)
    if args.get("contrib_prune") == "config":
        args["contrib_prune"] = _contrib()
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_reference_param_reload_is_refused():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)
    tr.mcmc, tr.adc, tr.strategy = None, adc.ADCConfig(scene_extent=4.4), "adc"
    with pytest.raises(ValueError):
        tr.referenceParamReload = True
    tr.referenceParamReload = False
    tr.adc, tr.strategy = None, "reference"
    tr.referenceParamReload = True
    assert tr.referenceParamReload


# ------------------------------------------------------------------------------------------------- the model's staging
def test_model_stages_and_commits_the_moments():
    import torch
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER, GaussModel
    p = az.gather_params(5, 4)
    model = GaussModel(p, "cpu")
    model.m.copy_(torch.arange(model.numel, dtype=torch.float32) + 1)
    model.v.copy_(-(torch.arange(model.numel, dtype=torch.float32) + 1))
    model.grad.fill_(3.0)
    out = model.stagingViews(7)
    sm, sv = model.stagingMoments()
    for k in ARENA_ORDER:
        out[k].fill_(0.25)
        sm[k].fill_(5.0)
        sv[k].fill_(6.0)
    model.commitStaged(zero=False, moments=True)
    assert model.N == 7
    mo, vo = model.getMoments()
    for k in ARENA_ORDER:
        assert mo[k].shape[0] == 7 and bool((mo[k] == 5.0).all()) and bool((vo[k] == 6.0).all())
        assert bool((model.getParams()[k] == 0.25).all())
    assert not bool(model.grad.any())
    rows = sum(int(np.prod(mo[k].shape)) for k in ARENA_ORDER)
    assert float(model.m.sum()) == 5.0 * rows and float(model.v.sum()) == 6.0 * rows        # the pads are zero
    # the event of the other strategies: the moments are zeroed, as ever
    model.stagingViews(6)
    model.commitStaged()
    assert model.N == 6 and not bool(model.m.any()) and not bool(model.v.any())
    # ... and a second kept-moments event reuses the spare buffers (the old arenas), whose pads must not leak
    model.m.fill_(9.0)
    model.stagingViews(3)
    sm, sv = model.stagingMoments()
    for k in ARENA_ORDER:
        sm[k].fill_(1.0)
        sv[k].fill_(2.0)
    model.commitStaged(zero=False, moments=True)
    rows = sum(int(np.prod(v.shape)) for v in model.getMoments()[0].values())
    assert float(model.m.sum()) == 1.0 * rows and float(model.v.sum()) == 2.0 * rows
    with pytest.raises(ValueError):
        model.stagingViews(4, stride=8)
        model.stagingMoments()


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
    for meth in ("setADCStats", "adcAccumulate", "adcClassify", "adcGather", "adcGatherMoments", "adcResetOpacity"):
        assert callable(getattr(GaussianRenderer, meth))
    body = re.search(r"typedef struct gs_adc_params \{(.*?)\} gs_adc_params;", plain, flags=re.S).group(1)
    assert re.findall(r"float (\w+);", body) == [n for n, _ in _lib.gs_adc_params._fields_]
    assert "GaussianTrainer.swift:343-393" in src and ":858-893" in src
    assert re.search(r"#define GSPLAT_ABI_VERSION 6\b", src)
    from gaussiansplattingmlx_amd import build
    assert "adc.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "adc.hip"))


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_set_adc_stats(None, None, None, None) == 1
    assert lib.gs_adc_accumulate(None, 0, None, None, 0, None, None, None) == 1
    assert lib.gs_adc_classify(None, 0, None, None, None, None, 3, None, None, 1, 0, None, None) == 1
    assert lib.gs_adc_gather(None, 0, 1, *([None] * 9), 0, *([None] * 6)) == 1
    assert lib.gs_adc_gather_moments(None, 0, 1, None, None, None, None, None) == 1
    assert lib.gs_adc_reset_opacity(None, 0, None, None, None, 0.01) == 1
