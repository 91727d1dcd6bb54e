"""AbsGS densification on the device (include/gsplat.h gs_set_absgrad): the absolute sums the ABSGRAD
instantiations of the fused blend backward (csrc/blend_v2.hip) leave per Gaussian, against the float64 rule
(gaussiansplattingmlx_amd/absgrad.py) on the float64 oracle's records and lists; that nothing else of the step moves; the
statistic the accumulator gets (csrc/densify.hip) and the trainer's use of it; the overflow gate; the refusals.

Every case is the scene of tests/test_absgrad_cpu.py (160 x 120, N = 3000, camera 0, tile lists of up to 1521 and 2739 entries)
under that file's cotangents, handed to renderBackward; the float64 results are that file's, computed once.

Bars.  (Ax, Ay) per column: the project's gradient metric max|a - b| / max|b| <= 1e-3 (test_absgrad_cpu.py: float32 records and
stops alone move the float64 rule by 1.5e-6).  The accumulator against hypot(W/2 Ax, H/2 Ay) of the device's own (Ax, Ay):
1e-6 per element (two float32 products, a sum, one correctly rounded square root).  The trainer's accumulator against the
running float32 sum of the per-step statistics: 1e-5 per element over 12 steps.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import absgrad as ag

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
ABS_BAR, GRAD_BAR = 1e-3, 1e-3
W, H, N = 160, 120, 3000


def _load(name):
    spec = importlib.util.spec_from_file_location("_absg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_absgrad_cpu")


def _renderer(tile=(16, 16), white=False, aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, tile, white, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _backward(r, variant, params=None):
    """One fused forward and backward of camera 0 under the variant's cotangents; returns (result, gradients)."""
    p, cams = cpu.scene()
    cot, cd, ca = cpu.cotangents(variant)
    res = r.renderChecked(_dev(p) if params is None else params, cams[0], wantDepth=variant == "depth")
    g = r.renderBackward(_t(cot), _t(cd), _t(ca))
    return res, g


# ------------------------------------------------------------------------------------------ 1. the sums against float64
@pytest.mark.parametrize("tile,variant", [((16, 16), "plain"), ((50, 38), "plain"), ((16, 16), "depth"), ((16, 16), "white"),
                                          ((16, 16), "alpha")])
def test_absolute_sums_match_float64(oracle64, tile, variant):
    A64, S64 = cpu.want(oracle64, tile, variant)
    r = _renderer(tile, white=variant == "white")
    assert r.blockLists == (tile != (16, 16))
    r.setAbsgrad(True)
    _backward(r, variant)
    got = _np(r.absgrad())
    assert got.shape == (N, 2) and got.dtype == np.float32
    for col in range(2):
        err = _rel(got[:, col], A64[:, col])
        print(f"{tile} {variant} column {col}: device against float64 {err:.3e} (bar {ABS_BAR:.0e}), max {A64[:, col].max():.3e}")
        assert err <= ABS_BAR
    # radius 0 or in no tile list: exactly 0.0 (the fused forward's lists are subsets of the oracle's: trimmed rects)
    fw = cpu.forward(oracle64, tile, variant == "white")
    listed = np.zeros(N, bool)
    listed[fw["bin"].sortedIdx] = True
    radius0 = np.asarray(fw["proj"]["radii"]).reshape(-1) <= 0
    assert not listed[radius0].any()
    print(f"{tile} {variant}: {int((~listed).sum())} Gaussians in no list ({int(radius0.sum())} of radius 0), "
          f"{int((A64.sum(axis=1) == 0).sum())} with a zero float64 sum, {int((got.sum(axis=1) == 0).sum())} with a zero device sum")
    assert not got[~listed].any()
    assert (got >= 0).all() and np.isfinite(got).all()


# ------------------------------------------------------------------------------------- 2. nothing else of the step moves
@pytest.mark.parametrize("variant", ["plain", "depth"])
def test_gradients_and_render_are_those_of_absgrad_off(variant):
    r = _renderer()
    res0, g0 = _backward(r, variant)
    img0, alpha0 = res0.render.clone(), res0.alpha.clone()
    g0 = {k: v.clone() for k, v in g0.items()}
    r.setAbsgrad(True)
    res1, g1 = _backward(r, variant)
    assert torch.equal(res1.render, img0) and torch.equal(res1.alpha, alpha0)
    for k in KEYS:
        err = _rel(_np(g1[k]), _np(g0[k]))
        print(f"{variant} {k}: gradient with absgrad on against off {err:.3e} (bar {GRAD_BAR:.0e})")
        assert err <= GRAD_BAR, k
    r.setAbsgrad(False)
    from gaussiansplattingmlx_amd._lib import GsplatError
    with pytest.raises(GsplatError) as e:
        r.absgrad()
    assert e.value.code == 5


# ---------------------------------------------------------------------------------------------------- 3. the accumulator
def test_accumulator_gets_the_absgrad_statistic():
    r = _renderer()
    # the |grad xyz| statistic of the same step
    norm = torch.zeros(N, device="cuda")
    r.setGradNormAccum(norm)
    _, g = _backward(r, "plain")
    want_norm = np.linalg.norm(_np(g["xyz"]).astype(np.float64), axis=1)
    assert _rel(_np(norm), want_norm) <= 1e-6
    # ... and the AbsGS one
    acc = torch.zeros(N, device="cuda")
    r.setGradNormAccum(acc)
    r.setAbsgrad(True)
    _backward(r, "plain")
    A = _np(r.absgrad()).astype(np.float64)
    stat = ag.absgrad_statistic(A, W, H)
    one = _np(acc).astype(np.float64)
    assert (stat > 0).sum() > 2000
    big = stat > 1e-30          # float32 carries 24 bits down to 1.2e-38; below, the same absolute step
    err = np.abs(one - stat)[big] / stat[big]
    print(f"accumulator against hypot(W/2 Ax, H/2 Ay): {err.max():.3e} per element (bar 1e-6); {int((stat > 0).sum() - big.sum())} "
          f"elements below 1e-30")
    assert err.max() <= 1e-6 and np.abs(one - stat)[~big].max() <= 1e-36 and not one[stat == 0].any()
    # the mode matters
    diff = _rel(one / one.max(), _np(norm).astype(np.float64) / float(norm.max()))
    print(f"AbsGS statistic against |grad xyz| of the same step, each over its maximum: {diff:.3e}; "
          f"max {one.max():.3e} against {float(norm.max()):.3e}")
    assert _rel(one, _np(norm)) > 10 * ABS_BAR and diff > 10 * ABS_BAR
    # a second backward adds to it
    _backward(r, "plain")
    two = _np(acc).astype(np.float64)
    stat2 = ag.absgrad_statistic(_np(r.absgrad()).astype(np.float64), W, H)
    err2 = np.abs(two - (one + stat2))[big] / (one + stat2)[big]
    assert err2.max() <= 1e-6
    assert two.sum() > 1.9 * one.sum()
    r.setGradNormAccum(None)


# ------------------------------------------------------------------------------------------------------------ 4. trainer
def test_trainer_accumulates_the_statistic_and_classifies_on_it(oracle32):
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = cpu.scene()
    r = _renderer()
    tp = _dev(perturb(p, 5, 0.1))
    targets = [r.renderChecked(tp, c).render.clone() for c in cams]
    model = GaussModel(p, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, absgrad=ag.AbsGradConfig())
    assert tr.gradientThreshold == 0.0008
    running = np.zeros(N, np.float32)
    for it in range(12):                   # (no densify event: densifyFromIter = 500)
        tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
        A = _np(r.absgrad())
        hw, hh = np.float32(0.5 * W), np.float32(0.5 * H)
        running = running + np.hypot(hw * A[:, 0], hh * A[:, 1], dtype=np.float32)
    assert r._absgrad and model.N == N and tr.denomGradAccumulation == 12
    got = _np(tr.xyzGradAccumulation)
    nz = running > 1e-30        # (float32's normal range, as above)
    err = np.abs(got.astype(np.float64) - running)[nz] / running[nz]
    print(f"xyzGradAccumulation against the running float32 sum of 12 steps: {err.max():.3e} per element (bar 1e-5)")
    assert nz.sum() > 2000 and err.max() <= 1e-5 and np.abs(got - running)[~nz].max() <= 1e-35
    # the event classifies on it: the trainer's own thresholds, the oracle's rule, exactly
    params = {k: _np(v).copy() for k, v in model.getParams().items()}
    want_a, want_c = oracle32.classify_gaussians(got, 12.0, params["scales"], params["opacity"], tr.gradientThreshold, tr.maxScale,
                                                 tr.minOpacity, True)
    got_a, got_c = r.classifyGaussians(tr.xyzGradAccumulation, 12.0, model.getParams()["scales"],
                                       model.getParams()["opacity"].reshape(-1), tr.gradientThreshold, tr.maxScale, tr.minOpacity)
    assert np.array_equal(_np(got_a), want_a) and np.array_equal(_np(got_c), want_c)
    tr.densifyFromIter = 1
    st = tr.split_and_prune(12)
    count = {k: int((want_a == v).sum()) for k, v in (("keep", 0), ("split", 1), ("clone", 2), ("prune", 3))}
    print(f"the event behind step 12: {st}")
    assert {k: st[k] for k in count} == count and st["total"] == int(want_c.sum())
    assert st["split"] + st["clone"] > 0 and st["keep"] > 0          # (the threshold divides this model)
    assert model.N == st["total"] and tr.denomGradAccumulation == 0


# ------------------------------------------------------------------------------------------------------ 5. overflow gate
def test_an_overflowed_step_adds_nothing():
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel
    p, cams = cpu.scene()
    r0 = _renderer()
    r0.renderForward(_dev(p), cams[0])
    r0.sync()
    M = r0.stats()["M"]
    r0.close()
    r = _renderer()
    r.reserve(N, M // 3)                                     # too small on purpose: a reported overflow
    r.setAbsgrad(True)
    acc = torch.full((N,), 0.5, device="cuda")
    r.setGradNormAccum(acc)
    model = GaussModel(p, r.device)
    before = model.arena.clone()
    res = r.renderForward(model.getParams(), cams[0], wantDepth=False)
    try:                                                     # may or may not have seen the flag yet: both are in contract
        _, gc, _ = r.lossForwardBackward(res.render, torch.rand(H, W, 3, device="cuda"), 0.2)
        r.renderBackwardAdam(gc, model.arena, model.m, model.v, [1e-2] * 6)
    except GsplatError as e:
        assert e.code == 3
    with pytest.raises(GsplatError) as ei:
        r.sync()
    assert ei.value.code == 3 and r.stats()["overflow"] == 1
    assert torch.equal(acc, torch.full((N,), 0.5, device="cuda"))
    assert torch.equal(model.arena, before)
    r.setGradNormAccum(None)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(monkeypatch):
    p, cams = cpu.scene()
    out = torch.zeros(N, 2, device="cuda")
    # a context whose fused path is the generic kernels
    monkeypatch.setenv("GSPLAT_BLOCK_LISTS", "0")
    rg = _renderer((50, 38))
    assert not rg.blockLists
    assert rg.lib.gs_set_absgrad(rg.ctx, 1) == 1                                   # GS_ERR_INVALID_ARG
    assert rg.lib.gs_set_absgrad(rg.ctx, 0) == 0
    rg.close()
    monkeypatch.delenv("GSPLAT_BLOCK_LISTS")
    r = _renderer()
    assert r.lib.gs_set_absgrad(r.ctx, 2) == 1
    assert r.lib.gs_get_absgrad(r.ctx, N, out.data_ptr()) == 5                     # GS_ERR_NO_FORWARD: absgrad is off
    r.setAbsgrad(True)
    assert r.lib.gs_get_absgrad(r.ctx, N, out.data_ptr()) == 5                     # ... and no backward has run
    params = _dev(p)
    r.renderChecked(params, cams[0], wantDepth=False)
    assert r.lib.gs_get_absgrad(r.ctx, N, out.data_ptr()) == 5
    cot = _t(cpu.cotangents("plain")[0])
    g = [torch.zeros(N, k, device="cuda") for k in (3, 3, 4, 1)]
    cc = torch.zeros(3 * N + 16, device="cuda")
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 1
    assert not any(bool(t.any()) for t in g)
    r.renderBackward(cot)                                                           # the forward is still usable
    assert r.lib.gs_get_absgrad(r.ctx, N - 1, out.data_ptr()) == 2                 # GS_ERR_SIZE_MISMATCH
    assert r.lib.gs_get_absgrad(r.ctx, N, None) == 1
    assert r.lib.gs_get_absgrad(r.ctx, N, out.data_ptr()) == 0 and bool(out.any())
    r.setAbsgrad(False)
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 0
