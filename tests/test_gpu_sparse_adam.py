"""Sparse Adam on the device (include/gsplat.h gs_set_sparse_adam): the mask the fused forward leaves, one
fused step against the same step with the setting off (csrc/projection.hip, the SPARSE forms of proj_bwd_fused_kernel),
the unfused path and gs_adam_step_visible (csrc/optim.hip, adam_visible_kernel) against the numpy rule
(gaussiansplattingmlx_amd/sparse_adam.py), the trainer, the overflow gate, the refusals, and that off is off.

Scenes, cameras and row orders are those of tests/test_sparse_adam_cpu.py, where both oracles give the visible counts: camera A
sees every Gaussian, camera B 2436 of 3000 (all 46 full waves mixed in the natural order; in the blocked order the invisible
rows come first: four all-invisible workgroups, then wave 8 mixed at 52 / 12).

Bars.  Invisible rows: bit-identical, every element of parameter and both moments.  Visible rows, two device runs against each
other (the blend backward's float atomics are not bit-reproducible from run to run): the share bar of
test_fused_backward_adam_matches_backward_then_adam, mean(|a - b| > 1e-3 max|b|) < 1e-3 per tensor, the parameters compared as
their change over the step.  gs_adam_step_visible against numpy: the bars of test_adam_step_matches_numpy.
"""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import sparse_adam as sa

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
W, H = 160, 120
SHARE_TOL, SHARE = 1e-3, 1e-3


def _load(name):
    spec = importlib.util.spec_from_file_location("_sag_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_sparse_adam_cpu")


def _renderer(K=25, tile=(16, 16), aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(cpu.DEGREE[K], W, H, tile, False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cot():
    """The colour cotangent of test_absgrad_cpu.cotangents("plain")."""
    return torch.as_tensor((np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)).astype(np.float32), device="cuda")


def _ordered(N, K, order, oracle32):
    """(params, cameras, camera B's visibility by the float32 oracle) of scene (N, K) in the row order."""
    p, cams = cpu.scene(N, K)
    vis = cpu.oracle_visible(oracle32, N, K, cams[1])
    assert (int(vis.sum()), int((~vis).sum())) == cpu.TABLE[(N, K)]
    if order == "blocked":
        perm = cpu.blocked_order(vis)
        p = {k: np.ascontiguousarray(v[perm]) for k, v in p.items()}
        vis = vis[perm]
    return p, cams, vis


def _rows(model, name):
    """The six tensors' rows of one of the model's buffers, as numpy copies."""
    return {k: _np(v).copy() for k, v in model._carve(getattr(model, name), model.N, model.stride).items()}


def _state(model):
    return {name: _rows(model, name) for name in ("arena", "m", "v")}


def _share(a, b):
    return float(np.mean(np.abs(a - b) > SHARE_TOL * np.abs(b).max())) if b.size else 0.0


def _assert_invisible_untouched(after, before, vis, what):
    for name in ("arena", "m", "v"):
        for k in KEYS:
            a, b = after[name][k][~vis], before[name][k][~vis]
            assert np.array_equal(_bits(a), _bits(b)), (what, name, k, int((_bits(a) != _bits(b)).sum()))


def _assert_visible_close(got, want, start, vis, what):
    """Per tensor, the share bar: the parameters as their change over the step, the moments as they are."""
    for name in ("arena", "m", "v"):
        for k in KEYS:
            a, b = got[name][k][vis].astype(np.float64), want[name][k][vis].astype(np.float64)
            if name == "arena":
                s = start["arena"][k][vis].astype(np.float64)
                a, b = a - s, b - s
            sh = _share(a, b)
            print(f"{what} {name}.{k}: share of visible elements further than {SHARE_TOL:.0e} max|b| = {sh:.2e} (bar {SHARE:.0e})")
            assert sh < SHARE, (what, name, k)


def _moved_rows(after, before):
    moved = None
    for name in ("arena", "m", "v"):
        for k in KEYS:
            if after[name][k].size == 0:          # (features_rest at K = 1)
                continue
            d = (_bits(after[name][k]) != _bits(before[name][k])).reshape(after[name][k].shape[0], -1).any(axis=1)
            moved = d if moved is None else (moved | d)
    return moved


def _restore(model, clone):
    for name in ("arena", "m", "v"):
        getattr(model, name).copy_(clone[name])


# --------------------------------------------------------------------------------------------------------------- 1. the mask
@pytest.mark.parametrize("tile,trim", [((16, 16), 2), ((16, 16), 0), ((50, 38), 2)])
def test_mask_is_radius_positive(oracle32, tile, trim):
    N, K = 3000, 25
    p, cams, vis = _ordered(N, K, "scattered", oracle32)
    r = _renderer(K, tile)
    r.setTuning(trim_rects=trim)
    r.setSparseAdam(True)
    params = _dev(p)
    res = r.renderForward(params, cams[1], want_radii=True)
    got = _np(r.visibility())
    assert got.dtype == np.bool_ and got.shape == (N,)
    assert np.array_equal(got, vis)                                   # the float32 oracle's radii > 0, exactly
    assert np.array_equal(got, _np(res.radii) > 0)                    # the forward's own
    r.sync()
    assert int(got.sum()) == r.stats()["N_visible"] == cpu.TABLE[(N, K)][0]
    print(f"tile {tile} trim_rects {trim}: {int(got.sum())} visible, longest tile list {r.stats()['max_tile_list']}")
    # camera A sees everything
    r.renderForward(params, cams[0])
    assert bool(r.visibility().all())
    r.setTuning(trim_rects=2)


def test_mask_does_not_depend_on_depth_cuts(oracle32):
    N, K = 3000, 25
    p, cams, vis = _ordered(N, K, "scattered", oracle32)
    r = _renderer(K)
    r.setSparseAdam(True)
    r.cutMinDropped = 0                                               # always cut
    params = _dev(p)
    r.renderForward(params, cams[1], viewKey="b")                     # first visit: no cuts yet
    assert not r.forwardMissed()
    assert np.array_equal(_np(r.visibility()), vis)
    r.renderBackward(_cot())                                          # the backward's item kernel records the view's cuts
    r.renderForward(params, cams[1], viewKey="b")                     # second visit: binned under them
    if r.forwardMissed():
        r.renderForward(params, cams[1], viewKey="b", depthCuts=False)
        assert not r.forwardMissed()
    assert np.array_equal(_np(r.visibility()), vis)
    r.sync()
    assert r.stats()["N_visible"] == int(vis.sum())


# ---------------------------------------------------------------------------------------------------------- 2. one fused step
CASES = [("3000-25-scattered", 3000, 25, "scattered", {}), ("3000-25-blocked", 3000, 25, "blocked", {}),
         ("3001-25-blocked", 3001, 25, "blocked", {}), ("1500-16-scattered", 1500, 16, "scattered", {}),
         ("700-4-scattered", 700, 4, "scattered", {}), ("333-1", 333, 1, "scattered", {}),
         ("3000-25-capacity-4096", 3000, 25, "scattered", dict(capacity=4096)), ("3000-25-antialiased", 3000, 25, "scattered", dict(aa=True)),
         ("3000-25-pose", 3000, 25, "blocked", dict(pose=True))]


@pytest.mark.parametrize("tag,N,K,order,opt", CASES, ids=[c[0] for c in CASES])
def test_one_fused_step(oracle32, tag, N, K, order, opt):
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cams, vis = _ordered(N, K, order, oracle32)
    ninv = int((~vis).sum())
    r = _renderer(K, aa=bool(opt.get("aa")))
    model = GaussModel(p, r.device)
    if "capacity" in opt:
        model.restride(opt["capacity"])
        assert model.stride == opt["capacity"] and model.N == N
    lrs = getLearningRates(0, 1000)
    cot = _cot()
    delta = grad = None
    if opt.get("pose"):
        delta, grad = torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda")
        r.setPoseCorrection(delta, grad)
    # moments: one dense step on camera A, where every Gaussian is visible (and, by the oracle, every one of B's invisible rows
    # gets a non-zero gradient)
    r.renderForward(model.getParams(), cams[0], wantDepth=False)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
    clone = {name: getattr(model, name).clone() for name in ("arena", "m", "v")}
    start = _state(model)
    # dense
    r.renderForward(model.getParams(), cams[1], wantDepth=False)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
    dense = _state(model)
    dense_pose = None if grad is None else _np(grad).copy()
    # sparse, from the same state
    _restore(model, clone)
    r.setSparseAdam(True)
    res = r.renderForward(model.getParams(), cams[1], wantDepth=False, want_radii=True)
    mask = _np(r.visibility())
    assert np.array_equal(mask, _np(res.radii) > 0)
    # (the oracle saw the parameters before camera A's step moved them, and knows neither the anti-aliased mode nor the composed
    # camera: the step is judged on the device's own mask, which test_mask_is_radius_positive holds against the oracle's)
    print(f"{tag}: {int((mask != vis).sum())} rows whose visibility differs from the float32 oracle's on the start parameters")
    assert int((mask != vis).sum()) <= 3
    vis = mask
    ninv = int((~vis).sum())
    waves = np.pad(vis, (0, -N % 64)).reshape(-1, 64)[:N // 64].sum(axis=1)
    if order == "blocked":
        assert int((waves[:8] == 0).sum()) >= 7 and ((waves > 0) & (waves < 64)).any()      # all-invisible workgroups and a mixed wave
    else:
        assert ((waves > 0) & (waves < 64)).sum() >= len(waves) - 1                          # (nearly) every full wave is mixed
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
    sparse = _state(model)
    sparse_pose = None if grad is None else _np(grad).copy()
    # the pads and the rows from N on were never written
    on = sa.element_mask(np.ones(N, bool), model.seg_end, sa.model_row_floats(model), N)
    for name in ("arena", "m", "v"):
        assert np.array_equal(_bits(_np(getattr(model, name))[~on]), _bits(_np(clone[name])[~on])), name

    _assert_invisible_untouched(sparse, start, vis, tag)
    moved = _moved_rows(dense, start)
    print(f"{tag}: {ninv} invisible rows; the dense step moved {int(moved[~vis].sum())} of them, the sparse step none; "
          f"{int((~_moved_rows(sparse, start))[vis].sum())} visible rows unmoved by the sparse step")
    assert int(moved[~vis].sum()) >= math.ceil(ninv * 500 / 564)           # the test has teeth
    # a visible row moves wherever the dense step moves it -- on a zero gradient too, its moments decay; a row that neither
    # camera's cotangent reached has zero moments and a zero gradient, and stays put in both
    smoved = _moved_rows(sparse, start)
    assert abs(int(smoved[vis].sum()) - int(moved[vis].sum())) <= 2 and int(smoved[vis].sum()) > int(vis.sum()) // 2
    _assert_visible_close(sparse, dense, start, vis, tag)
    if grad is not None:
        err = np.abs(sparse_pose - dense_pose).max() / np.abs(dense_pose).max()
        print(f"{tag}: pose gradient sparse against dense {err:.3e} (bar 1e-3), max {np.abs(dense_pose).max():.3e}")
        assert np.abs(dense_pose).max() > 0 and err <= 1e-3
        r.setPoseCorrection(None, None)


# ----------------------------------------------------------------------------------------------------------- 3. unfused path
def _targets(r, p, cams):
    from gaussiansplattingmlx_amd.scenes import perturb
    tp = _dev(perturb(p, 5, 0.1))
    return [r.renderChecked(tp, c).render.clone() for c in cams]


def test_unfused_step_matches_the_fused_sparse_step(oracle32):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    N, K = 3000, 25
    p, cams, vis = _ordered(N, K, "scattered", oracle32)
    r = _renderer(K)
    targets = _targets(r, p, cams)
    out = {}
    for fuse in (True, False):
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse, sparse_adam=True, densify=False)
        tr.trainStep(cams[0], targets[0])                             # camera A: every row gets moments
        assert bool(r.visibility().all()) and not r.sparseAdam        # (the trainer puts the setting back)
        start = _state(model)
        tr.trainStep(cams[1], targets[1])
        mask = _np(r.visibility())                                    # (of parameters camera A's step has moved a little)
        print(f"fuse_adam={fuse}: {int(mask.sum())} visible, {int((mask != vis).sum())} rows differ from the oracle's start mask")
        assert int((mask != vis).sum()) <= 3
        out[fuse] = (start, _state(model), mask)
        _assert_invisible_untouched(out[fuse][1], start, mask, f"fuse_adam={fuse}")
        assert int(_moved_rows(out[fuse][1], start)[mask].sum()) > int(mask.sum()) // 2
    both = out[True][2] & out[False][2]
    assert int((out[True][2] != out[False][2]).sum()) <= 1
    _assert_visible_close(out[False][1], out[True][1], out[True][0], both, "unfused against fused")


# ------------------------------------------------------------------------------ 4. gs_adam_step_visible against the numpy rule
@pytest.mark.parametrize("layout", ["strided-1100", "packed-odd-tail"])
def test_adam_step_visible_matches_numpy(layout):
    r = _renderer()
    N, widths = 1001, (3, 3, 72, 3, 4, 1)
    rng = np.random.default_rng(11)
    if layout == "strided-1100":
        seg_len = [1100 * w for w in widths]                          # rows N .. 1099 of every segment: the strided tail
    else:
        seg_len = [(N * w + 3) & ~3 for w in widths[:-1]] + [N * widths[-1]]      # pads of 1, 1, 0, 1, 0 floats; n % 4 == 1
    seg_end = np.cumsum(seg_len).astype(np.int64)
    n = int(seg_end[-1])
    assert (n % 4 == 1) == (layout != "strided-1100")
    lrs = np.array([1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 2.5e-2], np.float32)
    p, g = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    vis = rng.random(N) < 0.4
    assert 0.3 < vis.mean() < 0.5
    on = sa.element_mask(vis, seg_end, widths, N)
    assert int(on.sum()) == int(vis.sum()) * sum(widths)
    # the moving elements start from zero moments, as test_adam_step_matches_numpy's do (its bars are for sums without
    # cancellation: the device contracts b m + (1 - b) g into one rounding, numpy rounds twice); every other element holds
    # moments that a touch would change
    m, v = (0.1 * rng.normal(size=n)).astype(np.float32), (0.01 * rng.random(n)).astype(np.float32)
    m[on] = 0.0
    v[on] = 0.0
    lr_el = np.repeat(lrs, seg_len).astype(np.float32)
    tp, tg, tm, tv = (torch.as_tensor(a, device="cuda") for a in (p, g, m, v))
    tvis = torch.as_tensor(vis, device="cuda")
    b1, b2, eps, scale = 0.9, 0.999, 1e-15, 0.5
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    for _ in range(3):
        r.adamStepVisible(tp, tg, tm, tv, seg_end, lrs, widths, N, tvis, b1, b2, eps, scale)
        p, m, v = sa.adam_visible(p, g, m, v, lr_el, on, b1, b2, eps, scale)
    gp, gm, gv = _np(tp), _np(tm), _np(tv)
    for got, first, what in ((gp, p0, "p"), (gm, m0, "m"), (gv, v0, "v")):
        assert np.array_equal(_bits(got[~on]), _bits(first[~on])), what      # masked rows, rows >= N, pads: every bit
    print(f"{layout}: n = {n}, {int(on.sum())} of {n} elements move; max |p - numpy| = {np.abs(gp - p).max():.3e}, "
          f"|m - numpy| = {np.abs(gm - m).max():.3e}, |v - numpy| = {np.abs(gv - v).max():.3e}")
    np.testing.assert_allclose(gp, p, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(gm, m, rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(gv, v, rtol=2e-6, atol=1e-12)
    assert (gp[on] != p0[on]).all()
    # argument checks, as gs_adam_step's
    args = lambda se, w, nn, visible: r.lib.gs_adam_step_visible(      # noqa: E731
        r.ctx, n, tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), 6, se.ctypes.data_as(C.c_void_p),
        lrs.ctypes.data_as(C.c_void_p), np.asarray(w, np.int32).ctypes.data_as(C.c_void_p), C.c_float(b1), C.c_float(b2),
        C.c_float(eps), C.c_float(scale), nn, visible)
    assert args(seg_end, (3, 3, 0, 3, 4, 1), N, tvis.data_ptr()) == 1            # a row width below 1
    short = seg_end.copy()
    short[-1] -= 4
    assert args(short, widths, N, tvis.data_ptr()) == 2                          # segments do not cover the arena
    assert args(seg_end, widths, -1, tvis.data_ptr()) == 1
    assert args(seg_end, widths, N, None) == 5                                   # NULL mask and no forward under the setting
    assert np.array_equal(_bits(_np(tp)), _bits(gp))


# ------------------------------------------------------------------------------------------------------------------ 5. trainer
@pytest.mark.parametrize("fuse", [True, False])
def test_trainer_moves_only_what_each_step_saw(oracle32, fuse):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    N, K = 3000, 25
    p, cams, vis_b = _ordered(N, K, "scattered", oracle32)
    r = _renderer(K)
    targets = _targets(r, p, cams)
    model = GaussModel(p, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse, sparse_adam=True, densify=False)
    seen = []
    for it in range(6):
        before = _state(model)
        loss = tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
        vis = _np(r.visibility())
        seen.append(int(vis.sum()))
        _assert_invisible_untouched(_state(model), before, vis, f"step {it}")
        assert np.isfinite(_np(loss)).all()
        assert not r.sparseAdam
    print(f"fuse_adam={fuse}: visible per step {seen}")
    # (the parameters move between the visits: a count may change by a borderline Gaussian or two)
    assert seen[0] == seen[3] == N and abs(seen[1] - int(vis_b.sum())) <= 3 and abs(seen[4] - seen[1]) <= 3
    assert 0 < seen[2] < N and abs(seen[5] - seen[2]) <= 3
    assert np.isfinite(_np(model.arena)).all()


# -------------------------------------------------------------------------------------------------------- 6. gate and refusals
def test_an_overflowed_step_moves_no_row(oracle32):
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel
    N, K = 3000, 25
    p, cams, _ = _ordered(N, K, "scattered", oracle32)
    r0 = _renderer(K)
    r0.renderForward(_dev(p), cams[1])
    r0.sync()
    M = r0.stats()["M"]
    r0.close()
    r = _renderer(K)
    r.reserve(N, M // 3)                                     # too small on purpose: a reported overflow
    r.setSparseAdam(True)
    model = GaussModel(p, r.device)
    model.m.fill_(0.25)
    model.v.fill_(0.125)
    before = {name: getattr(model, name).clone() for name in ("arena", "m", "v")}
    res = r.renderForward(model.getParams(), cams[1], wantDepth=False)
    try:                                                     # may or may not have seen the flag yet: both are in contract
        _, gc, _ = r.lossForwardBackward(res.render, torch.rand(H, W, 3, device="cuda"), 0.2)
        r.renderBackwardAdam(gc, model.arena, model.m, model.v, [1e-2] * 6)
    except GsplatError as e:
        assert e.code == 3
    with pytest.raises(GsplatError) as ei:
        r.sync()
    assert ei.value.code == 3 and r.stats()["overflow"] == 1
    for name in ("arena", "m", "v"):
        assert torch.equal(getattr(model, name), before[name]), name


def test_refusals(oracle32):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    N, K = 3000, 25
    p, cams, vis = _ordered(N, K, "scattered", oracle32)
    r = _renderer(K)
    out = torch.zeros(N, dtype=torch.uint8, device="cuda")
    assert r.lib.gs_set_sparse_adam(r.ctx, 2) == 1
    assert r.lib.gs_get_visibility(r.ctx, N, out.data_ptr()) == 5                  # GS_ERR_NO_FORWARD: no forward at all
    params = _dev(p)
    r.renderForward(params, cams[1], wantDepth=False)
    assert r.lib.gs_get_visibility(r.ctx, N, out.data_ptr()) == 5                  # ... and none under the setting
    r.setSparseAdam(True)
    assert r.lib.gs_get_visibility(r.ctx, N, out.data_ptr()) == 5
    # a backward + Adam of a forward made before the setting went on has no mask to go by
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel
    cot = _cot()
    model = GaussModel(p, r.device)
    before = model.arena.clone()
    r.setSparseAdam(False)
    r.renderForward(model.getParams(), cams[1], wantDepth=False)
    r.setSparseAdam(True)
    with pytest.raises(GsplatError) as ei:
        r.renderBackwardAdam(cot, model.arena, model.m, model.v, [1e-3] * 6)
    assert ei.value.code == 5 and torch.equal(model.arena, before) and not bool(model.m.any())
    r.renderForward(params, cams[1], wantDepth=False)
    assert r.lib.gs_get_visibility(r.ctx, N - 1, out.data_ptr()) == 2              # GS_ERR_SIZE_MISMATCH
    assert r.lib.gs_get_visibility(r.ctx, N, None) == 1
    assert r.lib.gs_get_visibility(r.ctx, N, out.data_ptr()) == 0 and np.array_equal(_np(out) != 0, vis)
    # the data-parallel entry points
    g = [torch.zeros(N, k, device="cuda") for k in (3, 3, 4, 1)]
    cc = torch.zeros(3 * N + 16, device="cuda")
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 1
    assert r.lib.gs_render_backward_dp_begin(r.ctx, cot.data_ptr(), None, None, cc.data_ptr()) == 1
    assert r.lib.gs_render_backward_dp_finish(r.ctx, *[t.data_ptr() for t in g]) == 1
    assert not any(bool(t.any()) for t in g) and not bool(cc.any())
    # ... and the other entries the setting refuses: each returns GS_ERR_INVALID_ARG with the sparse Adam message, whatever else
    # is wrong with the arguments (null pointers and zeros here)
    def dummy_call(name):
        fn = getattr(r.lib, name)
        args = [None if t is C.c_void_p or hasattr(t, "contents") else (0.0 if t is C.c_float else 0) for t in fn.argtypes[1:]]
        rc = fn(r.ctx, *args)
        return rc, r.lib.gs_last_error(r.ctx).decode()
    others = ("gs_dp_step", "gs_sh_grad_from_views_adam", "gs_sh_grad_from_views_adam_dir", "gs_render_backward_dp_geom",
              "gs_render_backward_dp_finish_geom")
    for name in others:
        rc, msg = dummy_call(name)
        assert rc == 1 and msg.startswith(name + ":") and "sparse Adam is on" in msg, (name, rc, msg)
    r.setSparseAdam(False)
    for name in others:             # (off: whatever these arguments earn, it is not that refusal)
        rc, msg = dummy_call(name)
        assert rc != 0 and "sparse Adam" not in msg, (name, rc, msg)
    r.setSparseAdam(True)
    # MCMC and the 3-D filter, in either order
    mp = MCMCConfig(cap_max=N).params(0, 1)
    assert r.lib.gs_set_mcmc(r.ctx, C.byref(mp)) == 1
    assert r.lib.gs_set_mcmc(r.ctx, None) == 0
    f = torch.full((N,), 1e-3, device="cuda")
    assert r.lib.gs_set_filter3d(r.ctx, f.data_ptr()) == 1
    assert r.lib.gs_set_filter3d(r.ctx, None) == 0
    r.setSparseAdam(False)
    assert r.lib.gs_set_mcmc(r.ctx, C.byref(mp)) == 0
    assert r.lib.gs_set_sparse_adam(r.ctx, 1) == 1
    assert r.lib.gs_set_mcmc(r.ctx, None) == 0
    assert r.lib.gs_set_filter3d(r.ctx, f.data_ptr()) == 0
    assert r.lib.gs_set_sparse_adam(r.ctx, 1) == 1
    assert r.lib.gs_set_filter3d(r.ctx, None) == 0
    assert r.lib.gs_set_sparse_adam(r.ctx, 1) == 0 and r.lib.gs_set_sparse_adam(r.ctx, 0) == 0
    # off again: the data-parallel backward is served
    r.renderForward(params, cams[1], wantDepth=False)
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 0


# ---------------------------------------------------------------------------------------------------------------- 7. off is off
def test_off_is_off(oracle32):
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER, GaussModel, arenaLearningRates, getLearningRates
    N, K = 3000, 25
    p, cams, vis = _ordered(N, K, "scattered", oracle32)
    cot = _cot()
    # a renderer that never heard of the setting, and one that had it on and off again
    r0, r1 = _renderer(K), _renderer(K)
    r1.setSparseAdam(True)
    r1.renderForward(_dev(p), cams[1], wantDepth=False)
    r1.setSparseAdam(False)
    results = []
    for r in (r0, r1):
        model = GaussModel(p, r.device)
        model.m.copy_(torch.as_tensor(np.random.default_rng(5).normal(0, 1e-3, model.numel).astype(np.float32)))
        model.v.copy_(torch.as_tensor((np.random.default_rng(6).random(model.numel) * 1e-6).astype(np.float32)))
        start = _state(model)
        flat0 = {name: _np(getattr(model, name)).copy() for name in ("arena", "m", "v")}
        res = r.renderForward(model.getParams(), cams[1], wantDepth=False)
        img = res.render.clone()
        out = torch.zeros(N, dtype=torch.uint8, device="cuda")
        assert r.lib.gs_get_visibility(r.ctx, N, out.data_ptr()) == 5            # GS_ERR_NO_FORWARD
        # the parent's dense step, spelt out: the unfused backward's gradients through numpy's dense Adam
        grads = r.renderBackward(cot, out=model.getGrads())
        assert grads is not None
        gflat = _np(model.grad).copy()
        lr_el = np.repeat(np.asarray(arenaLearningRates(0, 1000), np.float32),
                          np.diff(np.concatenate([[0], model.seg_end]))).astype(np.float32)
        want_flat = sa.adam_dense(flat0["arena"], gflat, flat0["m"], flat0["v"], lr_el)
        r.renderForward(model.getParams(), cams[1], wantDepth=False)
        r.renderBackwardAdam(cot, model.arena, model.m, model.v, getLearningRates(0, 1000))
        got = _state(model)
        want = {}
        for name, flat in zip(("arena", "m", "v"), want_flat):
            t = torch.as_tensor(flat)
            want[name] = {k: _np(x).copy() for k, x in model._carve(t, model.N, model.stride).items()}
        _assert_visible_close(got, want, start, np.ones(N, bool), "setting off against backward + numpy Adam")
        assert _moved_rows(got, start)[~vis].all()                               # dense: the invisible rows move too
        results.append((img, got))
    assert torch.equal(results[0][0], results[1][0])                             # the render
    _assert_visible_close(results[1][1], results[0][1], start, np.ones(N, bool), "had the setting on once against never")
    assert list(ARENA_ORDER)[0] == "xyz"
