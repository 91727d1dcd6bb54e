"""Depth supervision on the device (include/gsplat.h gs_depth_loss / gs_depth_normalize, GaussianRenderer.depthLoss /
expectedDepth, GaussianTrainer(depth=DepthConfig(...))) against the float64 restatement
(tests/depth_loss_numpy.py), against the existing depth term of gs_loss_forward_backward, and -- a train step -- against the
oracle's loop and the manual call sequence.

Bars, fixed before the first run on the card:
  - float64 (measured: Ld within 9.4e-8, cotangents within 1.9e-7 relative): Ld within 2e-6 (the project's loss bar, test_gpu_parity.test_loss_forward_backward); every cotangent element within
    1e-3 of its image's largest component and within 1e-5 relative of its own float64 value where that is non-zero (a cotangent
    is a sign times at most four float32 operations: 1e-5 leaves more than 50 ulp); invalid pixels exactly 0.0f; the outputs are
    pre-filled with NaN and must come back finite;
  - mode 0 with scale 1, offset 0 against lossForwardBackward(..., lambda_depth): cot_depth torch.equal, loss[3] and loss[0]
    within 2e-6;
  - two calls torch.equal; mask=None torch.equal to a mask of ones; nothing valid gives Ld == 0 and zero cotangents;
    scale / offset torch.equal to a target transformed beforehand in float32 with the same two operations;
  - expectedDepth is D / a in float32 on valid pixels, 0 elsewhere;
  - three train steps in each mode, fuse_adam on and off, against the oracle loop (render_forward, loss_forward_backward, the
    numpy depth loss, render_backward with cotDepth / cotAlpha, Adam): test_gpu_trajectory's own bars -- per-step loss 1e-5,
    moments 1e-3 of the largest magnitude on all but 1e-3 of the elements and none beyond 2e-2, parameters beyond 1e-3 on no
    larger a share than 1.5 x the float64 oracle loop's + 5e-4, no element further than sign flips can take it.  The float32
    to float64 oracle distance is printed beside every figure.
    Measured (MI355X, 64 x 64, 300 Gaussians, three steps; worst over the modes and fuse_adam on / off, the float64 oracle
    loop's distance from the float32 one in brackets): loss 2.3e-8 (2.8e-8); parameters 2.6e-5 of the tensor's largest
    magnitude (4.8e-5), first moments 2.2e-6 (2.8e-5), second moments 2.7e-6 (2.2e-5); no element beyond 1e-3 on either
    side: the depth term fits the file's bars as they are;
  - a step with exposure, random background or sparse Adam is the manual sequence renderForward, lossForwardBackward,
    depthLoss, renderBackwardAdam with both cotangents, to the bit, on test_gpu_loss_mask's one-block-per-splat scene (where the
    blend backward's float atomics have one term per Gaussian and bits mean something); depth=None is today's step to the bit;
    the renderer's depth_gradient knob is what it was before the step, also when the step raises;
  - what it is for: two runs of 60 steps are compared, no absolute number is fixed.

Shapes, chosen for the reduction (256 threads a block, at most 512 blocks): (37, 53) fewer pixels than one grid, (152, 200)
several blocks, (300, 450) more pixels than 512 x 256 threads -- the grid-stride loops wrap."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_BAR, COT_MAX_BAR, COT_REL_BAR = 2e-6, 1e-3, 1e-5
SHAPES = [(37, 53), (152, 200), (300, 450)]
MODES = [0, 1, 2]
LAM, AMIN = 0.3, 0.05


def _load(name):
    spec = importlib.util.spec_from_file_location("_dlg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dln = _load("depth_loss_numpy")
traj = _load("test_gpu_trajectory")
lmg = _load("test_gpu_loss_mask")
ge = lmg.ge
en = lmg.en


def _renderer(W, H):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, (16, 16), False)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


_cases = {}
_renderers = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_contexts():
    """The renderers and device images the tests of this file share live as long as the file's tests do, no longer."""
    yield
    for r in _renderers.values():
        r.close()
    _renderers.clear()
    _cases.clear()


def _r(H, W):
    if (H, W) not in _renderers:
        _renderers[(H, W)] = _renderer(W, H)
    return _renderers[(H, W)]


def _case(H, W, mode):
    """The inputs of one shape and mode on the host and the device with the float64 result: computed once, never written."""
    if (H, W, mode) not in _cases:
        D, a, target, mask = dln.inputs(H, W, mode, AMIN)
        _cases[(H, W, mode)] = dict(D=D, a=a, target=target, mask=mask, dev=tuple(_dev(x) for x in (D, a, target, mask)),
                                    want=dln.depth_loss(mode, D, a, target, mask, LAM, AMIN))
    return _cases[(H, W, mode)]


def _call(r, mode, D, a, target, mask, lam=LAM, amin=AMIN, scale=1.0, offset=0.0, base=(0.25, 0.0, 0.0, float("nan"))):
    """gs_depth_loss into NaN-filled cotangents and a loss that holds `base`: (loss, cotDepth, cotAlpha), tensors of their own."""
    out = dict(loss=torch.tensor(base, dtype=torch.float32, device="cuda"),
               cotDepth=torch.full((r.H, r.W), float("nan"), device="cuda"),
               cotAlpha=torch.full((r.H, r.W), float("nan"), device="cuda"))
    return r.depthLoss(D, a, target, mask, r.depthLossParams(mode, lam, amin, scale, offset), out=out)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ float64
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_against_float64(H, W, mode):
    c = _case(H, W, mode)
    r = _r(H, W)
    loss, cd, ca = _call(r, mode, *c["dev"])
    L64, cd64, ca64, valid = c["want"]
    loss, cd, ca = _np(loss), _np(cd), _np(ca)
    assert valid.any() and not valid.all()
    if mode:
        blk = (slice(H // 5, 2 * (H // 5)), slice(0, W // 4))
        assert (c["a"][blk] == np.float32(AMIN)).all() and valid[blk][c["mask"][blk] != 0].all()      # a == alpha_min counts
        assert not valid[: H // 5, : W // 4].any()                                                  # a == 0 does not
    else:
        ties = valid & (c["target"] == c["D"])
        assert ties.any() and not cd[ties].any()
    print(f"{H}x{W} mode {mode}: Ld {loss[3]:.9g} float64 {float(L64):.12g} (diff {abs(float(loss[3]) - float(L64)):.3g}), "
          f"loss[0] diff {abs(float(loss[0]) - (0.25 + float(np.float32(LAM)) * float(L64))):.3g}, valid {int(valid.sum())}")
    assert np.isfinite(loss).all() and np.isfinite(cd).all() and np.isfinite(ca).all()
    assert abs(float(loss[3]) - float(L64)) <= LOSS_BAR
    assert abs(float(loss[0]) - (0.25 + float(np.float32(LAM)) * float(L64))) <= LOSS_BAR
    for name, got, want in (("cot_depth", cd, cd64), ("cot_alpha", ca, ca64)):
        nz = want != 0
        err = np.abs(got.astype(np.float64) - want)
        rel = float((err[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
        print(f"  {name}: max error {float(err.max()):.3g} of {float(np.abs(want).max()):.3g}, max relative {rel:.3g}")
        assert float(err.max()) <= COT_MAX_BAR * float(np.abs(want).max()) + 0.0
        assert rel <= COT_REL_BAR
        assert not got[~valid].any() and np.array_equal(got != 0, nz)
    if mode == 0:
        assert not ca.any()


# ------------------------------------------------------------------------------------------------------------ the existing term
@pytest.mark.parametrize("H,W", SHAPES)
def test_accumulated_mode_is_the_existing_depth_term(H, W):
    c = _case(H, W, 0)
    r = _r(H, W)
    D, a, target, mask = c["dev"]
    ren, tgt, _ = ge._images(H, W)
    ren, tgt = _dev(ren), _dev(tgt)
    lo, _, gd = r.lossForwardBackward(ren, tgt, 0.2, D, target, mask, LAM)
    lo, gd = lo.clone(), gd.clone()
    plain, _, _ = r.lossForwardBackward(ren, tgt, 0.2)
    loss, cd, ca = r.depthLoss(D, None, target, mask, r.depthLossParams(0, LAM), out=dict(
        loss=plain, cotDepth=torch.full((H, W), float("nan"), device="cuda")))
    print(f"{H}x{W}: depth term {float(loss[3]):.9g} existing {float(lo[3]):.9g}; total {float(loss[0]):.9g} existing {float(lo[0]):.9g}")
    assert ca is None and loss is plain
    assert torch.equal(cd, gd)
    assert abs(float(loss[3]) - float(lo[3])) <= LOSS_BAR and abs(float(loss[0]) - float(lo[0])) <= LOSS_BAR
    assert torch.equal(loss[1:3], lo[1:3])


# ------------------------------------------------------------------------------------------------------------ determinism, edges
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_determinism_and_edges(H, W, mode):
    c = _case(H, W, mode)
    r = _r(H, W)
    D, a, target, mask = c["dev"]
    first = _call(r, mode, D, a, target, mask)
    assert _equal(first, _call(r, mode, D, a, target, mask))
    assert _equal(first, _call(r, mode, D, a, target, c["mask"] != 0))                    # a host bool array
    ones = _call(r, mode, D, a, target, torch.ones(H, W, dtype=torch.uint8, device="cuda"))
    assert _equal(ones, _call(r, mode, D, a, target, None)) and not torch.equal(ones[1], first[1])
    empties = [(D, a, torch.zeros(H, W, dtype=torch.uint8, device="cuda"))]
    if mode:
        empties.append((D, torch.zeros_like(a), mask))
        empties.append((torch.zeros_like(D), torch.zeros_like(a), None))
    if mode == 2:
        empties.append((torch.zeros_like(D), a, mask))
    for De, ae, me in empties:
        loss, cd, ca = _call(r, mode, De, ae, target, me)
        assert _np(loss).tolist()[:3] == [0.25, 0.0, 0.0] and float(loss[3]) == 0.0
        assert not bool(cd.any()) and not bool(ca.any())
    # alpha_min = 0: a pixel nothing was blended into has no expected depth, and nothing is NaN or Inf
    loss, cd, ca = _call(r, mode, D, a, target, None, amin=0.0)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(cd).all()) and bool(torch.isfinite(ca).all())
    # scale and offset: the target transformed beforehand on the host, in float32, with the same two operations
    s, o = np.float32(0.75), np.float32(0.125)
    pre = (s * c["target"] + o).astype(np.float32)
    assert pre.dtype == np.float32
    assert _equal(_call(r, mode, D, a, target, mask, scale=float(s), offset=float(o)), _call(r, mode, D, a, _dev(pre), mask))
    assert not _equal(_call(r, mode, D, a, target, mask, scale=float(s), offset=float(o)), first)


def test_expected_depth_and_argument_errors():
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd._lib import GsplatError
    H, W = 37, 53
    c = _case(H, W, 1)
    r = _r(H, W)
    D, a, target, mask = c["dev"]
    e = r.expectedDepth((D, a), AMIN)
    ok = (c["a"] >= np.float32(AMIN)) & (c["a"] > 0)
    assert tuple(e.shape) == (H, W) and np.array_equal(_np(e)[ok], c["D"][ok] / c["a"][ok]) and not _np(e)[~ok].any()
    assert ok[H // 5: 2 * (H // 5), : W // 4].all() and not ok[: H // 5, : W // 4].any()
    assert bool(torch.isfinite(r.expectedDepth((D, a), 0.0)).all())
    inplace = D.clone()                                                     # out may be depth itself (include/gsplat.h)
    r._check(r.lib.gs_depth_normalize(r.ctx, H * W, C.c_void_p(inplace.data_ptr()), C.c_void_p(a.data_ptr()), C.c_float(AMIN),
                                      C.c_void_p(inplace.data_ptr())))
    assert torch.equal(inplace, e)
    from gaussiansplattingmlx_amd.renderer import RenderResult
    assert torch.equal(r.expectedDepth(RenderResult(None, D.view(H, W, 1), a.view(H, W, 1), None, None), AMIN).view(H, W), e)
    with pytest.raises(ValueError):
        r.expectedDepth(RenderResult(None, None, a, None, None))
    P = r.depthLossParams
    ok_call = lambda p, cot_alpha=True, alpha=a: r.depthLoss(D, alpha, target, mask, p, out=dict(
        loss=torch.zeros(4, device="cuda"), cotDepth=torch.empty(H, W, device="cuda"),
        cotAlpha=torch.empty(H, W, device="cuda") if cot_alpha else None))
    ok_call(P(1, LAM))
    for bad, text in ((P(3, LAM), "mode"), (P(-1, LAM), "mode"), (P(1, LAM, -0.01), "alpha_min"), (P(1, float("nan")), "finite"),
                      (P(1, LAM, AMIN, float("inf")), "finite"), (P(1, LAM, AMIN, 1.0, float("nan")), "finite")):
        with pytest.raises(GsplatError, match="GS_ERR_INVALID_ARG") as ei:
            ok_call(bad)
        assert text in str(ei.value)
    for mode in (1, 2):
        with pytest.raises(GsplatError, match="GS_ERR_INVALID_ARG"):
            ok_call(P(mode, LAM), cot_alpha=False)
    ok_call(P(0, LAM), cot_alpha=False, alpha=None)                        # mode 0 needs neither
    p = P(1, LAM)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    z4, img = torch.zeros(4, device="cuda"), torch.empty(H, W, device="cuda")
    args = [ptr(D), ptr(a), ptr(target), ptr(mask), ptr(z4), ptr(img), ptr(torch.empty(H, W, device="cuda"))]
    for i in (0, 1, 2, 4, 5, 6):                                             # every image but the mask
        broken = list(args)
        broken[i] = None
        assert _lib.STATUS.get(r.lib.gs_depth_loss(r.ctx, C.byref(p), *broken)) == "GS_ERR_INVALID_ARG"
        assert b"gs_depth_loss" in r.lib.gs_last_error(r.ctx)
    assert _lib.STATUS.get(r.lib.gs_depth_loss(r.ctx, None, *args)) == "GS_ERR_INVALID_ARG"
    with pytest.raises(ValueError):
        r.depthLoss(D, a, target, torch.zeros(H, W, device="cuda"), P(1, LAM))      # a float mask
    with pytest.raises(ValueError):
        r.depthLoss(D, a, target[:-1], mask, P(1, LAM))
    with pytest.raises(ValueError):
        P("median", LAM)


# ------------------------------------------------------------------------------------------------------------ the oracle
SW, SH, SN, STEPS = 64, 64, 300, 3


def _depth_targets(o, p0, cams, mode, seed=11):
    """Per view: the oracle's own depth image at p0, normalised or inverted per mode, times 1 +- delta (delta in [0.05, 0.3]), and
    the mask a > 0.2: no pixel of it gets near alpha_min, a tie or D = 0 within three steps, in either loop."""
    rng = np.random.default_rng(seed)
    tds, masks = [], []
    for c in cams:
        fw = o.render_forward(p0, c.as_dict(), SW, SH, 16, 16, 4)
        D, a = fw["depth"].reshape(SH, SW).astype(np.float64), fw["alpha"].reshape(SH, SW).astype(np.float64)
        mask = a > 0.2
        safe = np.where(mask, a, 1.0)
        x = D if mode == 0 else (D / safe if mode == 1 else safe / np.where(mask, D, 1.0))
        delta = rng.uniform(0.05, 0.3, (SH, SW)) * rng.choice([-1.0, 1.0], (SH, SW))
        tds.append(np.where(mask, x * (1.0 + delta), 0.0).astype(np.float32))
        masks.append(mask.astype(np.uint8))
    return tds, masks


def _oracle_depth_loop(o, p0, cams, targets, tds, masks, mode, lam, steps=STEPS):
    """test_gpu_trajectory._oracle_loop with the depth term: render_forward, loss_forward_backward, the numpy depth loss on the
    forward's depth and alpha, render_backward with its two cotangents, Adam."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    dt = o.dtype
    p = {k: v.astype(dt).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    b1, b2, eps, one = dt.type(0.9), dt.type(0.999), dt.type(1e-15), dt.type(1)
    losses = []
    for it in range(steps):
        vi = it % len(cams)
        cam = cams[vi].as_dict()
        fw = o.render_forward(p, cam, SW, SH, 16, 16, 4)
        loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(SH, SW, 3), targets[vi].astype(dt), 0.2)
        Ld, cd, ca, _ = dln.depth_loss(mode, fw["depth"].reshape(SH, SW), fw["alpha"].reshape(SH, SW), tds[vi], masks[vi], lam,
                                       AMIN, dtype=dt.type)
        g = o.render_backward(p, cam, SW, SH, 16, 16, 4, fw, cot.reshape(-1, 3), cd.reshape(-1).astype(dt), ca.reshape(-1).astype(dt))
        losses.append(float(loss) + float(np.float32(lam)) * float(Ld))
        lr = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
        for k in traj.KEYS:
            gk = np.asarray(g[k], dt).reshape(p[k].shape)
            m[k] = b1 * m[k] + (one - b1) * gk
            v[k] = b2 * v[k] + (one - b2) * gk * gk
            p[k] = (p[k] - dt.type(lr[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
    return losses, p, m, v


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_three_steps_against_the_oracle_loop(oracle32, oracle64, mode, fuse):
    """Measured on an MI355X (worst over the three modes and fuse_adam on / off; the float64 oracle loop's distance from the
    float32 one in brackets): per-step loss 2.3e-8 (2.8e-8); parameters 2.6e-5 of the tensor's largest magnitude (4.8e-5), first
    moments 2.2e-6 (2.8e-5), second moments 2.7e-6 (2.2e-5); share of elements beyond 1e-3: 0 (0)."""
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, GaussianTrainer, GaussModel, getLearningRates
    lam = 0.5
    p0, cams = traj._scene(71, SN, SW, SH, 0.06)
    tp = perturb(p0, 5, 0.1)
    targets = [oracle32.render_forward(tp, c.as_dict(), SW, SH, 16, 16, 4)["color"].reshape(SH, SW, 3).copy() for c in cams]
    tds, masks = _depth_targets(oracle32, p0, cams, mode)
    want_l, want_p, want_m, want_v = _oracle_depth_loop(oracle32, p0, cams, targets, tds, masks, mode, lam)
    ref_l, ref_p, ref_m, ref_v = _oracle_depth_loop(oracle64, p0, cams, targets, tds, masks, mode, lam)
    r = _renderer(SW, SH)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, fuse_adam=fuse,
                         depth=DepthConfig(mode=dln.MODES[mode], weight=lam, alpha_min=AMIN))
    got_l = []
    for it in range(STEPS):
        vi = it % len(cams)
        loss = tr.trainStep(cams[vi], _dev(targets[vi]), viewKey=vi, targetDepth=_dev(tds[vi]), depthMask=_dev(masks[vi]))
        got_l.append(float(loss[0]))
        assert float(loss[3]) > 0
    assert r.stats()["overflow"] == 0
    N = model.N
    got_p = {k: _np(model.getParams()[k]).copy() for k in traj.KEYS}
    got_m = {k: _np(model._carve(model.m, N)[k]).copy() for k in traj.KEYS}
    got_v = {k: _np(model._carve(model.v, N)[k]).copy() for k in traj.KEYS}
    rep = {}
    for tag, got, want, ref in (("param", got_p, want_p, ref_p), ("m", got_m, want_m, ref_m), ("v", got_v, want_v, ref_v)):
        traj._compare(tag, got, want, p0, rep)
        traj._compare("oracle32_vs_64." + tag, {k: ref[k] for k in traj.KEYS}, want, p0, rep)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    dref = np.abs(np.asarray(ref_l) - np.asarray(want_l))
    print(f"mode {mode} fuse {fuse}: loss {got_l}; |hip - oracle32| {dl.max():.3g}, |oracle64 - oracle32| {dref.max():.3g}")
    for tag in ("param", "m", "v"):
        for k in traj.KEYS:
            e, ref = rep[f"{tag}.{k}"], rep[f"oracle32_vs_64.{tag}.{k}"]
            print(f"  {tag}.{k}: max_rel {e['max_rel']:.3g} share_beyond {e['share_beyond']:.3g} | oracle64: max_rel "
                  f"{ref['max_rel']:.3g} share_beyond {ref['share_beyond']:.3g}")
    assert dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in traj.KEYS:
        for tag in ("m", "v"):
            e = rep[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = rep[f"param.{k}"], rep[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * STEPS * 1.01 + 1e-6, (k, e)


# ------------------------------------------------------------------------------------------------------------ composition
def _block_inputs():
    """test_gpu_loss_mask's one-block-per-splat scene with a colour target, its alpha, and a depth target per mode from the
    scene's own render (the device's): expected depth times 1.1 where alpha >= 0.2, holes (0) elsewhere."""
    if "block" not in _cases:
        p, cam = lmg._block_scene()
        r = _renderer(SW, SH)
        res = r.renderForward(lmg._params(lmg.traj_perturbed(p)), cam)
        target, alpha = res.render.reshape(SH, SW, 3).clone(), res.alpha.reshape(SH, SW).clone()
        res = r.renderForward(lmg._params(p), cam)
        D, a = res.depth.reshape(SH, SW).clone(), res.alpha.reshape(SH, SW).clone()
        keep = a >= 0.2
        safe = torch.where(keep, a, torch.ones_like(a))
        x = {0: D, 1: D / safe, 2: safe / torch.where(keep, D, torch.ones_like(D))}
        tds = {m: torch.where(keep, x[m] * 1.1, torch.zeros_like(D)).contiguous() for m in MODES}
        assert int(keep.sum()) > 200
        _cases["block"] = (p, cam, target, alpha, tds)
    return _cases["block"]


def _adam(r, m):
    from gaussiansplattingmlx_amd.trainer import arenaLearningRates
    lrs = (C.c_float * 6)(*arenaLearningRates(0, 1000))
    seg = (C.c_longlong * 6)(*[int(x) for x in m.seg_end])
    p_ = lambda t: C.c_void_p(t.data_ptr())
    r._check(r.lib.gs_adam_step(r.ctx, m.numel, p_(m.arena), p_(m.grad), p_(m.m), p_(m.v), 6, seg, lrs, C.c_float(0.9),
                                C.c_float(0.999), C.c_float(1e-15), C.c_float(1.0)))


def _manual_depth_step(variant, mode, fuse=True, lam=0.5):
    """renderForward, lossForwardBackward, depthLoss, renderBackwardAdam with both cotangents, on a renderer and a model of its
    own, under the variant's setting."""
    from gaussiansplattingmlx_amd.background import BackgroundConfig
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cam, target, alpha, tds = _block_inputs()
    r = _renderer(SW, SH)
    m = GaussModel(p, r.device)
    r.setTuning(depth_gradient=1)
    if variant == "exposure":
        M, grad = ge._exposure(en.IDENTITY)
        r.setExposure(M, grad)
    elif variant == "background":
        b = BackgroundConfig(seed=3).color_at(0)
        r.setBackground(b)
        target = r.compositeTarget(target, alpha, b)
    elif variant == "sparse_adam":
        r.setSparseAdam(True)
    res = r.renderForward(m.getParams(), cam, wantDepth=True)
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    td = tds[mode]
    loss, cd, ca = r.depthLoss(res.depth, res.alpha if mode else None, td, (td > 0).to(torch.uint8),
                               r.depthLossParams(mode, lam, AMIN), out=dict(loss=loss))
    assert (ca is None) == (mode == 0)
    if fuse:
        r.renderBackwardAdam(cot, m.arena, m.m, m.v, getLearningRates(0, 1000), cotDepth=cd, cotAlpha=ca)
    else:
        r.renderBackward(cot, cd, ca, out=m.getGrads())
        _adam(r, m)
    r.sync()
    return loss.clone(), m


@pytest.mark.parametrize("variant,mode,fuse", [("plain", 0, True), ("plain", 1, True), ("plain", 2, True), ("plain", 1, False),
                                               ("exposure", 1, True), ("background", 1, True), ("background", 2, True),
                                               ("sparse_adam", 1, True)])
def test_one_depth_step_is_the_manual_sequence(variant, mode, fuse):
    from gaussiansplattingmlx_amd.background import BackgroundConfig
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    p, cam, target, alpha, tds = _block_inputs()
    kw, step_kw = {}, {}
    if variant == "exposure":
        kw = dict(exposure_opt=True, n_views=1)
    elif variant == "background":
        kw = dict(background=BackgroundConfig(seed=3))
        step_kw = dict(targetAlpha=alpha)
    elif variant == "sparse_adam":
        kw = dict(sparse_adam=True)
    r = _renderer(SW, SH)
    r.setTuning(depth_gradient=0)
    tr, model = lmg._trainer(r, p, fuse_adam=fuse, depth=DepthConfig(mode=dln.MODES[mode], weight=0.5, alpha_min=AMIN), **kw)
    loss = tr.trainStep(cam, target, viewKey=0, targetDepth=tds[mode], **step_kw).clone()       # depthMask=None: target > 0
    assert r.getTuning("depth_gradient") == 0
    loss2, m2 = _manual_depth_step(variant, mode, fuse)
    print(f"{variant} mode {mode} fuse {fuse}: loss {_np(loss)} manual {_np(loss2)}; max diff arena "
          f"{float((model.arena - m2.arena).abs().max()):.3g} m {float((model.m - m2.m).abs().max()):.3g} v {float((model.v - m2.v).abs().max()):.3g}")
    assert float(loss[3]) > 0 and torch.equal(loss, loss2)
    assert bool(m2.m.any())
    assert torch.equal(model.arena, m2.arena) and torch.equal(model.m, m2.m) and torch.equal(model.v, m2.v)
    # the depth term did its work: without it the step is another one
    tr0, model0 = lmg._trainer(_renderer(SW, SH), p, fuse_adam=fuse, **kw)
    loss0 = tr0.trainStep(cam, target, viewKey=0, **step_kw)
    assert not torch.equal(loss0, loss) and not torch.equal(model0.m, model.m)


@pytest.mark.parametrize("fuse", [True, False])
def test_without_a_config_the_step_is_todays(fuse):
    p, cam, target, alpha, tds = _block_inputs()
    r = _renderer(SW, SH)
    tr, model = lmg._trainer(r, p, fuse_adam=fuse)
    assert tr.depth is None and tr._cotDepth is None and tr._cotAlpha is None
    loss = tr.trainStep(cam, target).clone()
    loss2, m2 = lmg._manual_step(p, cam, target, None, fuse)          # wantDepth=False, depth_gradient=0: the step as it was
    assert torch.equal(loss, loss2) and float(loss[3]) == 0.0
    assert torch.equal(model.arena, m2.arena) and torch.equal(model.m, m2.m) and torch.equal(model.v, m2.v)
    assert r._fused["depth"] is None                                   # the step rendered no depth image
    with pytest.raises(ValueError, match="targetDepth"):
        tr.trainStep(cam, target, targetDepth=tds[1])


@pytest.mark.parametrize("knob", [0, 1])
def test_the_depth_gradient_knob_is_put_back(knob):
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    p, cam, target, alpha, tds = _block_inputs()
    r = _renderer(SW, SH)
    r.setTuning(depth_gradient=knob)
    tr, model = lmg._trainer(r, p, depth=DepthConfig(mode="expected"))
    tr.trainStep(cam, target, targetDepth=tds[1])
    assert r.getTuning("depth_gradient") == knob
    before = model.arena.clone()
    for bad in (dict(targetDepth=tds[1][:-1]), dict(targetDepth=tds[1], depthMask=torch.zeros(SH, SW, device="cuda")),
                dict(targetDepth=tds[1], depthAlign=(1.0, float("nan")))):
        with pytest.raises(ValueError):
            tr.trainStep(cam, target, **bad)                        # raised inside the step, behind the knob's change
        assert r.getTuning("depth_gradient") == knob
    with pytest.raises(ValueError, match="targetDepth"):
        tr.trainStep(cam, target)
    assert r.getTuning("depth_gradient") == knob and torch.equal(model.arena, before)
    # depthAlign reaches the kernel: (2, 0) on half the target is the step on the target itself
    tr1, m1 = lmg._trainer(_renderer(SW, SH), p, depth=DepthConfig(mode="expected"))
    tr2, m2 = lmg._trainer(_renderer(SW, SH), p, depth=DepthConfig(mode="expected"))
    l1 = tr1.trainStep(cam, target, targetDepth=tds[1]).clone()
    l2 = tr2.trainStep(cam, target, targetDepth=tds[1] * 0.5, depthAlign=(2.0, 0.0)).clone()
    assert torch.equal(l1, l2) and torch.equal(m1.arena, m2.arena)


@pytest.mark.parametrize("mode", [1, 2])
def test_host_depth_maps_get_their_own_default_mask(mode):
    """Two different depth maps of one shape as host arrays (TrainData.depthArray[i]) on consecutive steps, without a depthMask:
    each upload may land where the previous one lay, and each step must still leave out its OWN map's holes.  Against the same
    two steps with the masks spelled out."""
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    p, cam, target, alpha, tds = _block_inputs()
    a = _np(tds[mode])
    b = a.copy()
    a[:, : SW // 2] = 0.0                    # view one: holes on the left
    b[: SH // 2, :] = 0.0                    # view two: holes at the top
    b *= np.float32(1.05)
    assert (a > 0).any() and (b > 0).any() and ((a > 0) != (b > 0)).any()
    cfg = dict(mode=dln.MODES[mode], weight=0.5, alpha_min=AMIN)
    tr1, m1 = lmg._trainer(_renderer(SW, SH), p, depth=DepthConfig(**cfg))
    tr2, m2 = lmg._trainer(_renderer(SW, SH), p, depth=DepthConfig(**cfg))
    for td in (a, b):
        l1 = tr1.trainStep(cam, target, targetDepth=td.copy()).clone()                       # a fresh host array every step
        l2 = tr2.trainStep(cam, target, targetDepth=_dev(td), depthMask=_dev((td > 0).astype(np.uint8))).clone()
        assert float(l1[3]) > 0 and torch.equal(l1, l2)
        assert torch.equal(m1.arena, m2.arena) and torch.equal(m1.m, m2.m) and torch.equal(m1.v, m2.v)
    # the second map under the first map's mask is another step: the comparison above can tell the two apart
    tr3, m3 = lmg._trainer(_renderer(SW, SH), p, depth=DepthConfig(**cfg))
    tr3.trainStep(cam, target, targetDepth=_dev(a), depthMask=_dev((a > 0).astype(np.uint8)))
    l3 = tr3.trainStep(cam, target, targetDepth=_dev(b), depthMask=_dev((a > 0).astype(np.uint8))).clone()
    assert not torch.equal(l3, l1)


@pytest.mark.parametrize("variant", ["mcmc", "antialiased", "loss_mask", "absgrad"])
def test_a_depth_step_composes(variant):
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    p, cams = lmg._step_scene()
    r = _renderer(SW, SH)
    res = r.renderForward(lmg._params(lmg.traj_perturbed(p)), cams[0])
    target = res.render.reshape(SH, SW, 3).clone()
    td = r.expectedDepth(res, 0.2).reshape(SH, SW) * 1.1
    kw, step_kw = {}, {}
    if variant == "mcmc":
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=int(lmg.SN * 1.2)))
    elif variant == "antialiased":
        r.setAntialiased(True)
    elif variant == "loss_mask":
        step_kw = dict(lossMask=lmg._half_mask())
    else:
        from gaussiansplattingmlx_amd.absgrad import AbsGradConfig
        kw = dict(absgrad=AbsGradConfig(), densify=True)
    tr, model = lmg._trainer(r, p, depth=DepthConfig(mode="expected", weight=(1.0, 0.01)), **kw)
    before = model.arena.clone()
    loss = tr.trainStep(cams[0], target, viewKey=0, targetDepth=td, **step_kw)
    assert np.isfinite(float(loss[0])) and float(loss[3]) > 0
    assert bool(torch.isfinite(model.arena[: model.numel]).all()) and not torch.equal(model.arena, before)


# ------------------------------------------------------------------------------------------------------------ what it is for
def _layer(cam, z, jitter):
    """16 x 16 blobs of one colour on the image's 4-pixel grid at camera depths z (an array, or one number)."""
    fx, fy = 0.9 * SW, 0.9 * SW * 1.02
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    n = i.size
    px, py = 2.0 + 4.0 * j.reshape(-1) + jitter[0], 2.0 + 4.0 * i.reshape(-1) + jitter[1]
    z = np.broadcast_to(np.asarray(z, np.float64), (n,))
    pc = np.stack([(px - SW / 2) * z / fx, (py - SH / 2) * z / fy, z, np.ones(n)], 1)
    rot = np.zeros((n, 4))
    rot[:, 0] = 1.0
    p = dict(xyz=(pc @ cam.c2w.T)[:, :3], features_dc=np.full((n, 1, 3), 1.0), features_rest=np.zeros((n, 24, 3)),
             scales=np.log(0.05 * z)[:, None].repeat(3, 1), rotation=rot, opacity=np.full(n, 1.0))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


def test_a_depth_prior_pulls_a_displaced_layer_back():
    """A layer of blobs of one colour at depth 4 in front of one camera: the training view is a uniform colour, which any depth
    renders alike.  The model starts with every blob moved along its view ray to a depth in [3, 5] (its size scaled with it, so
    that the picture stays what it was).  Sixty steps with DepthConfig(mode="expected") on the truth's expected depth against
    sixty without: the mean absolute error of expectedDepth against the truth, over the truth's pixels."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    rng = np.random.default_rng(5)
    cam = Camera(SW, SH, 0.9 * SW, 0.9 * SW * 1.02, look_at_c2w([2.2, -2.6, 1.7]))
    jitter = rng.uniform(-0.5, 0.5, (2, 256))
    truth = _layer(cam, 4.0, jitter)
    start = _layer(cam, rng.uniform(3.0, 5.0, 256), jitter)
    r = _renderer(SW, SH)
    res = r.renderForward(lmg._params(truth), cam)
    target = res.render.reshape(SH, SW, 3).clone()
    td = r.expectedDepth(res, 0.5).reshape(SH, SW).clone()
    seen = td > 0
    assert float(seen.float().mean()) > 0.9 and float((td[seen] - 4.0).abs().max()) < 0.2
    assert float(target[seen].std()) < 0.1                                    # a uniform colour

    def error(rr, params):
        e = rr.expectedDepth(rr.renderForward(params, cam), 0.05).reshape(SH, SW)
        return float((e - td)[seen].abs().mean())

    out = {}
    for with_depth in (True, False):
        rr = _renderer(SW, SH)
        tr, model = lmg._trainer(rr, start, **(dict(depth=DepthConfig(mode="expected", weight=1.0)) if with_depth else {}))
        e0 = error(rr, model.getParams())
        for _ in range(60):
            loss = tr.trainStep(cam, target, viewKey=0, **(dict(targetDepth=td) if with_depth else {}))
        assert np.isfinite(float(loss[0])) and bool(torch.isfinite(model.arena[: model.numel]).all())
        out[with_depth] = (e0, error(rr, model.getParams()))
    print(f"mean |expected depth - truth| over the layer: start {out[True][0]:.4g}; after 60 steps with the depth term "
          f"{out[True][1]:.4g}, without {out[False][1]:.4g}")
    assert abs(out[True][0] - out[False][0]) < 1e-5 and out[True][0] > 0.1
    assert out[True][1] < out[True][0] and out[True][1] < out[False][1], out
