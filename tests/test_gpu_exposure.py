"""Per-view exposure compensation on the device (include/gsplat.h gs_set_exposure / gs_apply_exposure,
GaussianTrainer(exposure_opt=True)) against the oracle's loss composed with the numpy restatement (tests/exposure_numpy.py).

Bars, fixed before the first run on the card:
  - identity exposure: the loss[4] and the cotangent are the plain loss's, np.array_equal (the kernels' fmaf order makes
    A r + b = r and A^T g = g exact for A = I, b = 0);
  - loss: 2e-6 absolute of the float32 composed oracle (test_gpu_parity.test_loss_forward_backward's bar);
  - cotangent and the 12-component gradient: 1e-3 relative to the largest component (the project's gradient bar);
  - the gradient's distance from the float64 composed oracle: at most twice the float32 composed oracle's own distance, with a
    floor of 2e-7 of the largest component (both are float32 computations of g that round differently; measured on this
    scene: the float32 oracle is 3.0e-8 away, 2e-7 is ~3 float32 ulps of the result);
  - finite differences: float64 central differences of the composed oracle loss at h = 1e-6, 1e-3 relative.  Step-size study
    (this file's scene, 152 x 200, the float64 oracle alone; largest deviation from the analytic VJP, relative to its largest
    component):
        h = 1e-2  9.1e-4      h = 1e-4  9.1e-5      h = 1e-6  1.1e-8
        h = 3e-3  4.2e-4      h = 3e-5  8.4e-5      h = 1e-7  1.1e-7
        h = 1e-3  3.1e-4      h = 1e-5  3.7e-5
    The L1 term's kinks (|c - G| at c = G) make larger steps cross pixels whose sign flips; below 1e-6 the float64 loss's
    rounding grows as 1 / h.  h = 1e-6 sits at the minimum;
  - recovery: 300 Adam steps on M alone at exposureLearningRate(t, 300) from the identity.  The same loop in numpy on the
    float32 oracle ends 6.5e-4 (max norm) from M* (100 steps: 1.5e-3, 200: 8.3e-4, 400: 8.7e-4 -- Adam without bias correction
    oscillates at ~lr near the optimum); bar 5e-3;
  - trajectories: test_gpu_trajectory's bars for the model; the exposures no further from the float32 loop than twice the
    float64 loop's distance plus 1e-6 (one float32 ulp of an O(1) entry per Adam step of the ten).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
LOSS_BAR, GRAD_BAR, FD_H, RECOVERY_BAR = 2e-6, 1e-3, 1e-6, 5e-3


def _load(name):
    spec = importlib.util.spec_from_file_location("_expog_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


en = _load("exposure_numpy")
traj = _load("test_gpu_trajectory")


def _renderer(W, H, aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, (16, 16), False, antialiased=aa)


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _images(H, W, seed=43):
    rng = np.random.default_rng(seed)
    ren = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    tgt = np.clip(ren + rng.normal(0, 0.15, ren.shape), 0, 1).astype(np.float32)
    depth = dict(rd=rng.uniform(1, 4, (H, W)).astype(np.float32), td=rng.uniform(1, 4, (H, W)).astype(np.float32),
                 mask=rng.uniform(size=(H, W)) > 0.5)
    return ren, tgt, depth


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _loss(r, ren, tgt, depth=None, key=None):
    kw = {}
    if depth is not None:
        kw = dict(renderDepth=_dev(depth["rd"]), targetDepth=_dev(depth["td"]), depthMask=_dev(depth["mask"]), lambda_depth=0.3)
    lo, gc, _ = r.lossForwardBackward(ren, tgt, 0.2, targetKey=key, **kw)
    return _np(lo).copy(), _np(gc).copy()


def _exposure(M):
    return _dev(np.asarray(M, np.float32).reshape(12)), torch.full((12,), float("nan"), device="cuda")


# ------------------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("H,W", [(152, 200), (37, 53), (800, 800)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_identity_exposure_is_the_plain_loss(oracle64, H, W, with_depth):
    r = _renderer(W, H)
    ren, tgt, depth = _images(H, W)
    dep = depth if with_depth else None
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    want = _loss(r, ren_d, tgt_d, dep)
    M, grad = _exposure(en.IDENTITY)
    r.setExposure(M, grad)
    try:
        for key in (None, "view", "view"):          # target cache off, filling, reading
            got = _loss(r, ren_d, tgt_d, dep, key)
            assert np.array_equal(got[0], want[0]), (key, got[0], want[0])
            assert np.array_equal(got[1], want[1]), key
        g = _np(grad).copy()
    finally:
        r.setExposure(None, None)
    assert torch.equal(ren_d, _dev(ren))            # the render is not written
    if (H, W) == (152, 200):
        kw = dict(renderDepth=depth["rd"], targetDepth=depth["td"], depthMask=depth["mask"], lambdaDepth=0.3) if with_depth else {}
        _, _, dM, _ = en.composed(oracle64, ren, tgt, en.IDENTITY, 0.2, **kw)
        assert _rel(g, dM) <= GRAD_BAR, (g, dM)


def test_null_is_off():
    H, W = 120, 160
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W, 3)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    want = _loss(r, ren_d, tgt_d)
    M, grad = _exposure(en.random_exposure(np.random.default_rng(1)))
    r.setExposure(M, grad)
    exposed = _loss(r, ren_d, tgt_d)
    r.setExposure(None, None)
    assert not np.array_equal(exposed[0], want[0])
    grad.fill_(12345.0)
    got = _loss(r, ren_d, tgt_d)
    torch.cuda.synchronize()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert bool((grad == 12345.0).all())
    import ctypes as C
    from gaussiansplattingmlx_amd import _lib
    for a, b in ((M, None), (None, grad)):
        with pytest.raises(ValueError):
            r.setExposure(a, b)
        rc = r.lib.gs_set_exposure(r.ctx, None if a is None else C.c_void_p(a.data_ptr()),
                                   None if b is None else C.c_void_p(b.data_ptr()))
        assert _lib.STATUS.get(rc) == "GS_ERR_INVALID_ARG"
    with pytest.raises(ValueError):
        r.setExposure(torch.zeros(11, device="cuda"), torch.zeros(11, device="cuda"))
    with pytest.raises(ValueError):
        r.setExposure(torch.zeros(12, device="cuda", dtype=torch.float64), torch.zeros(12, device="cuda"))
    got = _loss(r, ren_d, tgt_d)                    # the refused calls left the ctx off
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("with_depth", [False, True])
def test_random_exposure_matches_the_composed_oracle(oracle32, oracle64, with_depth):
    H, W = 152, 200
    r = _renderer(W, H)
    ren, tgt, depth = _images(H, W)
    Mh = en.random_exposure(np.random.default_rng(5))
    M, grad = _exposure(Mh)
    r.setExposure(M, grad)
    try:
        lo, cot = _loss(r, _dev(ren), _dev(tgt), depth if with_depth else None)
        g = _np(grad).copy()
    finally:
        r.setExposure(None, None)
    kw = dict(renderDepth=depth["rd"], targetDepth=depth["td"], depthMask=depth["mask"], lambdaDepth=0.3) if with_depth else {}
    l32, dr32, dM32, _ = en.composed(oracle32, ren, tgt, Mh, 0.2, **kw)
    _, dr64, dM64, _ = en.composed(oracle64, ren, tgt, Mh, 0.2, **kw)
    assert abs(float(lo[0]) - l32) <= LOSS_BAR, (lo, l32)
    assert _rel(cot, dr32) <= GRAD_BAR
    assert _rel(g, dM64) <= GRAD_BAR, (g, dM64)
    scale = np.abs(dM64).max()
    d_gpu, d_32 = np.abs(g - dM64).max(), np.abs(dM32 - dM64).max()
    assert d_gpu <= max(2.0 * d_32, 2e-7 * scale), (d_gpu, d_32, scale)


def test_gradient_against_oracle_finite_differences(oracle64):
    H, W = 152, 200
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W)
    Mh = en.random_exposure(np.random.default_rng(5))
    M, grad = _exposure(Mh)
    r.setExposure(M, grad)
    try:
        _loss(r, _dev(ren), _dev(tgt))
        g = _np(grad).copy()
    finally:
        r.setExposure(None, None)
    M64 = Mh.astype(np.float64)
    fd = np.empty(12)
    for k in range(12):
        Mp, Mm = M64.copy(), M64.copy()
        Mp[k] += FD_H
        Mm[k] -= FD_H
        fd[k] = (en.composed(oracle64, ren, tgt, Mp)[0] - en.composed(oracle64, ren, tgt, Mm)[0]) / (2 * FD_H)
    assert _rel(g, fd) <= GRAD_BAR, (g, fd)


@pytest.mark.parametrize("H,W", [(152, 200), (37, 53)])
def test_repeated_calls_give_the_same_bits(H, W):
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W, 8)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    M, grad = _exposure(en.random_exposure(np.random.default_rng(2)))
    r.setExposure(M, grad)
    try:
        first = None
        for key in (None, None, "view", "view", "view", None):     # cache off, filling, reading, off again
            lo, cot = _loss(r, ren_d, tgt_d, key=key)
            got = (lo, cot, _np(grad).copy())
            if first is None:
                first = got
            assert all(np.array_equal(a, b) for a, b in zip(got, first)), key
    finally:
        r.setExposure(None, None)


def test_apply_exposure():
    r = _renderer(64, 48)
    rng = np.random.default_rng(4)
    Mh = en.random_exposure(rng)
    M = _dev(Mh)
    for n in (4096, 1001, 3):                      # four-pixel groups and the tail
        img = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        got = _np(r.applyExposure(_dev(img), M))
        assert np.abs(got - en.apply(Mh, img)).max() <= 1e-6
        assert np.array_equal(_np(r.applyExposure(_dev(img), _dev(en.IDENTITY))), img)
        x = _dev(img)
        out = r.applyExposure(x, M, out=x)         # in place
        assert out.data_ptr() == x.data_ptr() and np.array_equal(_np(x), got)
    img = rng.uniform(0, 1, (1001, 3)).astype(np.float32)
    x = _dev(img)
    y = torch.empty_like(x)
    r.applyExposure(x[1:], M, out=y[1:])           # 12-byte offsets: the unaligned path
    assert np.array_equal(_np(y[1:]), _np(r.applyExposure(_dev(img[1:]), M)))
    with pytest.raises(ValueError):
        r.applyExposure(x, torch.zeros(9, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ training
def test_recovery_renderer_loop():
    import ctypes as C
    from gaussiansplattingmlx_amd.renderer import _p
    from gaussiansplattingmlx_amd.trainer import exposureLearningRate
    H, W, steps = 64, 48, 300
    r = _renderer(W, H)
    rng = np.random.default_rng(43)
    img = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    Ms = en.random_exposure(np.random.default_rng(9))
    ren, tgt = _dev(img), _dev(en.apply(Ms, img, np.float32))
    E = _dev(en.IDENTITY.copy())
    grad, m, v = (torch.zeros(12, device="cuda") for _ in range(3))
    r.setExposure(E, grad)
    try:
        for t in range(steps):
            r.lossForwardBackward(ren, tgt, 0.2, targetKey="v")
            r._check(r.lib.gs_adam_step(r.ctx, 12, _p(E), _p(grad), _p(m), _p(v), 1, (C.c_longlong * 1)(12),
                                        (C.c_float * 1)(exposureLearningRate(t, steps)), C.c_float(0.9), C.c_float(0.999),
                                        C.c_float(1e-15), C.c_float(1.0)))
    finally:
        r.setExposure(None, None)
    err = np.abs(_np(E) - Ms).max()
    assert err <= RECOVERY_BAR, (err, _np(E), Ms)


def _exposure_oracle_loop(o, p0, cams, targets, W, H, steps=traj.STEPS):
    """test_gpu_trajectory._oracle_loop with each view's exposure: the loss of apply(E_v, render), the render's cotangent
    A^T g, and a float32 (or float64) numpy Adam on E_v at exposureLearningRate."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, exposureLearningRate, getLearningRates
    dt = o.dtype
    p = {k: v.astype(dt).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    E = np.tile(en.IDENTITY.astype(dt), (len(cams), 1))
    Em, Ev = np.zeros_like(E), np.zeros_like(E)
    b1, b2, eps, one = dt.type(0.9), dt.type(0.999), dt.type(1e-15), dt.type(1)
    z = np.zeros(W * H, dt)
    losses = []
    for it in range(steps):
        vi = it % len(cams)
        cam = cams[vi].as_dict()
        fw = o.render_forward(p, cam, W, H, 16, 16, 4)
        ren = fw["color"].reshape(H, W, 3)
        loss, dr, dM, _ = en.composed(o, ren, targets[vi].astype(dt), E[vi])
        g = o.render_backward(p, cam, W, H, 16, 16, 4, fw, dr.astype(dt).reshape(-1, 3), z, z)
        losses.append(loss)
        lr = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
        for k in KEYS:
            gk = np.asarray(g[k], dt).reshape(p[k].shape)
            m[k] = b1 * m[k] + (one - b1) * gk
            v[k] = b2 * v[k] + (one - b2) * gk * gk
            p[k] = (p[k] - dt.type(lr[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
        gE = dM.astype(dt)
        Em[vi] = b1 * Em[vi] + (one - b1) * gE
        Ev[vi] = b2 * Ev[vi] + (one - b2) * gE * gE
        E[vi] = (E[vi] - dt.type(exposureLearningRate(it, traj.TOTAL)) * Em[vi] / (np.sqrt(Ev[vi]) + eps)).astype(dt)
    return losses, p, m, v, E


def _exposure_scene(W=160, H=120, N=3000):
    from gaussiansplattingmlx_amd.scenes import perturb
    p0, cams = traj._scene(71, N, W, H, 0.06)
    tp = perturb(p0, 5, 0.1)
    Ms = [en.random_exposure(np.random.default_rng(20 + i)) for i in range(len(cams))]
    return p0, cams, tp, Ms


@pytest.mark.parametrize("variant", ["fused", "unfused"])
def test_train_trajectory_matches_the_composed_oracle_loop(oracle32, oracle64, variant):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel, PARAM_ORDER, getLearningRates
    W, H, N = 160, 120, 3000
    p0, cams, tp, Ms = _exposure_scene(W, H, N)
    targets = [en.apply(Ms[i], oracle32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3), np.float32)
               for i, c in enumerate(cams)]
    want_l, want_p, want_m, want_v, want_E = _exposure_oracle_loop(oracle32, p0, cams, targets, W, H)
    ref_l, ref_p, _, _, ref_E = _exposure_oracle_loop(oracle64, p0, cams, targets, W, H)
    r = _renderer(W, H)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, fuse_adam=(variant == "fused"),
                         exposure_opt=True, n_views=len(cams))
    tg = [_dev(t) for t in targets]
    got_l = []
    for it in range(traj.STEPS):
        vi = it % len(cams)
        got_l.append(float(tr.trainStep(cams[vi], tg[vi], viewKey=vi)[0]))
    assert r.stats()["overflow"] == 0 and tr.forwardMisses == 0
    Nm = model.N
    got_p = {k: _np(model.getParams()[k]).copy() for k in KEYS}
    got_m = {k: _np(model._carve(model.m, Nm)[k]).copy() for k in KEYS}
    got_v = {k: _np(model._carve(model.v, Nm)[k]).copy() for k in KEYS}
    report = {}
    traj._compare("param", got_p, want_p, p0, report)
    traj._compare("m", got_m, want_m, p0, report)
    traj._compare("v", got_v, want_v, p0, report)
    traj._compare("oracle32_vs_64.param", {k: ref_p[k] for k in KEYS}, want_p, p0, report)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    assert got_l[-1] < got_l[0] and dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        for tag in ("m", "v"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = report[f"param.{k}"], report[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * traj.STEPS * 1.01 + 1e-6, (k, e)
    got_E = tr.exposures().reshape(len(cams), 12)
    d_hip, d_64 = np.abs(got_E - want_E).max(), np.abs(np.asarray(ref_E, np.float64) - want_E).max()
    assert d_hip <= 2.0 * d_64 + 1e-6, (d_hip, d_64, got_E, want_E)
    assert np.abs(got_E - en.IDENTITY).max() > 1e-3           # the exposures trained


def _composition_trainer(kind):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams, tp, Ms = _exposure_scene(W, H, N)
    r = _renderer(W, H, aa=(kind == "antialiased"))
    tparams = {k: _dev(v) for k, v in tp.items()}
    targets = [r.applyExposure(r.renderForward(tparams, c).render, _dev(Ms[i])).clone() for i, c in enumerate(cams)]
    model = GaussModel(p0, r.device)
    kw = dict(iterationCount=1000, densify=False, exposure_opt=True, n_views=len(cams))
    if kind == "pose":
        kw["pose_opt"] = True
    elif kind == "mcmc":
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw.update(strategy="mcmc", mcmc=MCMCConfig(cap_max=2 * N))
    return GaussianTrainer(model, r, **kw), model, cams, targets


@pytest.mark.parametrize("kind", ["pose", "mcmc", "antialiased"])
def test_composes_with_the_other_features(kind):
    tr, model, cams, targets = _composition_trainer(kind)
    losses = [float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]) for i in range(30)]
    assert np.isfinite(losses).all() and bool(torch.isfinite(model.arena).all())
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    E = tr.exposures()
    assert np.isfinite(E).all()
    assert all(np.abs(E[v].reshape(12) - en.IDENTITY).max() > 1e-3 for v in range(3)), E
    if kind == "pose":
        assert np.isfinite(tr.poseCorrections()).all()


def test_trainer_state():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams, tp, Ms = _exposure_scene(W, H, N)
    r = _renderer(W, H)
    tparams = {k: _dev(v) for k, v in tp.items()}
    targets = [r.renderForward(tparams, c).render.clone() for c in cams]
    ren, tgt, _ = _images(H, W, 12)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    plain = _loss(r, ren_d, tgt_d)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, exposure_opt=True, n_views=4)
    for i in range(6):                              # views 0 .. 2 only
        tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)
    assert r._exposure == (None, None)
    got = _loss(r, ren_d, tgt_d)                    # the ctx's exposure was cleared behind the step
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    E = tr.exposures()
    assert E.shape == (4, 3, 4) and E.dtype == np.float32
    assert np.array_equal(E[3].reshape(12), en.IDENTITY)             # never visited
    assert not bool(tr._expo_m[3].any()) and not bool(tr._expo_v[3].any())
    assert all(np.abs(E[v].reshape(12) - en.IDENTITY).max() > 0 for v in range(3))
    # exposedRender: the render under the view's exposure
    x = _np(tr.exposedRender(ren_d, 1))
    assert np.abs(x - en.apply(E[1].reshape(12), ren)).max() <= 1e-6
    # a step that raises still clears the exposure
    seen = []

    def boom(*a, **k):
        seen.append(r._exposure[0] is not None)
        raise RuntimeError("boom")
    tr._trainStep = boom
    with pytest.raises(RuntimeError):
        tr.trainStep(cams[0], targets[0], viewKey=0)
    del tr._trainStep
    assert seen == [True] and r._exposure == (None, None)
    got = _loss(r, ren_d, tgt_d)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    # viewKey refusals, before the step touches anything
    before = tr.exposures().copy()
    it = tr.iteration
    for bad in (None, 4, -1, 1.5, [0]):
        with pytest.raises(ValueError):
            tr.trainStep(cams[0], targets[0], viewKey=bad)
    assert tr.iteration == it and np.array_equal(tr.exposures(), before) and r._exposure == (None, None)
    with pytest.raises(ValueError):
        tr.exposedRender(ren_d, 7)
