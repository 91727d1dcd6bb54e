"""Per-view bilateral grid colour correction on the device (include/gsplat.h gs_set_bilateral_grid / gs_apply_bilateral_grid,
GaussianTrainer(bilateral_grid=True)) against the oracle's loss composed with the numpy restatement
(tests/bilateral_grid_numpy.py), and against exposure compensation, which a constant grid is.

Bars, fixed before the first run on the card:
  - identity grid: the loss[4] and the cotangent are the plain loss's, np.array_equal (every lerp of equal values is
    fmaf(t, 0, a) = a, the identity M's fmaf order gives r and g back, and dgray = s (grid_l - 1) with s = 0 adds 0);
  - constant grid M: the loss[4] and the cotangent are gs_set_exposure(M)'s, np.array_equal (the slice returns M exactly,
    P_hi - P_lo = 0, the same expo_apply / expo_vjp); the node-summed gradient within 1e-4 of the largest component of
    exposure's (float32 pixel sums against exposure's float64 ones: ~1e-7 relative per partial sum, 1e-4 leaves three orders);
  - random smooth grids: loss within 2e-6 of the float32 composed oracle (test_gpu_parity's loss bar); cotangent and grid
    gradient within 1e-3 relative to the largest component of the float64 composed oracle (the project's gradient bar);
  - finite differences: float64 central differences of the composed oracle loss (+ tv_weight TV) at h = 1e-6, the step the
    exposure study found best on this scene size, 1e-3 relative;
  - determinism: the loss, the cotangent and the gradient of repeated calls, with the target cache off, filling and
    reading, have the same bits;
  - apply op: 1e-6 absolute of the numpy restatement in float32 (its emulated fmaf is at most an ulp off), the identity
    exact, in place the same bits as out of place;
  - fit: 200 Adam steps (lr 0.01, tv_weight 0) on a grid from the identity toward the images of a known smooth grid at
    64 x 48; the same loop in numpy on the float32 oracle gives a reference L1 of the corrected image; the device's final L1
    at most 1.5 x the numpy loop's + 1e-4, and both below a third of the L1 at the start;
  - trajectories: test_gpu_trajectory's bars for the model; the grids no further from the float32 loop than twice the float64
    loop's distance plus 1e-6 (one float32 ulp of an O(1) entry per Adam step of the ten).
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
LOSS_BAR, GRAD_BAR, FD_H, SUM_BAR = 2e-6, 1e-3, 1e-6, 1e-4
DEFAULT = (16, 16, 8)


def _load(name):
    spec = importlib.util.spec_from_file_location("_bgg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bg = _load("bilateral_grid_numpy")
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


def _grid(G):
    G = _dev(np.asarray(G, np.float32))
    return G, torch.full_like(G, float("nan"))


def _okw(depth, with_depth):
    return dict(renderDepth=depth["rd"], targetDepth=depth["td"], depthMask=depth["mask"], lambdaDepth=0.3) if with_depth else {}


# ------------------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("H,W", [(800, 800), (152, 200), (11, 37)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_identity_grid_is_the_plain_loss(H, W, with_depth):
    r = _renderer(W, H)
    ren, tgt, depth = _images(H, W)
    dep = depth if with_depth else None
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    want = _loss(r, ren_d, tgt_d, dep)
    G, grad = _grid(bg.identity(DEFAULT))
    r.setBilateralGrid(G, grad)
    try:
        for key in (None, "view", "view"):          # target cache off, filling, reading
            got = _loss(r, ren_d, tgt_d, dep, key)
            assert np.array_equal(got[0], want[0]), (key, got[0], want[0])
            assert np.array_equal(got[1], want[1]), key
        g = _np(grad).copy()
    finally:
        r.setBilateralGrid(None, None)
    assert torch.equal(ren_d, _dev(ren))            # the render is not written
    assert np.isfinite(g).all()


@pytest.mark.parametrize("H,W", [(152, 200), (11, 37)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_constant_grid_is_the_exposure(H, W, with_depth):
    r = _renderer(W, H)
    ren, tgt, depth = _images(H, W, 7)
    dep = depth if with_depth else None
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    Mh = en.random_exposure(np.random.default_rng(3))
    M, mgrad = _dev(Mh), torch.zeros(12, device="cuda")
    r.setExposure(M, mgrad)
    try:
        want = _loss(r, ren_d, tgt_d, dep)
        dM = _np(mgrad).copy()
    finally:
        r.setExposure(None, None)
    for shape in (DEFAULT, (2, 2, 2), (5, 3, 4)):
        G, grad = _grid(bg.constant(Mh, shape))
        r.setBilateralGrid(G, grad, shape, 10.0)
        try:
            got = _loss(r, ren_d, tgt_d, dep)
            g = _np(grad).copy()
        finally:
            r.setBilateralGrid(None, None)
        assert np.array_equal(got[0], want[0]), (shape, got[0], want[0])
        assert np.array_equal(got[1], want[1]), shape
        s = g.reshape(-1, 12).astype(np.float64).sum(0)
        assert np.abs(s - dM).max() <= SUM_BAR * np.abs(dM).max(), (shape, s, dM)


@pytest.mark.parametrize("shape", [DEFAULT, (2, 2, 2), (5, 3, 4)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_random_grid_matches_the_composed_oracle(oracle32, oracle64, shape, with_depth):
    H, W = 152, 200
    r = _renderer(W, H)
    ren, tgt, depth = _images(H, W)
    Gh = bg.random_grid(np.random.default_rng(5), shape)
    G, grad = _grid(Gh)
    r.setBilateralGrid(G, grad, shape, 10.0)
    try:
        lo, cot = _loss(r, _dev(ren), _dev(tgt), depth if with_depth else None)
        g = _np(grad).copy()
    finally:
        r.setBilateralGrid(None, None)
    kw = _okw(depth, with_depth)
    l32, dr32, _, _ = bg.composed(oracle32, ren, tgt, Gh, shape, 10.0, **kw)
    _, dr64, dG64, _ = bg.composed(oracle64, ren, tgt, Gh, shape, 10.0, **kw)
    assert abs(float(lo[0]) - l32) <= LOSS_BAR, (lo, l32)
    assert _rel(cot, dr32) <= GRAD_BAR and _rel(cot, dr64) <= GRAD_BAR
    assert _rel(g, dG64) <= GRAD_BAR, _rel(g, dG64)


def test_gradient_against_oracle_finite_differences(oracle64):
    H, W, shape, tvw = 152, 200, (5, 3, 4), 10.0
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W)
    Gh = bg.random_grid(np.random.default_rng(6), shape)
    G, grad = _grid(Gh)
    r.setBilateralGrid(G, grad, shape, tvw)
    try:
        _loss(r, _dev(ren), _dev(tgt))
        g = _np(grad).copy()
    finally:
        r.setBilateralGrid(None, None)
    G64 = Gh.astype(np.float64)

    def L(Gx):
        return bg.composed(oracle64, ren, tgt, Gx, shape)[0] + tvw * bg.tv(Gx, shape)
    rng = np.random.default_rng(9)
    idx = [tuple(rng.integers(0, n) for n in G64.shape) for _ in range(12)] + [(1, 2, 1, k) for k in range(12)]
    fd, an = np.empty(len(idx)), np.empty(len(idx))
    for n, i in enumerate(idx):
        Gp, Gm = G64.copy(), G64.copy()
        Gp[i] += FD_H
        Gm[i] -= FD_H
        fd[n], an[n] = (L(Gp) - L(Gm)) / (2 * FD_H), g[i]
    assert np.abs(fd - an).max() <= GRAD_BAR * np.abs(g).max(), (fd, an)


@pytest.mark.parametrize("H,W", [(152, 200), (11, 37)])
def test_repeated_calls_give_the_same_bits(H, W):
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W, 8)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    G, grad = _grid(bg.random_grid(np.random.default_rng(2), DEFAULT))
    r.setBilateralGrid(G, grad)
    try:
        first = None
        for key in (None, None, "view", "view", "view", None):     # cache off, filling, reading, off again
            lo, cot = _loss(r, ren_d, tgt_d, key=key)
            got = (lo, cot, _np(grad).copy())
            if first is None:
                first = got
            assert all(np.array_equal(a, b) for a, b in zip(got, first)), key
    finally:
        r.setBilateralGrid(None, None)


def test_null_is_off_and_exclusive_with_exposure():
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd.renderer import _p
    H, W = 120, 160
    r = _renderer(W, H)
    ren, tgt, _ = _images(H, W, 3)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    want = _loss(r, ren_d, tgt_d)
    G, grad = _grid(bg.random_grid(np.random.default_rng(1), DEFAULT))
    r.setBilateralGrid(G, grad)
    graded = _loss(r, ren_d, tgt_d)
    r.setBilateralGrid(None, None)
    assert not np.array_equal(graded[0], want[0])
    grad.fill_(12345.0)
    got = _loss(r, ren_d, tgt_d)
    torch.cuda.synchronize()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert bool((grad == 12345.0).all())

    def st(rc):
        return _lib.STATUS.get(rc)
    for a, b in ((G, None), (None, grad)):
        with pytest.raises(ValueError):
            r.setBilateralGrid(a, b)
        assert st(r.lib.gs_set_bilateral_grid(r.ctx, _p(a), _p(b), 16, 16, 8, C.c_float(10.0))) == "GS_ERR_INVALID_ARG"
    for shape, tv in (((1, 16, 8), 10.0), ((16, 65, 8), 10.0), ((16, 16, 33), 10.0), (DEFAULT, -1.0), (DEFAULT, float("nan"))):
        assert st(r.lib.gs_set_bilateral_grid(r.ctx, _p(G), _p(grad), *shape, C.c_float(tv))) == "GS_ERR_INVALID_ARG"
    with pytest.raises(ValueError):
        r.setBilateralGrid(torch.zeros(11, device="cuda"), torch.zeros(11, device="cuda"))
    got = _loss(r, ren_d, tgt_d)                    # the refused calls left the ctx off
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # exclusivity, both ways: the refused call leaves the other correction in place
    Mh = en.random_exposure(np.random.default_rng(4))
    M, mgrad = _dev(Mh), torch.zeros(12, device="cuda")
    r.setExposure(M, mgrad)
    exposed = _loss(r, ren_d, tgt_d)
    assert st(r.lib.gs_set_bilateral_grid(r.ctx, _p(G), _p(grad), 16, 16, 8, C.c_float(10.0))) == "GS_ERR_INVALID_ARG"
    assert np.array_equal(_loss(r, ren_d, tgt_d)[0], exposed[0])
    r.setExposure(None, None)
    r.setBilateralGrid(G, grad)
    assert st(r.lib.gs_set_exposure(r.ctx, _p(M), _p(mgrad))) == "GS_ERR_INVALID_ARG"
    assert np.array_equal(_loss(r, ren_d, tgt_d)[0], graded[0])
    r.setBilateralGrid(None, None)
    assert np.array_equal(_loss(r, ren_d, tgt_d)[0], want[0])


def test_apply_bilateral_grid():
    r = _renderer(64, 48)
    rng = np.random.default_rng(4)
    for shape, (H, W) in ((DEFAULT, (48, 64)), ((5, 3, 4), (37, 11)), ((2, 2, 2), (7, 5))):
        Gh = bg.random_grid(rng, shape)
        img = rng.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
        got = _np(r.applyBilateralGrid(_dev(img), _dev(Gh), shape))
        assert np.abs(got - bg.apply(Gh, img, shape)).max() <= 1e-6, shape
        assert np.array_equal(_np(r.applyBilateralGrid(_dev(img), _dev(bg.identity(shape)), shape)), img)
        x = _dev(img)
        out = r.applyBilateralGrid(x, _dev(Gh), shape, out=x)     # in place
        assert out.data_ptr() == x.data_ptr() and np.array_equal(_np(x), got)
    with pytest.raises(ValueError):
        r.applyBilateralGrid(_dev(img), torch.zeros(9, device="cuda"), (2, 2, 2))


# ------------------------------------------------------------------------------------------------------------ training
def _adam_np(p, g, m, v, lr):
    f = np.float32
    m[:] = f(0.9) * m + (f(1) - f(0.9)) * g
    v[:] = f(0.999) * v + (f(1) - f(0.999)) * g * g
    p[:] = p - (f(lr) * m) / (np.sqrt(v) + f(1e-15))


def test_fit_renderer_loop(oracle32):
    from gaussiansplattingmlx_amd.renderer import _p
    H, W, steps, lr, shape = 48, 64, 200, 0.01, (5, 3, 4)
    r = _renderer(W, H)
    rng = np.random.default_rng(43)
    img = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    Gs = bg.random_grid(np.random.default_rng(9), shape, 0.3)
    tgt = bg.apply(Gs, img, shape)
    ren_d, tgt_d = _dev(img), _dev(tgt)
    G = _dev(bg.identity(shape))
    grad, m, v = (torch.zeros_like(G) for _ in range(3))
    n = G.numel()
    r.setBilateralGrid(G, grad, shape, 0.0)
    try:
        for t in range(steps):
            r.lossForwardBackward(ren_d, tgt_d, 0.2, targetKey="v")
            r._check(r.lib.gs_adam_step(r.ctx, n, _p(G), _p(grad), _p(m), _p(v), 1, (C.c_longlong * 1)(n), (C.c_float * 1)(lr),
                                        C.c_float(0.9), C.c_float(0.999), C.c_float(1e-15), C.c_float(1.0)))
    finally:
        r.setBilateralGrid(None, None)
    Gn = bg.identity(shape).astype(np.float32)
    mn, vn = np.zeros_like(Gn), np.zeros_like(Gn)
    for t in range(steps):
        _, _, dG, _ = bg.composed(oracle32, img, tgt, Gn, shape)
        _adam_np(Gn, dG.astype(np.float32), mn, vn, lr)

    def l1(Gx):
        return float(np.abs(bg.apply(Gx, img, shape) - tgt).mean())
    start, dev_l1, np_l1 = l1(bg.identity(shape)), l1(_np(G)), l1(Gn)
    assert np_l1 < start / 3 and dev_l1 < start / 3, (start, dev_l1, np_l1)
    assert dev_l1 <= 1.5 * np_l1 + 1e-4, (dev_l1, np_l1)


def _grid_oracle_loop(o, p0, cams, targets, W, H, shape, lr, steps=traj.STEPS):
    """test_gpu_trajectory._oracle_loop with each view's grid: the loss of the render under G_v, the render's cotangent, and
    a float32 (or float64) numpy Adam on G_v at bilateralGridLearningRate (tv_weight 10)."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, bilateralGridLearningRate, getLearningRates
    dt = o.dtype
    p = {k: v.astype(dt).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    Gs = np.stack([bg.identity(shape).astype(dt)] * len(cams))
    Gm, Gv = np.zeros_like(Gs), np.zeros_like(Gs)
    b1, b2, eps, one = dt.type(0.9), dt.type(0.999), dt.type(1e-15), dt.type(1)
    z = np.zeros(W * H, dt)
    losses = []
    for it in range(steps):
        vi = it % len(cams)
        cam = cams[vi].as_dict()
        fw = o.render_forward(p, cam, W, H, 16, 16, 4)
        ren = fw["color"].reshape(H, W, 3)
        loss, dr, dG, _ = bg.composed(o, ren, targets[vi].astype(dt), Gs[vi], shape, 10.0)
        g = o.render_backward(p, cam, W, H, 16, 16, 4, fw, dr.astype(dt).reshape(-1, 3), z, z)
        losses.append(loss)
        lrs = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
        for k in KEYS:
            gk = np.asarray(g[k], dt).reshape(p[k].shape)
            m[k] = b1 * m[k] + (one - b1) * gk
            v[k] = b2 * v[k] + (one - b2) * gk * gk
            p[k] = (p[k] - dt.type(lrs[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
        gG = dG.astype(dt)
        Gm[vi] = b1 * Gm[vi] + (one - b1) * gG
        Gv[vi] = b2 * Gv[vi] + (one - b2) * gG * gG
        Gs[vi] = (Gs[vi] - dt.type(bilateralGridLearningRate(it, traj.TOTAL, lr)) * Gm[vi] / (np.sqrt(Gv[vi]) + eps)).astype(dt)
    return losses, p, m, v, Gs


def _grid_scene(W=160, H=120, N=3000):
    from gaussiansplattingmlx_amd.scenes import perturb
    p0, cams = traj._scene(71, N, W, H, 0.06)
    tp = perturb(p0, 5, 0.1)
    Gs = [bg.random_grid(np.random.default_rng(20 + i), DEFAULT) for i in range(len(cams))]
    return p0, cams, tp, Gs


@pytest.mark.parametrize("variant", ["fused", "unfused"])
def test_train_trajectory_matches_the_composed_oracle_loop(oracle32, oracle64, variant):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel, PARAM_ORDER, getLearningRates
    W, H, N, lr = 160, 120, 3000, 0.05
    p0, cams, tp, Gs = _grid_scene(W, H, N)
    targets = [bg.apply(Gs[i], oracle32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3), DEFAULT)
               for i, c in enumerate(cams)]
    want_l, want_p, want_m, want_v, want_G = _grid_oracle_loop(oracle32, p0, cams, targets, W, H, DEFAULT, lr)
    ref_l, ref_p, _, _, ref_G = _grid_oracle_loop(oracle64, p0, cams, targets, W, H, DEFAULT, lr)
    r = _renderer(W, H)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, fuse_adam=(variant == "fused"),
                         bilateral_grid=True, n_views=len(cams), bilateral_grid_lr=lr)
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
    lrs = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        for tag in ("m", "v"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = report[f"param.{k}"], report[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lrs[k] * traj.STEPS * 1.01 + 1e-6, (k, e)
    got_G = tr.bilateralGrids()
    d_hip, d_64 = np.abs(got_G - want_G).max(), np.abs(np.asarray(ref_G, np.float64) - want_G).max()
    assert d_hip <= 2.0 * d_64 + 1e-6, (d_hip, d_64)
    assert np.abs(got_G - bg.identity(DEFAULT)).max() > 1e-5         # the grids trained


def _composition_trainer(kind):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams, tp, Gs = _grid_scene(W, H, N)
    r = _renderer(W, H, aa=(kind == "antialiased"))
    tparams = {k: _dev(v) for k, v in tp.items()}
    targets = [r.applyBilateralGrid(r.renderForward(tparams, c).render, _dev(Gs[i])).clone() for i, c in enumerate(cams)]
    model = GaussModel(p0, r.device)
    kw = dict(iterationCount=1000, densify=False, bilateral_grid=True, n_views=len(cams), bilateral_grid_lr=0.05)
    if kind == "pose":
        kw["pose_opt"] = True
    elif kind == "mcmc":
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw.update(strategy="mcmc", mcmc=MCMCConfig(cap_max=2 * N))
    return GaussianTrainer(model, r, **kw), model, cams, targets


@pytest.mark.parametrize("kind", ["pose", "mcmc", "antialiased", "reload"])
def test_composes_with_the_other_features(kind):
    tr, model, cams, targets = _composition_trainer(kind)
    if kind == "reload":
        tr.referenceParamReload = True
    losses = [float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]) for i in range(30)]
    assert np.isfinite(losses).all() and bool(torch.isfinite(model.arena).all())
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    G = tr.bilateralGrids()
    assert np.isfinite(G).all()
    assert all(np.abs(G[v] - bg.identity(DEFAULT)).max() > 1e-4 for v in range(3))
    if kind == "pose":
        assert np.isfinite(tr.poseCorrections()).all()


def test_trainer_state():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams, tp, Gs = _grid_scene(W, H, N)
    r = _renderer(W, H)
    tparams = {k: _dev(v) for k, v in tp.items()}
    targets = [r.renderForward(tparams, c).render.clone() for c in cams]
    ren, tgt, _ = _images(H, W, 12)
    ren_d, tgt_d = _dev(ren), _dev(tgt)
    plain = _loss(r, ren_d, tgt_d)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, bilateral_grid=True, n_views=4,
                         bilateral_grid_shape=(5, 3, 4), bilateral_grid_lr=0.05)
    for i in range(6):                              # views 0 .. 2 only
        tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)
    assert r._bilateral == (None, None)
    got = _loss(r, ren_d, tgt_d)                    # the ctx's grid was cleared behind the step
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    G = tr.bilateralGrids()
    assert G.shape == (4, 3, 5, 4, 12) and G.dtype == np.float32
    assert np.array_equal(G[3], bg.identity((5, 3, 4)))             # never visited
    assert not bool(tr._bg_m[3].any()) and not bool(tr._bg_v[3].any())
    assert all(np.abs(G[v] - bg.identity((5, 3, 4))).max() > 0 for v in range(3))
    # only the visited view's grid moves
    before = tr.bilateralGrids().copy()
    tr.trainStep(cams[1], targets[1], viewKey=1)
    after = tr.bilateralGrids()
    assert not np.array_equal(after[1], before[1])
    assert all(np.array_equal(after[v], before[v]) for v in (0, 2, 3))
    # bilateralRender: the render under the view's grid
    x = _np(tr.bilateralRender(ren_d, 1))
    assert np.abs(x - bg.apply(after[1], ren, (5, 3, 4))).max() <= 1e-6
    # a step that raises still clears the grid
    seen = []

    def boom(*a, **k):
        seen.append(r._bilateral[0] is not None)
        raise RuntimeError("boom")
    tr._trainStep = boom
    with pytest.raises(RuntimeError):
        tr.trainStep(cams[0], targets[0], viewKey=0)
    del tr._trainStep
    assert seen == [True] and r._bilateral == (None, None)
    got = _loss(r, ren_d, tgt_d)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    # viewKey refusals, before the step touches anything
    before = tr.bilateralGrids().copy()
    it = tr.iteration
    for bad in (None, 4, -1, 1.5, [0]):
        with pytest.raises(ValueError):
            tr.trainStep(cams[0], targets[0], viewKey=bad)
    assert tr.iteration == it and np.array_equal(tr.bilateralGrids(), before) and r._bilateral == (None, None)
    with pytest.raises(ValueError):
        tr.bilateralRender(ren_d, 7)
