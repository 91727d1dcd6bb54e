"""The anti-aliased mode on the device (include/gsplat.h gs_set_antialiasing, GaussianRenderer(antialiased=True)) against the
oracle composed from the reference's ops in test_antialiasing_cpu.AAOracle (rho in float64, sigma(o) rho packed).

Tolerances were fixed before the first run on the card.  Images: the project's bar, 1e-4 L-inf, against the float64 composed
oracle.  Gradients: test_gpu_parity's metric, max |a - b| / max |b| per tensor, at 1e-3.  The pose gradient and the
finite-difference test: float64 central differences of the composed oracle's loss against the float32 kernels, at 5 % of the
largest component (the bar and the cause of test_gpu_pose_correction: the oracle's 3-sigma cull and integer radii make its
loss piecewise smooth).  Step sizes: h = 1e-4 for the raw parameters, in the plateau of this study (the float64 composed
oracle alone, _fd_scene, the opacity / scale_0 / xyz_0 of splat 7, the visible one with rho < 0.8 and the largest opacity
gradient; its chain rule gives 0.0030589, 0.0084885, -0.0097074):
    h = 1e-2   0.0030589   0.0084886  -0.0096794
    h = 1e-3   0.0030589   0.0084885  -0.0097074
    h = 1e-4   0.0030589   0.0084885  -0.0097074
    h = 1e-5   0.0030589   0.0084885  -0.0097074
    h = 1e-6   0.0030589   0.0084885  -0.0097074
and 1e-4 for the pose, the pose test's own study.  Energy: one splat of 0.3 px unblurred standard deviation, sigma(o) = 0.99, in front of the camera at depth 4.  The sum over
pixels of exp(-q / 2) is 2 pi sqrt(det Sigma_b) up to the grid's aliasing term (exp(-2 pi^2 0.39) = 5e-4 per axis).  The blend
drops alpha < 1/255.  With the mode on the splat's peak alpha is 0.99 x 0.09 / 0.39 = 0.23, and the cut falls at
q = 2 ln(255 x 0.23) = 8.1.  Outside it a continuous 2-D Gaussian keeps exp(-8.1 / 2) = 1.7 % of its mass, so the sum is at
least 0.56 x (1 - 0.017 - 0.001): inside the 5 % bar.  On the pixel grid (the splat's centre at a pixel corner) the float64
composed oracle gives 0.5588 against the target 0.5598.  With the mode off the peak is 0.99 (the blend's cap).  The cut at
q = 11.0 drops 0.4 %, so the sum is 0.99 x 2 pi x 0.39 x 0.996 = 2.42 (oracle: 2.4215), 4.3 x the mode's target and beyond
the 3 x bar.
Trajectories: test_gpu_trajectory's own loops, bars and scene, with AAOracle in place of the oracle.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd.camera import Camera, apply_pose_correction, look_at_c2w

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
IMG_BAR, GRAD_BAR, FD_BAR, FD_H = 1e-4, 1e-3, 5e-2, 1e-4


def _load(name):
    spec = importlib.util.spec_from_file_location("_aa_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_antialiasing_cpu")
traj = _load("test_gpu_trajectory")
AAOracle = cpu.AAOracle


def _renderer(W, H, tile=(16, 16), aa=True):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, tile, False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _parity_scene(W=160, H=120, N=3000):
    """test_gpu_trajectory's cloud with smaller splats (scale 0.03): rho from ~0.5 to 1 over the visible splats."""
    return traj._scene(71, N, W, H, 0.03)


def _step(r, params, cam, target):
    res = r.renderForward(params, cam)
    img, alpha, depth = res.render.clone(), res.alpha.clone(), res.depth.clone()
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    g = r.renderBackward(cot)
    return img, alpha, depth, float(loss[0]), {k: v.clone() for k, v in g.items()}


# ------------------------------------------------------------------------------------------------------------ the setter
def test_setter_refuses_bad_values_and_keeps_the_mode():
    from gaussiansplattingmlx_amd import _lib
    p, cams = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H)
    params = _dev(p)
    on = r.renderForward(params, cams[0]).render.clone()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    for bad in (2, -1, 255):
        assert r.lib.gs_set_antialiasing(r.ctx, bad) == invalid
        assert "gs_set_antialiasing" in r.lib.gs_last_error(r.ctx).decode()
    assert torch.equal(r.renderForward(params, cams[0]).render, on)          # still on
    r.setAntialiased(False)
    off = r.renderForward(params, cams[0]).render.clone()
    assert float((off - on).abs().max()) > 1e-3
    assert r.lib.gs_set_antialiasing(r.ctx, 2) == invalid
    assert torch.equal(r.renderForward(params, cams[0]).render, off)         # still off
    r.antialiased = True
    assert r.antialiased and torch.equal(r.renderForward(params, cams[0]).render, on)


def test_off_is_off():
    """A context that had the mode on and then off renders and differentiates like a fresh one, bit for bit (where the fresh
    one is itself run-to-run identical: the blend backward's float atomics are not on every scene)."""
    p, cams = _parity_scene()
    W, H = 160, 120
    params = _dev(p)
    fresh = _renderer(W, H, aa=False)
    target = fresh.renderForward(_dev(_perturbed(p)), cams[1]).render.clone()
    a = _step(fresh, params, cams[0], target)
    b = _step(fresh, params, cams[0], target)
    r = _renderer(W, H, aa=True)
    _step(r, params, cams[0], target)
    r.setAntialiased(False)
    c = _step(r, params, cams[0], target)
    for i in range(3):
        assert torch.equal(a[i], c[i]), i
    assert a[3] == c[3]
    for k in KEYS:
        if torch.equal(a[4][k], b[4][k]):
            assert torch.equal(a[4][k], c[4][k]), k
        else:
            assert torch.allclose(a[4][k], c[4][k], rtol=1e-5, atol=1e-7 * float(a[4][k].abs().max())), k


def test_backward_uses_its_forwards_mode():
    p, cams = _parity_scene()
    W, H = 160, 120
    params = _dev(p)
    r = _renderer(W, H)
    target = torch.zeros(H, W, 3, device="cuda")
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    want = {k: v.clone() for k, v in r.renderBackward(cot).items()}
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.setAntialiased(False)          # between the forward and its backward: changes nothing for that pair
    got = r.renderBackward(cot)
    for k in KEYS:
        assert _rel(_np(got[k]), _np(want[k])) <= 1e-5, k


# ------------------------------------------------------------------------------------------------------ forward parity
@pytest.mark.parametrize("variant", ["tiles16", "tiles16_untrimmed", "block_lists", "pose"])
def test_forward_matches_the_composed_oracle(oracle64, variant):
    p, cams = _parity_scene()
    W, H = 160, 120
    tile = (50, 38) if variant == "block_lists" else (16, 16)
    r = _renderer(W, H, tile)
    assert r.blockLists == (variant == "block_lists")
    if variant == "tiles16_untrimmed":
        r.setTuning(trim_rects=0)
    cam = cams[0]
    if variant == "pose":
        d = np.array([0.01, -0.02, 0.015, 0.05, -0.03, 0.04], np.float32)
        delta, grad = torch.as_tensor(d, device="cuda"), torch.zeros(6, device="cuda")
        r.setPoseCorrection(delta, grad)
        ocam = apply_pose_correction(cam, d)
    else:
        ocam = cam
    try:
        res = r.renderForward(_dev(p), cam, want_radii=True)
        img, alpha, depth, radii = _np(res.render), _np(res.alpha), _np(res.depth), _np(res.radii)
    finally:
        if variant == "pose":
            r.setPoseCorrection(None, None)
    fw = AAOracle(oracle64).render_forward(p, ocam.as_dict(), W, H, tile[0], tile[1], 4)
    assert np.abs(img.reshape(-1, 3) - fw["color"]).max() <= IMG_BAR
    assert np.abs(alpha.reshape(-1) - fw["alpha"]).max() <= IMG_BAR
    assert np.abs(depth.reshape(-1) - fw["depth"]).max() <= IMG_BAR * max(1.0, float(np.abs(fw["depth"]).max()))
    assert np.array_equal(radii > 0, fw["radii"] > 0)
    rho = fw["rho"][fw["radii"] > 0]
    assert rho.min() < 0.7                               # (the compensation matters on this scene)


# ----------------------------------------------------------------------------------------------------- gradient parity
@pytest.mark.parametrize("tile", [(16, 16), (50, 38)])
def test_gradients_match_the_composed_oracle(oracle64, tile):
    p, cams = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H, tile)
    cam = cams[0]
    o = AAOracle(oracle64)
    target = oracle64.render_forward(_perturbed(p), cam.as_dict(), W, H, tile[0], tile[1], 4)["color"].reshape(H, W, 3)
    _, _, _, loss, g = _step(r, _dev(p), cam, torch.as_tensor(target, dtype=torch.float32, device="cuda"))
    want_loss, fw, cot = cpu.aa_loss(o, p, cam.as_dict(), W, H, target, tile)
    z = np.zeros(W * H)
    want = o.render_backward(p, cam.as_dict(), W, H, tile[0], tile[1], 4, fw, cot.reshape(-1, 3), z, z)
    assert abs(loss - want_loss) <= 1e-5
    for k in KEYS:
        assert _rel(_np(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)) <= GRAD_BAR, (k, _rel(_np(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)))


def _perturbed(p):
    from gaussiansplattingmlx_amd.scenes import perturb
    return perturb(p, 5, 0.1)


def test_fused_adam_matches_backward_then_adam():
    """gs_render_backward_adam == gs_render_backward + gs_adam_step in the mode (test_gpu_parity's check, through the trainer)."""
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H)
    target = torch.rand(H, W, 3, device=r.device, generator=torch.Generator(device=r.device).manual_seed(3))
    out = {}
    for fuse in (False, True):
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse)
        for _ in range(3):
            tr.trainStep(cams[0], target)
        out[fuse] = (_np(model.arena).copy(), _np(model.m).copy(), _np(model.v).copy())
    start = _np(GaussModel(p, r.device).arena)
    a, b = out[True][0] - start, out[False][0] - start
    assert np.abs(b).max() > 0
    assert np.mean(np.abs(a - b) > 1e-3 * np.abs(b).max()) < 1e-3
    for k in (1, 2):
        ref = out[False][k]
        assert np.mean(np.abs(out[True][k] - ref) > 1e-3 * np.abs(ref).max()) < 1e-3, k


def test_pose_gradient_against_oracle_finite_differences(oracle64):
    W = H = 96
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    p = make_gaussians(300, "trained_like", 7)
    p["scales"] = (p["scales"] + 0.6).astype(np.float32)
    cam = Camera(W, H, 90.0, 90.0, look_at_c2w((3.0, -2.5, 2.0)))
    o = AAOracle(oracle64)
    r = _renderer(W, H)
    tgt = r.renderForward(_dev(make_gaussians(300, "trained_like", 8)), cam).render.clone()
    d0 = np.array([0.01, -0.008, 0.012, 0.03, -0.02, 0.025])
    delta, grad = torch.as_tensor(d0, dtype=torch.float32, device="cuda"), torch.zeros(6, device="cuda")
    r.setPoseCorrection(delta, grad)
    try:
        _step(r, _dev(p), cam, tgt)
    finally:
        r.setPoseCorrection(None, None)
    got = _np(grad).astype(np.float64)
    tnp = _np(tgt).astype(np.float64)
    d0 = _np(delta).astype(np.float64)

    def loss(d):
        return cpu.aa_loss(o, p, apply_pose_correction(cam, d).as_dict(), W, H, tnp)[0]
    fd = np.array([(loss(d0 + 1e-4 * e) - loss(d0 - 1e-4 * e)) / 2e-4 for e in np.eye(6)])
    assert np.abs(got - fd).max() <= FD_BAR * np.abs(fd).max(), (got, fd)


def test_gradients_against_oracle_finite_differences(oracle64):
    """Central differences of the float64 composed oracle's loss, independent of its hand-written chain rule, against the
    kernel's gradient: scale, rotation, opacity and xyz elements of the visible splats with the largest opacity gradients."""
    p, cam, W, H = cpu._fd_scene()
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    o = AAOracle(oracle64)
    c = cam.as_dict()
    tgt = oracle64.render_forward(make_gaussians(60, "trained_like", 4), c, W, H, 16, 16, 4)["color"].reshape(H, W, 3)
    r = _renderer(W, H)
    _, _, _, _, g = _step(r, _dev(p), cam, torch.as_tensor(tgt, dtype=torch.float32, device="cuda"))
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    fw = o.render_forward(p64, c, W, H, 16, 16, 4)
    go = _np(g["opacity"]).reshape(-1)
    vis = np.nonzero((fw["radii"] > 0) & (fw["rho"] < 0.8))[0]
    assert len(vis) >= 3
    pick = vis[np.argsort(-np.abs(go[vis]))[:3]]
    for k, cols in (("scales", (0, 2)), ("rotation", (0, 3)), ("opacity", (None,)), ("xyz", (0, 1))):
        gk_all = _np(g[k]).astype(np.float64)
        scale = np.abs(gk_all).max()
        for i in pick:
            for j in cols:
                idx = (i,) if j is None else (i, j)

                def L(d):
                    q = dict(p64); q[k] = p64[k].copy(); q[k][idx] += d
                    return cpu.aa_loss(o, q, c, W, H, tgt)[0]
                fd = (L(FD_H) - L(-FD_H)) / (2 * FD_H)
                gk = float(gk_all[idx])
                assert abs(gk - fd) <= FD_BAR * max(abs(fd), 1e-2 * scale), (k, idx, gk, fd)


# ------------------------------------------------------------------------------------------------------- energy, needles
def _one_splat(std_px, op, W=64, H=64, focal=60.0, depth=4.0, scales=None):
    K = 25
    s = np.log(std_px * depth / focal)
    p = dict(xyz=np.zeros((1, 3)), features_dc=np.full((1, 1, 3), 0.5), features_rest=np.zeros((1, K - 1, 3)),
             scales=np.array([scales if scales is not None else [s, s, s]]), rotation=np.array([[1.0, 0, 0, 0]]),
             opacity=np.array([np.log(op / (1 - op))]))
    cam = Camera(W, H, focal, focal, look_at_c2w([0.0, -depth, 0.0]))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, cam, W, H


def test_energy_of_a_sub_pixel_splat(oracle64):
    p, cam, W, H = _one_splat(0.3, 0.99)
    c = cam.as_dict()
    pr = oracle64.projection_forward(*oracle64.activations_forward(p["opacity"], p["scales"], p["rotation"])[1:],
                                     p["xyz"], np.concatenate([p["features_dc"], p["features_rest"]], 1), c["camCenter"],
                                     c["view"], c["proj"], c["fovX"], c["fovY"], c["focalX"], c["focalY"], W, H, 4)
    sig = 1 / (1 + np.exp(-float(p["opacity"][0])))
    u = pr["cov2d"][0] - 0.3 * np.eye(2)
    want = sig * 2 * np.pi * np.sqrt(np.linalg.det(u))
    assert 0.5 < want < 0.62 and abs(np.sqrt(u[0, 0]) - 0.3) < 0.01
    sums = {}
    for aa in (True, False):
        r = _renderer(W, H, aa=aa)
        sums[aa] = float(r.renderForward(_dev(p), cam).alpha.double().sum())
    assert abs(sums[True] - want) <= 0.05 * want, (sums, want)
    assert sums[False] > 3 * want, (sums, want)


def test_degenerate_needle_is_invisible():
    """A needle along the screen's x axis (two scales of exp(-60), whose squares are 0 in float32): the unblurred covariance
    is diag(a, 0) exactly, det Sigma = 0.  With the mode on it gets radius 0, no pairs and an exactly zero gradient; a
    second splat beside it is untouched.  With the mode off the needle renders (the blurred covariance is fine)."""
    needle, cam, W, H = _one_splat(0.3, 0.9, scales=[np.log(0.5), -60.0, -60.0])
    other, _, _, _ = _one_splat(1.5, 0.8)
    other["xyz"] = np.array([[0.8, 0.0, 0.5]], np.float32)
    both = {k: np.concatenate([needle[k], other[k]]) for k in KEYS}
    target = torch.zeros(H, W, 3, device="cuda")
    M = {}
    for aa in (True, False):
        r = _renderer(W, H, aa=aa)
        res = r.renderForward(_dev(both), cam, want_radii=True)
        radii = _np(res.radii)
        M[aa] = r.stats()["M"]
        _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
        g = r.renderBackward(cot)
        if aa:
            assert radii[0] == 0 and radii[1] > 0
            for k in KEYS:
                gk = _np(g[k])
                assert np.isfinite(gk).all() and not gk[0].any(), k
            assert np.abs(_np(g["opacity"])[1]) > 0
            alone = _renderer(W, H)
            alone.renderForward(_dev(other), cam)
            assert M[True] == alone.stats()["M"]
        else:
            assert radii[0] > 0
    assert M[False] > M[True]


# ------------------------------------------------------------------------------------------------------------ depth cuts
def test_depth_cuts_hold_when_the_mode_is_switched_on():
    """A view trained without the mode (its cuts and hints from those forwards), then rendered with it under its cuts and
    hints: the same bits as an uncut forward in the mode on a second context (exactness through miss detection)."""
    from gaussiansplattingmlx_amd.scenes import make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    params, cams, (W, H) = make_config("c2_100k_800", n_views=4)
    r, r2 = _renderer(W, H, aa=False), _renderer(W, H, aa=True)
    r.cutMinDropped = 0
    dev = r.device
    tp = {k: torch.as_tensor(v, device=dev) for k, v in perturb(params, 7).items()}
    targets = [r2.renderForward(tp, c).render.clone() for c in cams]
    model = GaussModel(params, dev)
    tr = GaussianTrainer(model, r, iterationCount=30000, densify=False)
    for i in range(12):
        tr.trainStep(cams[i % 4], targets[i % 4], viewKey=i % 4)
    r.setAntialiased(True)
    cut = 0
    for v in range(4):
        got = r.renderForward(model.getParams(), cams[v], viewKey=v)
        missed = r.forwardMissed()
        M_cut = r.stats()["M"]
        if missed:
            got = r.renderForward(model.getParams(), cams[v], viewKey=v, depthCuts=False)
        img, nc = got.render.clone(), r.lastContrib().clone()
        want = r2.renderForward(model.getParams(), cams[v])
        cut += int(missed or M_cut < r2.stats()["M"])
        assert torch.equal(img, want.render), v
        assert torch.equal(nc, r2.lastContrib()), v
    assert cut >= 1, cut


# ---------------------------------------------------------------------------------------------------- every step kind
@pytest.mark.parametrize("variant", ["fused", "unfused", "native_sh", "native_allreduce"])
def test_train_trajectory_matches_the_composed_oracle_loop(oracle32, oracle64, variant):
    """test_gpu_trajectory.test_train_trajectory_matches_the_oracle_loop (N = 3000, 16 x 16 tiles) in the mode, against its
    oracle loop with AAOracle: the same loops, the same bars."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    W, H, N = 160, 120, 3000
    p0, cams = traj._scene(71, N, W, H, 0.06)
    tp = perturb(p0, 5, 0.1)
    o32, o64 = AAOracle(oracle32), AAOracle(oracle64)
    targets = [o32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy() for c in cams]
    want_l, want_p, want_m, want_v = traj._oracle_loop(o32, p0, cams, targets, W, H)
    ref_l, ref_p, _, _ = traj._oracle_loop(o64, p0, cams, targets, W, H)
    r = _renderer(W, H)
    got_l, got_p, got_m, got_v, tr = traj._hip_loop(r, p0, cams, targets, variant)
    assert r.stats()["overflow"] == 0 and tr.forwardMisses == 0
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


@pytest.mark.parametrize("variant", ["local8", "local8_unfused"])
def test_eight_views_one_update_matches_the_composed_oracle_loop(oracle32, oracle64, variant):
    """test_gpu_trajectory.test_eight_views_one_update_matches_the_oracle_loop (views_per_rank = 8) in the mode."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    W, H, N, V = 160, 120, 3000, 8
    p0, _ = traj._scene(71, N, W, H, 0.06)
    cams = traj._scene_views(W, H, 12)
    tp = perturb(p0, 5, 0.1)
    o32, o64 = AAOracle(oracle32), AAOracle(oracle64)
    targets = [o32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy() for c in cams]
    want_l, want_p, want_m, want_v = traj._oracle_loop_multi(o32, p0, cams, targets, W, H, V)
    ref_l, ref_p, ref_m, ref_v = traj._oracle_loop_multi(o64, p0, cams, targets, W, H, V)
    r = _renderer(W, H)
    got_l, got_p, got_m, got_v, tr = traj._hip_loop_multi(r, p0, cams, targets, V, fuse_adam=variant == "local8")
    assert r.stats()["overflow"] == 0 and tr.forwardMisses == 0
    report = {}
    traj._compare("param", got_p, want_p, p0, report)
    traj._compare("m", got_m, want_m, p0, report)
    traj._compare("v", got_v, want_v, p0, report)
    traj._compare("oracle32_vs_64.param", {k: ref_p[k] for k in KEYS}, want_p, p0, report)
    traj._compare("oracle32_vs_64.m", {k: ref_m[k] for k in KEYS}, want_m, p0, report)
    traj._compare("oracle32_vs_64.v", {k: ref_v[k] for k in KEYS}, want_v, p0, report)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    assert got_l[-1] < got_l[0] and dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        for tag in ("m", "v"):
            e, ref = report[f"{tag}.{k}"], report[f"oracle32_vs_64.{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= max(2e-2, 2.0 * ref["max_rel"]), (tag, k, e, ref)
        e, ref = report[f"param.{k}"], report[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * traj.STEPS * 1.01 + 1e-6, (k, e)


def test_pose_opt_trains_in_the_mode():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams = traj._scene(71, N, W, H, 0.06)
    r = _renderer(W, H)
    targets = [r.renderForward(_dev(_perturbed(p0)), c).render.clone() for c in cams]
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, pose_opt=True, n_views=3)
    losses = [float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]) for i in range(30)]
    assert np.isfinite(losses).all() and bool(torch.isfinite(model.arena).all())
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    assert np.isfinite(tr.poseCorrections()).all()
