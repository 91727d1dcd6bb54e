"""The 3-D smoothing filter on the device (include/gsplat.h gs_set_filter3d, GaussianTrainer(filter_3d=True)) against
gaussiansplattingmlx_amd/filter3d.py and the oracle composed from the reference's ops in test_filter3d_cpu.Filter3DOracle
(activations_forward -> the filter in the oracle's precision -> projection_forward ..., sigma kappa (rho) packed).  Images and
gradients are held to the float64 oracle.  The trajectories follow test_gpu_trajectory's harness: the float32 oracle's loop is
what the kernels' loop is compared with, and the float64 oracle's loop measures the spread inherent in float32.  There the
filter step is float32 arithmetic in the kernels' order, as the wrapped oracle's own ops are.  (Composed from a float64 exp of
the raw scales instead, the float32 loop alone moves: ten steps on the CPU put 1.2e-3 of the features_dc moments beyond the
harness's 1e-3, from splats whose integer radius flips on the last bit of s.)

Tolerances were fixed before the first run on the card.  Images: the project's bar, 1e-4 L-inf, against the float64 composed
oracle.  Gradients: test_gpu_parity's metric, max |a - b| / max |b| per tensor, at 1e-3.  The pose gradient: float64 central
differences of the composed oracle's loss at h = 1e-4, at 5 % of the largest component (test_gpu_antialiasing's FD_BAR, its
step and its cause).  Fused Adam: that file's share bar.  Trajectories: test_gpu_trajectory's bars and oracle loop, with
Filter3DOracle in place of the oracle.

The filter width: per element 8 x 2^-23 (|x v02| + |y v12| + |z v22| + |v32|) / focal sqrt(0.2), evaluated in float64
(filter3d.width_bar).  The kernel's own error is three products and three sums for z (4 x 2^-24 of the sum of magnitudes), a
division, the constant's rounding and a product: 3.5 x 2^-23.  The inputs are float32 numbers handed to both sides unchanged.
Condition: the float32 and the float64 `seen` sets coincide -- asserted in float64: no (point, camera) pair within 1e-4
relative of the z = 0.2 or the margin thresholds; nothing is excluded from the comparison.  The scenes are built so that this
holds (a candidate point within 1e-3 of a threshold is not taken into the scene); float32 evaluates z and the two ratios to a
few 2^-24 relative of the terms' magnitudes, three orders of magnitude below 1e-4.

Bake: 1e-6 of the tensor's largest magnitude against filter3d.bake (logarithms of float32 numbers of order 1e-2 .. 1e1: a
few 2^-24 relative each).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import filter3d as f3
from gaussiansplattingmlx_amd.camera import Camera, apply_pose_correction, look_at_c2w

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
IMG_BAR, GRAD_BAR, FD_BAR, FD_H = 1e-4, 1e-3, 5e-2, 1e-4


def _load(name):
    spec = importlib.util.spec_from_file_location("_f3d_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_filter3d_cpu")
traj = _load("test_gpu_trajectory")
Filter3DOracle = cpu.Filter3DOracle


def _renderer(W, H, tile=(16, 16), aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, tile, False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _perturbed(p):
    from gaussiansplattingmlx_amd.scenes import perturb
    return perturb(p, 5, 0.1)


def _parity_scene(W=160, H=120, N=3000):
    """test_gpu_trajectory's cloud with small splats (scale 0.03) and the float32 filter of its three cameras (~0.012): kappa
    from ~0.3 to ~1 over the visible splats.  The oracle and the kernels get the same float32 widths."""
    p, cams = traj._scene(71, N, W, H, 0.03)
    filt = f3.filter_width(p["xyz"], cams).astype(np.float32)
    return p, cams, filt


def _step(r, params, cam, target):
    res = r.renderForward(params, cam)
    img, alpha, depth = res.render.clone(), res.alpha.clone(), res.depth.clone()
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    g = r.renderBackward(cot)
    return img, alpha, depth, float(loss[0]), {k: v.clone() for k, v in g.items()}


# ------------------------------------------------------------------------------------------------------- the filter width
def _ring(V, W=800, H=600, seed=0):
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(V):
        a = 2 * np.pi * i / V + rng.uniform(-0.1, 0.1)
        rad, h, focal = rng.uniform(3.0, 6.0), rng.uniform(-1.5, 2.5), rng.uniform(500.0, 1200.0)
        cams.append(Camera(W, H, focal, focal * 1.01, look_at_c2w([rad * np.cos(a), rad * np.sin(a), h], rng.uniform(-0.5, 0.5, 3))))
    return cams


def _point_threshold_distance(x, cams):
    d = np.full(x.shape[0], np.inf)
    for c in cams:
        _, _, p, lim = f3.camera_terms(x, c)
        z = p[:, 2]
        d = np.minimum(d, np.abs(z - f3.Z_NEAR) / f3.Z_NEAR)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.minimum(d, np.abs(np.abs(p[:, 0] / z) - lim[0]) / lim[0])
            d = np.minimum(d, np.abs(np.abs(p[:, 1] / z) - lim[1]) / lim[1])
    return d


def _width_scene(N, V, seed):
    """Points of a box that reaches outside every frustum and behind some cameras (float32 numbers), candidates within 1e-3 of a
    threshold of `seen` left out while the scene is built; the last point is one no camera sees."""
    cams = _ring(V, seed=seed)
    rng = np.random.default_rng(seed + 1)
    cand = rng.uniform(-4.0, 4.0, (int(N * 1.6) + 64, 3)).astype(np.float32)
    cand = cand[_point_threshold_distance(cand.astype(np.float64), cams) >= 1e-3]
    assert cand.shape[0] >= N - 1
    x = np.concatenate([cand[:N - 1], np.array([[0.0, 0.0, 500.0]], np.float32)])
    return x, cams


@pytest.mark.parametrize("N,V,seed", [(4000, 20, 11), (300_000, 100, 12)])
def test_filter_width_matches_the_float64_rule(N, V, seed):
    x, cams = _width_scene(N, V, seed)
    assert f3.threshold_distance(x, cams) >= 1e-4           # the condition: float32 and float64 see the same set
    want, seen, arg = f3.filter_width(x, cams, details=True)
    assert not seen[-1] and 0.2 < seen.mean() < 1.0 and len(np.unique(arg[seen])) >= 3
    r = _renderer(64, 64)
    r.setFilterCameras(cams)
    got = _np(r.computeFilter3D(_t(x))).astype(np.float64)
    bar = f3.width_bar(x, cams)
    err = np.abs(got - want)
    print(f"width N={N} V={V}: max err / bar = {(err / bar).max():.3f}, seen share {seen.mean():.3f}")
    assert np.all(err <= bar), float((err / bar).max())
    assert got[-1] == got[seen].max()                      # the never-seen rule, on the device's own numbers
    # into a caller's buffer, nothing allocated; the same bits again
    out = torch.full((N + 7,), -3.0, device="cuda")
    assert r.computeFilter3D(_t(x), out=out) is out
    assert np.array_equal(_np(out[:N]).astype(np.float64), got) and bool((out[N:] == -3.0).all())


def test_filter_width_when_nothing_is_seen_and_without_cameras():
    from gaussiansplattingmlx_amd._lib import GsplatError
    cams = _ring(5, seed=3)
    x = np.random.default_rng(4).uniform(-1, 1, (1000, 3)).astype(np.float32) + np.array([0, 0, 500.0], np.float32)
    assert not f3.filter_width(x, cams, details=True)[1].any()
    r = _renderer(64, 64)
    with pytest.raises(GsplatError, match="gs_compute_filter3d"):
        r.computeFilter3D(_t(x))
    r.setFilterCameras(cams)
    out = torch.full((1000,), 5.0, device="cuda")
    r.computeFilter3D(_t(x), out=out)
    assert not bool(out.any())
    r.setFilterCameras([])                                   # V = 0 empties the table
    with pytest.raises(GsplatError, match="gs_compute_filter3d"):
        r.computeFilter3D(_t(x))


# ------------------------------------------------------------------------------------------------------------ the setter
def test_off_is_off():
    """NULL after non-NULL: the image and gradients of a context that never had a filter, bit for bit (where that context is
    itself run-to-run identical: the blend backward's float atomics are not on every scene)."""
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    params = _dev(p)
    fresh = _renderer(W, H)
    target = fresh.renderForward(_dev(_perturbed(p)), cams[1]).render.clone()
    a = _step(fresh, params, cams[0], target)
    b = _step(fresh, params, cams[0], target)
    r = _renderer(W, H)
    r.setFilter3D(_t(filt))
    on = _step(r, params, cams[0], target)
    assert float((on[0] - a[0]).abs().max()) > 1e-3          # (the filter matters on this scene)
    r.setFilter3D(None)
    c = _step(r, params, cams[0], target)
    for i in range(3):
        assert torch.equal(a[i], c[i]), i
    assert a[3] == c[3]
    for k in KEYS:
        if torch.equal(a[4][k], b[4][k]):
            assert torch.equal(a[4][k], c[4][k]), k
        else:
            assert torch.allclose(a[4][k], c[4][k], rtol=1e-5, atol=1e-7 * float(a[4][k].abs().max())), k


@pytest.mark.parametrize("aa", [False, True])
def test_zero_filter_is_the_mode_off(aa):
    """f = 0: s_eff = sqrt(s s) = s and kappa = 1, so the filtered kernels compute what the default ones do -- within the image
    and gradient bars; whether to the bit is printed (DESIGN.md section 14 records it)."""
    p, cams, _ = _parity_scene()
    W, H = 160, 120
    params = _dev(p)
    r = _renderer(W, H, aa=aa)
    target = r.renderForward(_dev(_perturbed(p)), cams[1]).render.clone()
    a = _step(r, params, cams[0], target)
    r.setFilter3D(torch.zeros(3000, device="cuda"))
    z = _step(r, params, cams[0], target)
    exact = all(torch.equal(a[i], z[i]) for i in range(3)) and all(torch.equal(a[4][k], z[4][k]) for k in KEYS)
    print(f"zero filter (aa={aa}): bit-exact = {exact}; image max diff {float((a[0] - z[0]).abs().max()):.3e}; gradients "
          + ", ".join(f"{k} {_rel(_np(z[4][k]), _np(a[4][k])):.2e}" for k in KEYS))
    for i in range(3):
        assert float((a[i] - z[i]).abs().max()) <= IMG_BAR * max(1.0, float(a[i].abs().max()) if i == 2 else 1.0), i
    for k in KEYS:
        assert _rel(_np(z[4][k]), _np(a[4][k])) <= GRAD_BAR, k


def test_backward_uses_its_forwards_filter():
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    params = _dev(p)
    r = _renderer(W, H)
    f1, f2 = _t(filt), _t(filt * 3.0)
    target = torch.zeros(H, W, 3, device="cuda")
    r.setFilter3D(f1)
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    want = {k: v.clone() for k, v in r.renderBackward(cot).items()}
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.setFilter3D(f2)                # between the forward and its backward: changes nothing for that pair
    got = {k: v.clone() for k, v in r.renderBackward(cot).items()}
    for k in KEYS:
        assert _rel(_np(got[k]), _np(want[k])) <= 1e-5, k
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    other = r.renderBackward(cot)
    assert _rel(_np(other["scales"]), _np(want["scales"])) > 1e-2          # (the other filter is another function)
    r.setFilter3D(None)              # ... and NULL between the two likewise
    r.setFilter3D(f1)
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.setFilter3D(None)
    got = r.renderBackward(cot)
    for k in KEYS:
        assert _rel(_np(got[k]), _np(want[k])) <= 1e-5, k


# ------------------------------------------------------------------------------------------------------ forward parity
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("variant", ["tiles16", "tiles16_untrimmed", "block_lists", "pose"])
def test_forward_matches_the_composed_oracle(oracle64, variant, aa):
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    tile = (50, 38) if variant == "block_lists" else (16, 16)
    r = _renderer(W, H, tile, aa=aa)
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
    r.setFilter3D(_t(filt))
    try:
        res = r.renderForward(_dev(p), cam, want_radii=True)
        img, alpha, depth, radii = _np(res.render), _np(res.alpha), _np(res.depth), _np(res.radii)
    finally:
        if variant == "pose":
            r.setPoseCorrection(None, None)
    fw = Filter3DOracle(oracle64, filt, aa).render_forward(p, ocam.as_dict(), W, H, tile[0], tile[1], 4)
    errs = (np.abs(img.reshape(-1, 3) - fw["color"]).max(), np.abs(alpha.reshape(-1) - fw["alpha"]).max(),
            np.abs(depth.reshape(-1) - fw["depth"]).max())
    print(f"forward {variant} aa={aa}: colour {errs[0]:.2e} alpha {errs[1]:.2e} depth {errs[2]:.2e}")
    assert errs[0] <= IMG_BAR
    assert errs[1] <= IMG_BAR
    assert errs[2] <= IMG_BAR * max(1.0, float(np.abs(fw["depth"]).max()))
    assert np.array_equal(radii > 0, fw["radii"] > 0)
    assert fw["kappa"][fw["radii"] > 0].min() < 0.7           # (the filter matters on this scene)
    plain = oracle64.render_forward(p, ocam.as_dict(), W, H, tile[0], tile[1], 4)
    assert np.abs(plain["color"] - fw["color"]).max() > 1e-2


# ----------------------------------------------------------------------------------------------------- gradient parity
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("tile", [(16, 16), (50, 38)])
def test_gradients_match_the_composed_oracle(oracle64, tile, aa):
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H, tile, aa=aa)
    cam = cams[0]
    o = Filter3DOracle(oracle64, filt, aa)
    target = oracle64.render_forward(_perturbed(p), cam.as_dict(), W, H, tile[0], tile[1], 4)["color"].reshape(H, W, 3)
    r.setFilter3D(_t(filt))
    _, _, _, loss, g = _step(r, _dev(p), cam, torch.as_tensor(target, dtype=torch.float32, device="cuda"))
    want_loss, fw, cot = cpu.f3d_loss(o, p, cam.as_dict(), W, H, target, tile)
    z = np.zeros(W * H)
    want = o.render_backward(p, cam.as_dict(), W, H, tile[0], tile[1], 4, fw, cot.reshape(-1, 3), z, z)
    rels = {k: _rel(_np(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)) for k in KEYS}
    print(f"gradients tile={tile} aa={aa}: loss diff {abs(loss - want_loss):.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in rels.items()))
    assert abs(loss - want_loss) <= 1e-5
    for k in KEYS:
        assert rels[k] <= GRAD_BAR, (k, rels[k])


@pytest.mark.parametrize("aa", [False, True])
def test_fused_adam_matches_backward_then_adam(aa):
    """gs_render_backward_adam == gs_render_backward + gs_adam_step under the filter (test_gpu_antialiasing's check and share
    bar, through the trainer)."""
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams, _ = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H, aa=aa)
    target = torch.rand(H, W, 3, device=r.device, generator=torch.Generator(device=r.device).manual_seed(3))
    out = {}
    for fuse in (False, True):
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse, densify=False, filter_3d=True, filter_cameras=cams)
        for _ in range(3):
            tr.trainStep(cams[0], target)
        assert r.filter3D is None                                    # (the trainer binds its filter around its own steps only)
        out[fuse] = (_np(model.arena).copy(), _np(model.m).copy(), _np(model.v).copy())
    start = _np(GaussModel(p, r.device).arena)
    a, b = out[True][0] - start, out[False][0] - start
    assert np.abs(b).max() > 0
    assert np.mean(np.abs(a - b) > 1e-3 * np.abs(b).max()) < 1e-3
    for k in (1, 2):
        ref = out[False][k]
        assert np.mean(np.abs(out[True][k] - ref) > 1e-3 * np.abs(ref).max()) < 1e-3, k


@pytest.mark.parametrize("aa", [False, True])
def test_pose_gradient_against_oracle_finite_differences(oracle64, aa):
    W = H = 96
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    p = make_gaussians(300, "trained_like", 7)
    p["scales"] = (p["scales"] + 0.6).astype(np.float32)
    cam = Camera(W, H, 90.0, 90.0, look_at_c2w((3.0, -2.5, 2.0)))
    filt = f3.filter_width(p["xyz"], [cam]).astype(np.float32)      # (the cameras as given, unrefined)
    o = Filter3DOracle(oracle64, filt, aa)
    r = _renderer(W, H, aa=aa)
    tgt = r.renderForward(_dev(make_gaussians(300, "trained_like", 8)), cam).render.clone()
    d0 = np.array([0.01, -0.008, 0.012, 0.03, -0.02, 0.025])
    delta, grad = torch.as_tensor(d0, dtype=torch.float32, device="cuda"), torch.zeros(6, device="cuda")
    r.setPoseCorrection(delta, grad)
    r.setFilter3D(_t(filt))
    try:
        _step(r, _dev(p), cam, tgt)
    finally:
        r.setPoseCorrection(None, None)
    got = _np(grad).astype(np.float64)
    tnp = _np(tgt).astype(np.float64)
    d0 = _np(delta).astype(np.float64)

    def loss(d):
        return cpu.f3d_loss(o, p, apply_pose_correction(cam, d).as_dict(), W, H, tnp)[0]
    fd = np.array([(loss(d0 + FD_H * e) - loss(d0 - FD_H * e)) / (2 * FD_H) for e in np.eye(6)])
    print(f"pose gradient aa={aa}: {np.abs(got - fd).max() / np.abs(fd).max():.3e} of the largest component")
    assert np.abs(got - fd).max() <= FD_BAR * np.abs(fd).max(), (got, fd)


# ------------------------------------------------------------------------------------------------------------------ bake
def test_bake_matches_numpy_and_renders_as_the_filtered_model(tmp_path):
    from gaussiansplattingmlx_amd.ply import PlyWriter
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H)
    params, f = _dev(p), _t(filt)
    baked = r.bakeFilter3D(params, f)
    ws, wo = f3.bake(p["scales"], p["opacity"], filt)
    assert _rel(_np(baked["scales"]), ws) <= 1e-6 and _rel(_np(baked["opacity"]).reshape(-1), wo) <= 1e-6
    for k in ("xyz", "features_dc", "features_rest", "rotation"):
        assert baked[k] is params[k]
    # in place: the outputs may alias the inputs
    sc, op = params["scales"].clone(), params["opacity"].clone()
    r._check(r.lib.gs_filter3d_bake(r.ctx, 3000, sc.data_ptr(), op.data_ptr(), f.data_ptr(), sc.data_ptr(), op.data_ptr()))
    assert torch.equal(sc, baked["scales"]) and torch.equal(op, baked["opacity"])
    # a zero filter bakes the model itself
    same = r.bakeFilter3D(params, torch.zeros(3000, device="cuda"))
    assert _rel(_np(same["scales"]), p["scales"]) <= 1e-6 and _rel(_np(same["opacity"]), p["opacity"]) <= 1e-6
    # the baked model with the filter off is the filtered model
    for aa in (False, True):
        r.setAntialiased(aa)
        r.setFilter3D(f)
        want = r.renderForward(params, cams[0]).render.clone()
        r.setFilter3D(None)
        got = r.renderForward(baked, cams[0]).render.clone()
        plain = r.renderForward(params, cams[0]).render.clone()
        assert float((got - want).abs().max()) <= IMG_BAR, aa
        assert float((plain - want).abs().max()) > 1e-2
    r.setAntialiased(False)
    # save_snapshot -> ply load -> render: the trainer writes the baked parameters
    model = GaussModel(p, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, filter_3d=True, filter_cameras=cams)
    assert torch.equal(tr.filter3D(), r.computeFilter3D(params["xyz"]))
    tr.outputDirectory = tmp_path
    tr.save_snapshot(7)
    r.sync()
    ld = PlyWriter(r).loadGaussianBinaryPLYAsMLX(os.path.join(tmp_path, "iteration_7.ply"))
    loaded = dict(xyz=ld["positions"], features_dc=ld["features_dc"], features_rest=ld["features_rest"], scales=ld["scales"],
                  rotation=ld["rotations"], opacity=ld["opacities"].reshape(-1))
    r.setFilter3D(tr.filter3D())
    want = r.renderForward(params, cams[0]).render.clone()
    r.setFilter3D(None)
    got = r.renderForward(loaded, cams[0]).render.clone()
    assert float((got - want).abs().max()) <= IMG_BAR


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import ctypes as C
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams, filt = _parity_scene()
    W, H = 160, 120
    r = _renderer(W, H)
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    params, f = _dev(p), _t(filt)
    r.setFilter3D(f)
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, torch.zeros(H, W, 3, device="cuda"), 0.2)
    g = {k: torch.zeros_like(params[k]) for k in ("xyz", "scales", "rotation", "opacity")}
    cc = torch.zeros(_lib.load().gs_dp_cc_floats(3000), device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    lib = r.lib
    assert lib.gs_render_backward_dp(r.ctx, P(cot), None, None, P(g["xyz"]), P(g["scales"]), P(g["rotation"]), P(g["opacity"]),
                                     P(cc)) == invalid
    assert "3-D filter" in lib.gs_last_error(r.ctx).decode()
    assert lib.gs_render_backward_dp_begin(r.ctx, P(cot), None, None, P(cc)) == invalid
    assert lib.gs_render_backward_dp_finish(r.ctx, P(g["xyz"]), P(g["scales"]), P(g["rotation"]), P(g["opacity"])) == invalid
    assert lib.gs_render_backward_dp_geom(r.ctx, P(cot), None, None, P(cc), P(g["xyz"]), P(g["scales"]), P(g["rotation"]),
                                          P(g["opacity"]), P(g["xyz"])) == invalid
    assert lib.gs_render_backward_dp_finish_geom(r.ctx, P(g["xyz"]), P(g["scales"]), P(g["rotation"]), P(g["opacity"]),
                                                 P(g["xyz"])) == invalid
    args = _lib.gs_dp_step_args() if hasattr(_lib, "gs_dp_step_args") else None
    assert lib.gs_dp_step(r.ctx, 0, C.byref(args) if args is not None else None) == invalid
    assert "3-D filter" in lib.gs_last_error(r.ctx).decode()
    prm = MCMCConfig().params(0, 1)
    assert lib.gs_set_mcmc(r.ctx, C.byref(prm)) == invalid
    assert "3-D filter" in lib.gs_last_error(r.ctx).decode()
    assert lib.gs_set_mcmc(r.ctx, None) == 0
    # the other way round: no filter while the MCMC strategy is set
    r.setFilter3D(None)
    r.setMCMC(prm)
    assert lib.gs_set_filter3d(r.ctx, P(f)) == invalid and "gs_set_filter3d" in lib.gs_last_error(r.ctx).decode()
    r.setMCMC(None)
    # the plain backward of the filtered forward still runs
    r.setFilter3D(f)
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, torch.zeros(H, W, 3, device="cuda"), 0.2)
    assert bool(torch.isfinite(r.renderBackward(cot)["scales"]).all())
    r.setFilter3D(None)
    # the trainer's argument checks
    model = GaussModel(p, r.device)
    kw = dict(iterationCount=1000, densify=False, filter_3d=True)
    with pytest.raises(ValueError, match="filter_cameras"):
        GaussianTrainer(model, r, **kw)
    with pytest.raises(ValueError, match="filter_cameras"):
        GaussianTrainer(model, r, filter_cameras=[], **kw)
    with pytest.raises(ValueError, match="mcmc"):
        GaussianTrainer(model, r, filter_cameras=cams, strategy="mcmc", **kw)
    with pytest.raises(ValueError, match="filter_3d"):
        GaussianTrainer(model, r, filter_cameras=cams, views_per_rank=2, **kw)
    with pytest.raises(ValueError, match="filter_3d"):
        GaussianTrainer(model, r, filter_cameras=cams, process_group=object(), **kw)
    with pytest.raises(ValueError, match="filter_3d"):
        uid = C.create_string_buffer(_lib.GS_DP_UNIQUE_ID_BYTES)
        GaussianTrainer(model, r, filter_cameras=cams, exchange_impl="native", dp_bootstrap=(uid.raw, 0, 1), **kw)
    with pytest.raises(ValueError, match="filter_3d_interval"):
        GaussianTrainer(model, r, filter_cameras=cams, filter_3d_interval=0, **kw)
    with pytest.raises(ValueError, match="filter_3d=True"):
        GaussianTrainer(model, r, iterationCount=1000, filter_cameras=cams)


# -------------------------------------------------------------------------------------------------------------- trainer
def _hip_loop(r, p0, cams, targets, fuse, steps=None):
    """test_gpu_trajectory._hip_loop with the trainer's filter on."""
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    steps = traj.STEPS if steps is None else steps
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, fuse_adam=fuse, filter_3d=True, filter_cameras=cams)
    tg = [torch.as_tensor(t, device=r.device) for t in targets]
    losses = []
    for it in range(steps):
        v = it % len(cams)
        losses.append(float(tr.trainStep(cams[v], tg[v], viewKey=v)[0]))
    N = model.N
    params = {k: _np(model.getParams()[k]).copy() for k in KEYS}
    mom = {k: _np(model._carve(model.m, N)[k]).copy() for k in KEYS}
    var = {k: _np(model._carve(model.v, N)[k]).copy() for k in KEYS}
    return losses, params, mom, var, tr


@pytest.mark.parametrize("variant", ["fused", "unfused"])
def test_train_trajectory_matches_the_composed_oracle_loop(oracle32, oracle64, variant):
    """test_gpu_trajectory.test_train_trajectory_matches_the_oracle_loop (N = 3000, 16 x 16 tiles) under the trainer's filter
    (computed once: ten steps stay below filter_3d_interval), against its oracle loop with Filter3DOracle: the same bars."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    W, H, N = 160, 120, 3000
    p0, cams = traj._scene(71, N, W, H, 0.06)
    r = _renderer(W, H)
    r.setFilterCameras(cams)
    filt = _np(r.computeFilter3D(_t(p0["xyz"])))             # the kernel's own float32 widths (held to the rule above)
    assert np.all(np.abs(filt - f3.filter_width(p0["xyz"], cams)) <= f3.width_bar(p0["xyz"], cams))
    tp = perturb(p0, 5, 0.1)
    o32, o64 = Filter3DOracle(oracle32, filt), Filter3DOracle(oracle64, filt)
    targets = [o32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy() for c in cams]
    want_l, want_p, want_m, want_v = traj._oracle_loop(o32, p0, cams, targets, W, H)
    ref_l, ref_p, _, _ = traj._oracle_loop(o64, p0, cams, targets, W, H)
    got_l, got_p, got_m, got_v, tr = _hip_loop(r, p0, cams, targets, variant == "fused")
    assert r.stats()["overflow"] == 0 and tr.forwardMisses == 0
    report = {}
    traj._compare("param", got_p, want_p, p0, report)
    traj._compare("m", got_m, want_m, p0, report)
    traj._compare("v", got_v, want_v, p0, report)
    traj._compare("oracle32_vs_64.param", {k: ref_p[k] for k in KEYS}, want_p, p0, report)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    print(f"trajectory {variant}: loss diff {dl.max():.2e}; " + ", ".join(
        f"{k} {report['param.' + k]['share_beyond']:.1e}/{report['oracle32_vs_64.param.' + k]['share_beyond']:.1e}" for k in KEYS))
    assert got_l[-1] < got_l[0] and dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        for tag in ("m", "v"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = report[f"param.{k}"], report[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * traj.STEPS * 1.01 + 1e-6, (k, e)


@pytest.mark.parametrize("planned", [True, False])
def test_filter_follows_a_densify_event(oracle32, planned):
    """A run that crosses a densify event: behind it the trainer's buffer holds the filter of the new positions for all new-N
    rows (bit for bit a fresh computeFilter3D), the next step's loss is finite, and the steady-state steps before and after
    allocate no more than the same steps of a trainer without the filter do."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 4000
    p, cam = traj._scene(63, N, W, H, 0.06)
    cam = cam[0]
    p["features_rest"] *= 0.05
    p["opacity"][:50] = -8.0
    tgt = oracle32.render_forward(perturb(p, 5, 0.1), cam.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3)
    allocs = {}
    for mode in (False, True):
        r = _renderer(W, H)
        r.reserve(3 * N, 4 << 20)
        model = GaussModel(p, r.device, capacity=3 * N)
        kw = dict(filter_3d=True, filter_cameras=[cam], filter_3d_interval=1000) if mode else {}
        tr = GaussianTrainer(model, r, iterationCount=1000, **kw)
        tr.plannedDensify, tr.noiseSource = planned, ("library" if planned else None)
        tr.densifyFromIter, tr.split_and_prune_per_iteration, tr.gradientThreshold = 4, 4, 2e-6
        target = torch.as_tensor(tgt, device=r.device)
        count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
        tr.trainStep(cam, target)                                     # (first step: the renderer's own buffers)
        r.sync()
        a0 = count()
        for _ in range(3):
            tr.trainStep(cam, target)
        r.sync()
        a1 = count()
        if mode:
            buf = tr._filter.data_ptr()
        tr.trainStep(cam, target)                                     # iteration 4: the event, behind its Adam step
        st = tr.lastDensifyStats
        assert st["prune"] >= 50 and st["split"] + st["clone"] > 0
        if mode:
            fresh = r.computeFilter3D(model.getParams()["xyz"])
            assert tr.filter3D().shape[0] == model.N and torch.equal(tr.filter3D(), fresh)
            assert tr._filter.data_ptr() == buf                       # (capacity 3 N: the buffer did not have to grow)
            assert float(fresh.min()) > 0
        loss = float(tr.trainStep(cam, target)[0])
        assert np.isfinite(loss)
        r.sync()
        a2 = count()
        for _ in range(2):
            tr.trainStep(cam, target)
        r.sync()
        allocs[mode] = (a1 - a0, count() - a2)
        assert bool(torch.isfinite(model.arena).all())
    print(f"allocations in steady-state steps (planned={planned}), without / with the filter: {allocs[False]} / {allocs[True]}")
    assert allocs[True] == allocs[False]


def test_filter_is_recomputed_on_its_interval_and_on_a_reload():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    W, H, N = 160, 120, 3000
    p0, cams = traj._scene(71, N, W, H, 0.06)
    r = _renderer(W, H, aa=True)
    targets = [r.renderForward(_dev(_perturbed(p0)), c).render.clone() for c in cams]
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, pose_opt=True, exposure_opt=True, n_views=3,
                         filter_3d=True, filter_cameras=cams, filter_3d_interval=5)
    f0 = tr.filter3D().clone()
    losses = []
    for i in range(4):
        losses.append(float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]))
    assert torch.equal(tr.filter3D(), f0)                              # xyz moved, the filter is the construction's
    losses.append(float(tr.trainStep(cams[1], targets[1], viewKey=1)[0]))
    assert not torch.equal(tr.filter3D(), f0)                          # behind step 5: the filter of the positions as they are now
    assert torch.equal(tr.filter3D(), r.computeFilter3D(model.getParams()["xyz"]))
    for i in range(5, 30):
        losses.append(float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]))
    assert np.isfinite(losses).all() and bool(torch.isfinite(model.arena).all())
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    # referenceParamReload: the cadence restores the last committed parameters, and the filter follows them
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=True, filter_3d=True, filter_cameras=cams, filter_3d_interval=3)
    tr.referenceParamReload = True
    tr.split_and_prune_per_iteration = 4
    f0 = tr.filter3D().clone()
    for i in range(4):
        tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)
    assert not torch.equal(tr.filter3D(), f0)                          # (iteration 3: the interval, moved positions)
    tr.trainStep(cams[1], targets[1], viewKey=1)                       # iteration 4: outside the densify window -> reload
    assert torch.equal(model.getParams()["xyz"], _t(p0["xyz"]))
    assert torch.equal(tr.filter3D(), f0)


# ------------------------------------------------------------------------------------------------------------ depth cuts
def test_depth_cuts_hold_when_the_filter_is_switched_on():
    """A view trained without the filter (its cuts and hints from those forwards), then rendered with it under its cuts and
    hints: the same bits as an uncut filtered forward on a second context (exactness through miss detection)."""
    from gaussiansplattingmlx_amd.scenes import make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    params, cams, (W, H) = make_config("c2_100k_800", n_views=4)
    r, r2 = _renderer(W, H), _renderer(W, H)
    r.cutMinDropped = 0
    dev = r.device
    tp = {k: torch.as_tensor(v, device=dev) for k, v in perturb(params, 7).items()}
    targets = [r2.renderForward(tp, c).render.clone() for c in cams]
    model = GaussModel(params, dev)
    tr = GaussianTrainer(model, r, iterationCount=30000, densify=False)
    for i in range(12):
        tr.trainStep(cams[i % 4], targets[i % 4], viewKey=i % 4)
    r.setFilterCameras(cams)
    filt = r.computeFilter3D(model.getParams()["xyz"])
    r.setFilter3D(filt)
    r2.setFilter3D(filt)
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
