"""GaussianTrainer.evaluate on the device against the float64 restatement (tests/metrics_numpy.py)
applied to the very images renderChecked returns, downloaded.

Setup: a 64 x 48 scene of 2000 Gaussians (scenes.make_gaussians, scales raised so that a splat covers a few pixels), four
cameras; the targets are renders of a perturbed copy of the model.

Bars (test_gpu_metrics': the kernels are the same): PSNR within 1e-5 dB (sse within 1e-6 relative), mean SSIM no further from
float64 than the float32 mirror's worst pixel on that view (floor 1e-6), a view's weight exact for {0, 255} masks.  State:
the arena, both Adam moments and the per-view rows torch.equal before and after; the renderer's background, loss mask, filter,
pose binding and depth_gradient knob what they were; the iteration counter untouched; a train step afterwards finite."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N = 64, 48, 2000
PSNR_BAR, SSIM_FLOOR = 1e-5, 1e-6


def _load(name):
    spec = importlib.util.spec_from_file_location("_ge_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("metrics_numpy")
_shared = {}


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _scene():
    """(params, cameras, targets as device tensors): built once; the targets are renders of a perturbed copy."""
    if "scene" not in _shared:
        from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
        from gaussiansplattingmlx_amd.renderer import GaussianRenderer
        from gaussiansplattingmlx_amd.scenes import make_gaussians, perturb
        p = make_gaussians(N, "trained_like", 31)
        p["scales"] += 2.0
        cams = [Camera(W, H, 60.0, 60.0, look_at_c2w(e)) for e in ([3.0, -2.5, 2.0], [-3.0, 2.0, 1.5], [0.5, 3.5, 2.0], [2.5, 2.5, -1.0])]
        r = GaussianRenderer(4, W, H, (16, 16), False)
        try:
            tp = {k: _dev(v) for k, v in perturb(p, 3, 0.1).items()}
            targets = [r.renderChecked(tp, c, wantDepth=False).render.clone() for c in cams]
        finally:
            r.close()
        _shared["scene"] = (p, cams, targets)
    return _shared["scene"]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _shared.clear()


def _trainer(kind="plain", **extra):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams, targets = _scene()
    r = GaussianRenderer(4, W, H, (16, 16), False)
    kw = dict(iterationCount=1000, densify=False)
    if kind == "exposure_filter":
        kw.update(exposure_opt=True, n_views=len(cams), filter_3d=True, filter_cameras=cams)
    kw.update(extra)
    return GaussianTrainer(GaussModel(p, r.device), r, **kw), r


def _renders(tr, r, keyed=False):
    """What evaluate measures, downloaded: renderChecked of every camera as a step renders it (exposed under the view's row
    when keyed)."""
    _, cams, _ = _scene()
    out = []
    if tr.filter_3d:
        r.setFilter3D(tr._filter)
    try:
        for i, c in enumerate(cams):
            img = r.renderChecked(tr.model.getParams(), c, wantDepth=False).render
            out.append(_np(tr.exposedRender(img, i) if keyed else img).copy())
    finally:
        if tr.filter_3d:
            r.setFilter3D(None)
    return out


def _check_view(tag, got_psnr, got_ssim, img, tgt, mask):
    m64, m32 = mn.image_metrics(img, tgt, mask), mn.image_metrics(img, tgt, mask, np.float32)
    seen = m64["w"] > 0
    bar = max(SSIM_FLOOR, float(np.abs(m32["map"].astype(np.float64) - m64["map"])[seen].max()))
    print(f"{tag}: psnr {got_psnr:.6f} ({m64['psnr']:.6f}) ssim {got_ssim:.9f} ({m64['ssim']:.9f}, bar {bar:.2e})")
    assert abs(got_psnr - m64["psnr"]) <= PSNR_BAR, (tag, got_psnr, m64["psnr"])
    assert abs(got_ssim - m64["ssim"]) <= bar, (tag, got_ssim, m64["ssim"], bar)
    return m64


def test_evaluate_equals_the_mirror_on_the_downloaded_renders():
    from gaussiansplattingmlx_amd.evaluation import EvalResult, fit_affine_colour
    tr, r = _trainer()
    try:
        _, cams, targets = _scene()
        masks = [None, mn.make_mask("soft", H, W, 1), mn.make_mask("binary", H, W, 2), None]
        res = tr.evaluate(cams, targets, masks=masks, color_correct=True)
        assert isinstance(res, EvalResult) and res.psnr.shape == (4,) and res.skipped == dict(psnr=0, ssim=0, cc_psnr=0, cc_ssim=0)
        imgs, tg = _renders(tr, r), [_np(t) for t in targets]
        for i in range(4):
            m64 = _check_view(f"view {i}", res.psnr[i], res.ssim[i], imgs[i], tg[i], masks[i])
            assert 5.0 < m64["psnr"] < 60.0 and 0.0 < m64["ssim"] < 0.9999          # a real comparison, neither blank nor equal
            if i != 1:
                assert res.weight[i] == m64["sums"][2]
            M = fit_affine_colour(mn.colour_moments(imgs[i], tg[i], masks[i]))
            _check_view(f"view {i} cc", res.cc_psnr[i], res.cc_ssim[i], mn.apply_affine(M, imgs[i], np.float32), tg[i], masks[i])
            assert res.cc_psnr[i] >= res.psnr[i] - 1e-4          # the best affine transform is no worse than the identity
        assert res.mean_psnr == float(res.psnr.mean()) and res.mean_cc_ssim == float(res.cc_ssim.mean())
        # color_correct=None: off on a trainer without per-view appearance
        plain = tr.evaluate(cams, targets, masks=masks)
        assert plain.cc_psnr is None and np.allclose(plain.psnr, res.psnr, rtol=0, atol=1e-6) and np.allclose(plain.ssim, res.ssim, rtol=0, atol=1e-8)
    finally:
        r.close()


def test_colour_correction_undoes_an_affine_colour_change():
    tr, r = _trainer()
    try:
        _, cams, _ = _scene()
        A = np.array([[0.55, 0.1, 0.05], [0.05, 0.6, 0.1], [0.1, 0.05, 0.5]])
        b = np.array([0.12, 0.08, 0.15])
        targets = [(np.clip(x, 0, 1).astype(np.float64) @ A.T + b).astype(np.float32) for x in _renders(tr, r)]
        assert all(0.0 < t.min() and t.max() < 1.0 for t in targets)
        res = tr.evaluate(cams, targets, color_correct=True)
        print("psnr", res.psnr, "cc_psnr", res.cc_psnr)
        assert (res.cc_psnr - res.psnr > 20.0).all() and (res.cc_ssim > res.ssim).all() and (res.cc_ssim > 0.999).all()
    finally:
        r.close()


@pytest.mark.parametrize("kind", ["plain", "exposure_filter"])
def test_evaluate_changes_no_state(kind):
    tr, r = _trainer(kind)
    try:
        _, cams, targets = _scene()
        keyed = kind == "exposure_filter"
        for i in range(4):
            tr.trainStep(cams[i], targets[i], viewKey=i)
        # settings of the caller's renderer that evaluate must hand back as they were
        mask = _dev(mn.make_mask("binary", H, W, 5))
        r.setLossMask(mask)
        r.setBackground([0.2, 0.3, 0.4])
        r.setTuning(depth_gradient=0)
        m = tr.model
        tables = {k: t.rows.clone() for k, t in tr._perView.items()}
        before = dict(arena=m.arena.clone(), m=m.m.clone(), v=m.v.clone())
        it = tr.iteration
        res = tr.evaluate(cams, targets, viewKeys=list(range(4)) if keyed else None)
        assert np.isfinite(res.psnr).all() and (res.cc_psnr is not None) == keyed
        with pytest.raises(ValueError):          # ... also when it raises half-way through its checks
            tr.evaluate(cams, [t[:-1] for t in targets])
        for k, was in before.items():
            assert torch.equal(getattr(m, k), was), k
        for k, was in tables.items():
            assert torch.equal(tr._perView[k].rows, was), k
        assert tr.iteration == it
        assert r.lossMask is mask and np.array_equal(r.background, np.asarray([0.2, 0.3, 0.4], np.float32))
        assert r.getTuning("depth_gradient") == 0 and r.filter3D is None
        assert r._exposure == (None, None) and getattr(r, "_pose", (None, None)) == (None, None)
        r.setLossMask(None)
        r.setBackground(None)
        r.setTuning(depth_gradient=1)
        loss = tr.trainStep(cams[0], targets[0], viewKey=0)
        assert bool(torch.isfinite(loss).all()) and tr.iteration == it + 1
    finally:
        r.close()


def test_view_keys_measure_under_the_view_s_exposure():
    tr, r = _trainer("exposure_filter")
    try:
        _, cams, targets = _scene()
        # targets under another exposure per view, so that the rows train away from the identity
        gains = [0.7, 0.85, 1.15, 1.3]
        tg = [(t * g).clamp(0, 1).contiguous() for t, g in zip(targets, gains)]
        for i in range(24):
            tr.trainStep(cams[i % 4], tg[i % 4], viewKey=i % 4)
        E = tr.exposures().reshape(4, 12)
        assert all(np.abs(E[i] - np.eye(3, 4, dtype=np.float32).reshape(12)).max() > 1e-3 for i in range(4))
        keyed = tr.evaluate(cams, tg, viewKeys=[0, 1, 2, 3], color_correct=False)
        held = tr.evaluate(cams, tg, color_correct=False)
        exposed, raw = _renders(tr, r, keyed=True), _renders(tr, r)
        for i in range(4):
            _check_view(f"keyed {i}", keyed.psnr[i], keyed.ssim[i], exposed[i], _np(tg[i]), None)
            _check_view(f"held out {i}", held.psnr[i], held.ssim[i], raw[i], _np(tg[i]), None)
        assert not np.array_equal(keyed.psnr, held.psnr)
        # one view of the four, by its key
        one = tr.evaluate([cams[2]], [tg[2]], viewKeys=[2], color_correct=False)
        assert abs(one.psnr[0] - keyed.psnr[2]) <= 1e-6 and abs(one.ssim[0] - keyed.ssim[2]) <= 1e-8
        with pytest.raises(ValueError):
            tr.evaluate(cams, tg, viewKeys=[0, 1, 2, 7])
    finally:
        r.close()


def test_view_keys_render_under_the_view_s_refined_pose():
    """A pose_opt trainer: keyed views are rendered under their learnt correction (bound on the device for the forward), held-out
    views under the camera as given; the renderer's pose binding is what it was afterwards.  The device composes the camera in
    float32 and refinedCamera in float64 on the host, so the two renders agree to rounding, not to the bit: PSNR within 0.01 dB."""
    tr, r = _trainer(pose_opt=True, n_views=4, pose_lr=(3e-3, 3e-3))
    try:
        _, cams, targets = _scene()
        for i in range(16):
            tr.trainStep(cams[i % 4], targets[i % 4], viewKey=i % 4)
        assert np.abs(tr.poseCorrections()).max() > 1e-3 and r._pose == (None, None)
        keyed = tr.evaluate(cams, targets, viewKeys=[0, 1, 2, 3])
        held = tr.evaluate(cams, targets)
        assert r._pose == (None, None) and keyed.cc_psnr is None
        tg = [_np(t) for t in targets]
        for i, c in enumerate(cams):
            raw = _np(r.renderChecked(tr.model.getParams(), c, wantDepth=False).render).copy()
            _check_view(f"held out {i}", held.psnr[i], held.ssim[i], raw, tg[i], None)
            ref = _np(r.renderChecked(tr.model.getParams(), tr.refinedCamera(i, c), wantDepth=False).render).copy()
            want = mn.image_metrics(ref, tg[i])
            print(f"keyed {i}: psnr {keyed.psnr[i]:.6f} (refinedCamera {want['psnr']:.6f}, held out {held.psnr[i]:.6f})")
            assert abs(keyed.psnr[i] - want["psnr"]) <= 0.01 and abs(keyed.ssim[i] - want["ssim"]) <= 1e-3
            assert abs(keyed.psnr[i] - held.psnr[i]) > 0.02
    finally:
        r.close()


def test_background_trainers_evaluate_over_their_fixed_colour():
    from gaussiansplattingmlx_amd import background as bgm
    colour = (0.2, 0.5, 0.7)
    tr, r = _trainer(background=bgm.BackgroundConfig(mode="fixed", color=colour))
    try:
        _, cams, targets = _scene()
        rng = np.random.default_rng(4)
        alphas = [rng.random((H, W), dtype=np.float32) for _ in cams]
        res = tr.evaluate(cams, targets, targetAlphas=alphas)
        assert r._background is None
        r.setBackground(colour)
        imgs = _renders(tr, r)
        r.setBackground(None)
        for i in range(4):
            tgt = bgm.composite(_np(targets[i]), alphas[i], colour).astype(np.float32)
            _check_view(f"view {i}", res.psnr[i], res.ssim[i], imgs[i], tgt, None)
        with pytest.raises(ValueError, match="targetAlphas"):
            tr.evaluate(cams, targets)
    finally:
        r.close()


def test_argument_checks():
    tr, r = _trainer()
    try:
        _, cams, targets = _scene()
        with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
            tr.evaluate(cams, [torch.zeros(H + 1, W, 3, device="cuda")] * 4)
        with pytest.raises(ValueError, match="one entry per camera"):
            tr.evaluate(cams, targets[:3])
        with pytest.raises(ValueError, match="one entry per camera"):
            tr.evaluate(cams, targets, masks=[None])
        with pytest.raises(ValueError, match="targetAlphas"):
            tr.evaluate(cams, targets, targetAlphas=[np.ones((H, W), np.float32)] * 4)
    finally:
        r.close()
