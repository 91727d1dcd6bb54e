"""Every MODE 2 form of the fused projection backward (csrc/projection.hip, proj_bwd_fused_kernel<2, POSE, AA, MCMC, F3D, SPARSE>)
against the unfused step of the same options: {plain, 3-D filter, MCMC, sparse Adam} x pose refinement x anti-aliasing, through the
trainer.  fuse_adam=True runs the MODE 2 form of the combination (gs_render_backward_adam); fuse_adam=False runs the MODE 0 plain /
F3D / POSE forms (gs_render_backward) and the op-level Adam, regularisers and noise.  The per-feature tests pair most forms; the
crossings (POSE x MCMC x AA, POSE x SPARSE x AA, ...) are paired only here.

Shape: two trainSteps on one 160 x 120 view, N = 321 at K = 25 / degree 4 -- two full 128-thread workgroups and a third of one full
wave and a one-row wave; the rows (72 floats) stay in registers from the staging load to the update (adam_rows_kept).  The plain form
also at K = 16: rows of 45 floats, not a multiple of four, the scalar staging (adam_rows).  The cloud reaches past the view's edges
and behind the camera (some 30 rows are invisible, a few in every full wave), so sparse Adam has invisible rows.

Bar: test_fused_backward_adam_matches_backward_then_adam's (tests/test_gpu_parity.py) -- at most a share 1e-3 of the elements further
than 1e-3 of the reference's largest magnitude from the unfused run, for the arena (as its change over the two steps, which must not be
zero), m, v and xyzGradAccumulation (all zero under the MCMC strategy, non-zero elsewhere); the pose correction, where there is one,
the same way.  The blend backward's float atomics rule out bit equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H, N = 160, 120, 321
STEPS = 2
TOL, SHARE = 1e-3, 1e-3
DEGREE = {25: 4, 16: 3}
FEATURES = ("plain", "f3d", "mcmc", "sparse")
CASES = [(f, pose, aa, 25) for f in FEATURES for pose in (False, True) for aa in (False, True)] + [("plain", False, False, 16)]
_scenes = {}


def _np(t):
    return t.detach().cpu().numpy()


def _scene(K):
    """(params, camera, target, visible) -- test_gpu_parity's _scene with the cloud spread beyond the view's edges."""
    if K in _scenes:
        return _scenes[K]
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import perturb
    rng = np.random.default_rng(65)
    cam = Camera(W, H, 0.9 * W, 0.9 * W * 1.02, look_at_c2w([2.2, -2.6, 1.7]))
    p = dict(xyz=rng.uniform(-5.0, 5.0, (N, 3)), features_dc=rng.normal(0, 1, (N, 1, 3)),
             features_rest=rng.normal(0, 0.08, (N, K - 1, 3)), scales=rng.normal(np.log(0.12), 0.5, (N, 3)),
             rotation=rng.normal(0, 1, (N, 4)), opacity=rng.normal(0.3, 1.5, N))
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    r = GaussianRenderer(DEGREE[K], W, H, (16, 16), False)
    dev = lambda q: {k: torch.as_tensor(v, device=r.device) for k, v in q.items()}      # noqa: E731
    vis = _np(r.renderForward(dev(p), cam, want_radii=True).radii) > 0
    target = r.renderForward(dev(perturb(p, 5, 0.1)), cam).render.clone()
    r.close()
    # some rows off screen, most on; the last (one-row) wave's row and rows of every other wave on
    waves = np.pad(vis, (0, -N % 64)).reshape(-1, 64).sum(axis=1)
    print(f"K={K}: {int(vis.sum())} of {N} visible, per wave {waves.tolist()}")
    assert 16 <= int((~vis).sum()) < N // 2 and (waves > 0).all()
    _scenes[K] = (p, cam, target, vis)
    return _scenes[K]


def _run(feature, pose, aa, K, fuse):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cam, target, _ = _scene(K)
    r = GaussianRenderer(DEGREE[K], W, H, (16, 16), False, antialiased=aa)
    kw = dict(iterationCount=1000, fuse_adam=fuse)      # (densify on: the kernels feed xyzGradAccumulation; two steps reach no event)
    if pose:
        kw.update(pose_opt=True, n_views=1, pose_lr=(1e-3, 1e-3))
    if feature == "f3d":
        kw.update(filter_3d=True, filter_cameras=[cam])
    elif feature == "mcmc":
        kw.update(strategy="mcmc", mcmc=MCMCConfig(cap_max=N, refine_start=10**6))
    elif feature == "sparse":
        kw.update(sparse_adam=True)
    model = GaussModel(p, r.device)
    start = _np(model.arena).copy()
    tr = GaussianTrainer(model, r, **kw)
    for _ in range(STEPS):      # (pose: the correction starts at zero and has moved by the second step)
        loss = tr.trainStep(cam, target, viewKey=0)
    assert np.isfinite(_np(loss)).all()
    out = dict(arena=_np(model.arena) - start, m=_np(model.m).copy(), v=_np(model.v).copy(),
               xyzGradAccumulation=_np(tr.xyzGradAccumulation).copy())
    if pose:
        out["pose_delta"] = tr.poseCorrections()[0].copy()
    r.close()
    return out


@pytest.mark.parametrize("feature,pose,aa,K", CASES,
                         ids=[f"{f}{'-pose' if q else ''}{'-aa' if a else ''}-K{K}" for f, q, a, K in CASES])
def test_fused_form_matches_unfused_step(feature, pose, aa, K):
    got, want = _run(feature, pose, aa, K, True), _run(feature, pose, aa, K, False)
    assert sorted(got) == sorted(want)
    assert np.abs(want["arena"]).max() > 0
    for k in sorted(want):
        a, b = got[k].astype(np.float64), want[k].astype(np.float64)
        scale = np.abs(b).max()
        share = float(np.mean(np.abs(a - b) > TOL * scale))
        print(f"{feature} pose={pose} aa={aa} K={K} {k}: max|ref| {scale:.3e}, max|diff| {np.abs(a - b).max():.3e}, "
              f"share beyond {TOL:.0e} max|ref| = {share:.2e} (bar {SHARE:.0e})")
        # (the MCMC strategy keeps no densification statistic: zero in both runs, and compared as such)
        assert scale > 0 or (k == "xyzGradAccumulation" and feature == "mcmc"), k
        assert share < SHARE, k
