"""An off-centre principal point on the device (camera.py Camera(cx=, cy=)): the projection kernels and
the fused render read all of proj, so the same scene through gs_projection_*, gs_render_* and a fused train step, against the
oracles; and the 3-D filter's camera table with the offset folded in (include/gsplat.h gs_set_filter3d_cameras).

Bars, fixed before the first run on the card.  Projection against the float32 oracle: test_gpu_parity's
test_projection_forward_backward -- means2d, depths, rects and radii bit for bit, colour, cov2d and conic at rtol 1e-5, the
VJP at rtol 2e-4 with an absolute floor of 2e-5 of the tensor's largest magnitude.  Against the float64 oracle the same VJP
bar; the forward at rtol 1e-4 with a floor of 1e-5 of the largest magnitude, because the float32 ORACLE is itself 3.5e-5
relative from the float64 one on this scene (cov2d and conic: the determinant's cancellation; colour 8e-5 on small
components) -- measured between the two oracles on the CPU, not on the kernels.  Render: image 1e-4 L-inf, gradients 1e-3 of
the tensor's largest magnitude (the project's bars).  Filter widths: filter3d.width_bar, with the float32 and float64 SEEN
sets coinciding (no point within 1e-3 relative of a threshold, asserted)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import filter3d as f3
from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N, K, DEGREE = 64, 48, 300, 16, 3
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
RGB_TOL, GRAD_RTOL = 1e-4, 1e-3


def _load(name):
    spec = importlib.util.spec_from_file_location("_intr_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_intrinsics_cpu")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _renderer(tile=(16, 16)):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(DEGREE, W, H, tile, False)


def _scene():
    rng = np.random.default_rng(11)
    cam = Camera(W, H, 70.0, 66.0, look_at_c2w([2.2, -2.6, 1.7]), cx=39.25, cy=18.5)
    p = dict(xyz=rng.uniform(-0.9, 0.9, (N, 3)), features_dc=rng.normal(0, 1, (N, 1, 3)),
             features_rest=rng.normal(0, 0.08, (N, K - 1, 3)), scales=rng.normal(np.log(0.05), 0.5, (N, 3)),
             rotation=rng.normal(0, 1, (N, 4)), opacity=rng.normal(0.3, 1.5, N))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, cam


def test_projection_with_an_off_centre_camera_matches_both_oracles(oracle32, oracle64):
    p, cam = _scene()
    c = cam.as_dict()
    assert c["proj"][2, 0] != 0 and c["proj"][2, 1] != 0
    shs = np.concatenate([p["features_dc"], p["features_rest"]], 1)
    rng = np.random.default_rng(5)
    cots = dict(depths=rng.normal(size=N), means2d=rng.normal(size=(N, 2)), cov2d=rng.normal(size=(N, 2, 2)),
                color=rng.normal(size=(N, 3)), conic=rng.normal(size=(N, 2, 2)) * 100)
    cots = {k: v.astype(np.float32) for k, v in cots.items()}
    r = _renderer()
    gcam = r._camera(c["view"], c["proj"], c["camCenter"], c["fovX"], c["fovY"], c["focalX"], c["focalY"])
    got = gb = None
    for name, o in (("float32", oracle32), ("float64", oracle64)):
        op, sc, rt = o.activations_forward(p["opacity"], p["scales"], p["rotation"])
        want = o.projection_forward(sc, rt, p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"],
                                    c["focalX"], c["focalY"], W, H, DEGREE)
        wb = o.projection_backward(sc, rt, p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"],
                                   c["focalX"], c["focalY"], W, H, DEGREE, cots["depths"], cots["means2d"], cots["cov2d"],
                                   cots["color"], cots["conic"])
        if got is None:          # (the kernels run once, on the float32 oracle's activations: float32 numbers for both oracles)
            sc32, rt32 = np.asarray(sc, np.float32), np.asarray(rt, np.float32)
            got = {k: _np(v) for k, v in r.projectionScreenFused(sc32, rt32, p["xyz"], shs, gcam).items()}
            gb = {k: _np(v) for k, v in r.projectionScreenFusedVJP(sc32, rt32, p["xyz"], shs, gcam, cots["means2d"], cots["depths"],
                                                                   cots["color"], cots["cov2d"], cots["conic"]).items()}
            assert (got["radii"] > 0).sum() >= 200
        if name == "float32":
            for k in ("means2d", "depths", "rectMin", "rectMax", "radii"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            np.testing.assert_allclose(got["color"], want["color"], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(got["cov2d"], want["cov2d"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(got["conic"], want["conic"], rtol=1e-5, atol=1e-9)
        else:
            np.testing.assert_array_equal(got["radii"], want["radii"])
            for k in ("means2d", "depths", "color", "cov2d", "conic"):
                w_ = np.asarray(want[k], np.float64)
                err = np.abs(got[k].astype(np.float64) - w_)
                print(f"{k} against float64: max err / bar = {(err / (1e-4 * np.abs(w_) + 1e-5 * np.abs(w_).max())).max():.3f}")
                np.testing.assert_allclose(got[k], w_, rtol=1e-4, atol=1e-5 * np.abs(w_).max(), err_msg=k)
        for k in ("gradScales", "gradRot", "gradMeans3d", "gradShs", "gradCamCenterPoint"):
            np.testing.assert_allclose(gb[k], wb[k], rtol=2e-4, atol=2e-5 * np.abs(wb[k]).max(), err_msg=f"{k} ({name})")
    # the means really are the off-centre ones: shifted by cx - W / 2 against the centred camera's
    c0 = Camera(W, H, 70.0, 66.0, cam.c2w).as_dict()
    g0 = r._camera(c0["view"], c0["proj"], c0["camCenter"], c0["fovX"], c0["fovY"], c0["focalX"], c0["focalY"])
    m0 = _np(r.projectionScreenFused(sc32, rt32, p["xyz"], shs, g0)["means2d"])
    np.testing.assert_allclose(got["means2d"] - m0, np.broadcast_to([39.25 - W / 2, 18.5 - H / 2], m0.shape), atol=1e-4)
    r.close()


def test_fused_render_with_an_off_centre_camera_matches_the_oracle(oracle32):
    from gaussiansplattingmlx_amd.scenes import perturb
    p, cam = _scene()
    c = cam.as_dict()
    o = oracle32
    fw = o.render_forward(p, c, W, H, 16, 16, DEGREE, False)
    tgt = o.render_forward(perturb(p, 99), c, W, H, 16, 16, DEGREE, False)["color"].reshape(H, W, 3)
    r = _renderer()
    res = r.renderForward({k: torch.as_tensor(v) for k, v in p.items()}, cam, want_radii=True)
    img = _np(res.render)
    err = np.abs(img.reshape(-1, 3) - fw["color"]).max()
    print(f"image: max err {err:.2e} (bar {RGB_TOL:.0e}), max {fw['color'].max():.3f}")
    assert fw["color"].max() > 0.2 and err <= RGB_TOL
    np.testing.assert_array_equal(_np(res.radii), fw["proj"]["radii"])
    loss, cc, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), tgt, 0.2)
    lo, gc, _ = r.lossForwardBackward(res.render, tgt, 0.2)
    assert abs(_np(lo)[0] - loss) < 1e-5
    want = o.render_backward(p, c, W, H, 16, 16, DEGREE, fw, cc.reshape(-1, 3), np.zeros(W * H, np.float32),
                             np.zeros(W * H, np.float32), False)
    got = r.renderBackward(gc)
    for k in KEYS:
        rel = _rel(_np(got[k]), want[k].reshape(_np(got[k]).shape))
        print(f"grad {k}: rel {rel:.2e} (bar {GRAD_RTOL:.0e})")
        assert rel <= GRAD_RTOL, k
    # the centred camera renders something else: the offset reaches the image
    img0 = _np(r.renderForward({k: torch.as_tensor(v) for k, v in p.items()}, Camera(W, H, 70.0, 66.0, cam.c2w)).render)
    assert np.abs(img0 - img).max() > 0.05
    r.close()


@pytest.mark.parametrize("fuse", [True, False])
def test_a_fused_train_step_runs_with_an_off_centre_camera(fuse):
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cam = _scene()
    r = _renderer()
    target = r.renderForward({k: torch.as_tensor(v, device=r.device) for k, v in perturb(p, 5, 0.1).items()}, cam).render.clone()
    model = GaussModel(p, r.device)
    start = _np(model.arena).copy()
    tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse)
    for _ in range(2):
        loss = tr.trainStep(cam, target, viewKey=0)
    assert np.isfinite(_np(loss)).all() and np.isfinite(_np(model.arena)).all()
    assert np.abs(_np(model.arena) - start).max() > 0
    r.close()


def test_filter_width_of_off_centre_cameras():
    x, cams = cpu.off_centre_filter_scene(N=500)
    assert len(cams) == 3 and f3.threshold_distance(x, cams) >= 1e-3       # the condition: float32 and float64 see the same set
    want, seen, arg = f3.filter_width(x, cams, details=True)
    centred, seen0, _ = f3.filter_width(x, cams, details=True, fold=False)
    _, sets = cpu._direct_width(x, cams)
    _, sets0 = cpu._direct_width(x, cams, centred=True)
    assert (sets != sets0).any(axis=0).sum() >= 1 and (want != centred).any() and 0.2 < seen.mean() < 1.0
    r = _renderer()
    xt = torch.as_tensor(x, device="cuda")
    r.setFilterCameras(cams)
    got = _np(r.computeFilter3D(xt)).astype(np.float64)
    bar = f3.width_bar(x, cams)
    err = np.abs(got - want)
    print(f"off-centre widths: max err / bar = {(err / bar).max():.3f}; {int((want != centred).sum())} widths differ from the centred table's")
    assert np.all(err <= bar), float((err / bar).max())
    # a centred table: the fold is skipped, the rule is the one without the principal point
    plain = [Camera(c.imageWidth, c.imageHeight, c.focalX, c.focalY, c.c2w) for c in cams]
    r.setFilterCameras(plain)
    got0 = _np(r.computeFilter3D(xt))
    bar0 = f3.width_bar(x, plain)
    assert np.all(np.abs(got0.astype(np.float64) - centred) <= bar0)
    np.testing.assert_array_equal(f3.filter_width(x, plain), centred)
    # ... and the same bits from structs whose proj carries no offset at all (what a caller without proj hands over)
    bare = []
    for c in plain:
        g = r._camera(c.worldViewTransform, np.zeros(16, np.float32), c.cameraCenter, c.FoVx, c.FoVy, c.focalX, c.focalY)
        bare.append(g)
    r.setFilterCameras(bare)
    np.testing.assert_array_equal(_np(r.computeFilter3D(xt)), got0)
    r.close()
