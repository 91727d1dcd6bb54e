"""The fisheye camera model on the device (include/gsplat.h gs_set_camera_model; csrc/gs_math.h fisheye_map
and the FISHEYE forms of csrc/projection.hip) against the numpy restatement tests/fisheye_numpy.py.

Scene (fisheye_numpy.scene): 64 x 48, N = 300, K = 16, the camera inside the cloud so that theta runs from 0 to about 80 degrees,
principal point (30.5, 25.25), and hand-placed rows: on the axis, either side of the series threshold, z either side of 0.2, behind
the camera, and one at z = 0.21 with r / z = 5.4.

Bars, fixed before the first run on the card.
1. Op-level.  means2d, depths, radii, rects: the float32 restatement's bits (it is built from mul, add, div and sqrt in the kernel's
   order, and projection.hip is compiled without FMA contraction), on the rows where the restatement's two precisions agree on
   ceil(sqrt(lambda_max)) -- at most 1 % of rows may differ there (this seed: none).  cov2d, conic and the three gradients: four
   times the distance between the float32 and the float64 restatement on this scene, each as max |a - b| / max |b| over all
   rows.  Measured distances: cov2d 3.28e-7, conic 3.63e-7, gradMeans3d 2.00e-7, gradScales 2.68e-7, gradRot 3.70e-7; the bars
   are 1.32e-6, 1.46e-6, 8.1e-7, 1.08e-6, 1.48e-6.  The test recomputes the distances and asserts they are the recorded ones.
2. Fused render against the oracle's pack_gaussians -> tile_bin -> blend_forward fed by the restated projection (colours from the
   oracle's projection_forward): image, depth, alpha 1e-4 L-inf; gradients 1e-3 of each tensor's largest magnitude: the
   project's bars (test_gpu_parity, smoke()).
3. Fused backward + Adam against backward then Adam: test_gpu_antialiasing's share bar, mean(|a - b| > 1e-3 max|b|) < 1e-3.
4. Switching: images byte-identical; gradients within 2.6e-5 of the tensor's largest magnitude, the largest run-to-run ratio
   DESIGN.md section 21 records for the backward's atomics (features_rest, 1.0e-8 on 3.95e-4) -- and bit-equal where the fresh
   context is itself run-to-run identical.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisheye_numpy as F  # noqa: E402

from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
W, H, N, K, DEGREE = F.SCENE_W, F.SCENE_H, F.SCENE_N, F.SCENE_K, F.SCENE_DEGREE
IMG_BAR, GRAD_BAR, SHARE_TOL, SHARE, RERUN_BAR = 1e-4, 1e-3, 1e-3, 1e-3, 2.6e-5
DIST = dict(cov2d=3.28e-7, conic=3.63e-7, gradMeans3d=2.00e-7, gradScales=2.68e-7, gradRot=3.70e-7)      # measured (header)
OP_BARS = dict(cov2d=1.32e-6, conic=1.46e-6, gradMeans3d=8.1e-7, gradScales=1.08e-6, gradRot=1.48e-6)   # 4 x


def _camera(model="fisheye", c2w=None):
    return Camera(W, H, *F.SCENE_FOCAL, F.scene_c2w() if c2w is None else c2w, cx=F.SCENE_PRINCIPAL[0], cy=F.SCENE_PRINCIPAL[1],
                  model=model)


def _renderer(tile=(16, 16), aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(DEGREE, W, H, tile, False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _cots(seed=9):
    rng = np.random.default_rng(seed)
    return dict(means2d=rng.standard_normal((N, 2)).astype(np.float32), depths=rng.standard_normal(N).astype(np.float32),
                cov2d=rng.standard_normal((N, 2, 2)).astype(np.float32), conic=rng.standard_normal((N, 2, 2)).astype(np.float32),
                color=rng.standard_normal((N, 3)).astype(np.float32))


@pytest.fixture(scope="module")
def restated():
    """The scene and both restatements of its projection and VJP, computed once."""
    p, pv = F.scene()
    cam = _camera()
    c = cam.as_dict()
    s32, q32 = F.activated(p, np.float32)
    m32 = p["xyz"]
    cot = _cots()
    f32 = F.project(s32, q32, m32, c, W, H, np.float32)
    f64 = F.project(s32.astype(np.float64), q32.astype(np.float64), m32.astype(np.float64), c, W, H, np.float64)
    g32 = F.project_vjp(s32, q32, m32, c, W, H, cot["means2d"], cot["depths"], cot["cov2d"], cot["conic"], np.float32, f32)
    g64 = F.project_vjp(s32.astype(np.float64), q32.astype(np.float64), m32.astype(np.float64), c, W, H, cot["means2d"],
                        cot["depths"], cot["cov2d"], cot["conic"], np.float64, f64)
    return dict(p=p, pv=pv, cam=cam, s=s32, q=q32, cot=cot, f32=f32, f64=f64, g32=g32, g64=g64)


# ------------------------------------------------------------------------------------------------------ 1. op-level projection
def test_op_level_projection_matches_the_restatement(restated, oracle32):
    R = restated
    p, cam, f32, f64 = R["p"], R["cam"], R["f32"], R["f64"]
    for k, d in DIST.items():          # the bars stand on these distances
        now = _rel((f32 if k in f32 else R["g32"])[k], (f64 if k in f64 else R["g64"])[k])
        print(f"restatements apart, {k}: {now:.3e} (recorded {d:.3e})")
        assert abs(now - d) <= 0.01 * d, (k, now, d)
    r = _renderer()
    r.setCameraModel("fisheye")
    assert r.cameraModel == "fisheye"
    got_model = C.c_int(-1)
    assert r.lib.gs_get_camera_model(r.ctx, C.byref(got_model)) == 0 and got_model.value == 1
    gcam = r._camera(cam.worldViewTransform, cam.projectionMatrix, cam.cameraCenter, cam.FoVx, cam.FoVy, cam.focalX, cam.focalY)
    shs = np.concatenate([p["features_dc"], p["features_rest"]], 1)
    out = {k: _np(v) for k, v in r.projectionScreenFused(R["s"], R["q"], p["xyz"], shs, gcam).items()}
    tie = np.ceil(np.sqrt(f32["lambdaMax"])) != np.ceil(np.sqrt(f64["lambdaMax"]))
    print(f"radius ties between the restatement's precisions: {int(tie.sum())} of {N} rows")
    assert tie.sum() <= N // 100
    keep = ~tie
    for k in ("means2d", "depths", "radii", "rectMin", "rectMax"):
        a, b = out[k][keep], f32[k][keep]
        bad = int((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(1).sum())
        print(f"{k}: {bad} rows differ from the float32 restatement's bits; largest difference {np.abs(a.astype(np.float64) - b).max():.3e}")
        assert np.array_equal(a, b), k
    hand = F.HAND_ROWS
    assert out["radii"][hand["z_below_near"]] == 0 and out["radii"][hand["behind"]] == 0
    assert out["radii"][hand["z_at_near"]] > 0 and out["radii"][hand["steep"]] > 0 and out["radii"][hand["on_axis"]] > 0
    assert out["means2d"][hand["on_axis"]].tolist() == [30.0, 24.75]
    for k in ("cov2d", "conic"):
        e = _rel(out[k], f64[k])
        print(f"{k} against float64: {e:.3e} (bar {OP_BARS[k]:.2e})")
        assert np.isfinite(out[k]).all() and e <= OP_BARS[k], k
    # colour does not depend on the model: the oracle's own
    c = cam.as_dict()
    pin = oracle32.projection_forward(R["s"], R["q"], p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"],
                                      c["focalX"], c["focalY"], W, H, DEGREE)
    assert np.abs(out["color"] - pin["color"]).max() <= 1e-5
    cot = R["cot"]
    g = {k: _np(v) for k, v in r.projectionScreenFusedVJP(R["s"], R["q"], p["xyz"], shs, gcam, cot["means2d"], cot["depths"],
                                                         np.zeros((N, 3), np.float32), cot["cov2d"], cot["conic"]).items()}
    for k in ("gradMeans3d", "gradScales", "gradRot"):
        e = _rel(g[k], R["g64"][k])
        print(f"{k} against float64: {e:.3e} (bar {OP_BARS[k]:.2e})")
        assert np.isfinite(g[k]).all() and e <= OP_BARS[k], k
    # and the setting reaches nothing else: back to pinhole, the op is what a context that never left it computes
    r.setCameraModel("pinhole")
    back = r.projectionScreenFused(R["s"], R["q"], p["xyz"], shs, gcam)
    never = _renderer().projectionScreenFused(R["s"], R["q"], p["xyz"], shs, gcam)
    front = torch.as_tensor(R["pv"][:, 2] >= 0.2, device="cuda")
    for k in back:
        assert torch.equal(back[k][front], never[k][front]), k
    assert np.array_equal(_np(back["radii"]), pin["radii"])


# ------------------------------------------------------------------------------------------------------------- 2. fused render
class FisheyeOracle:
    """The oracle's composed pipeline (Oracle.render_forward / render_backward) with the restated fisheye projection in place of
    its pinhole one; colours and their gradients stay the oracle's."""

    def __init__(self, o):
        self.o = o

    def _proj(self, p, c, sc, rt, shs):
        o = self.o
        dt = o.dtype
        pin = o.projection_forward(sc, rt, p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"], c["focalX"],
                                   c["focalY"], W, H, DEGREE)
        fe = F.project(np.asarray(sc, dt), np.asarray(rt, dt), np.asarray(p["xyz"], dt), c, W, H, dt)
        return pin, fe

    def render_forward(self, p, c, tile):
        o = self.o
        op, sc, rt = o.activations_forward(p["opacity"], p["scales"], p["rotation"])
        shs = np.concatenate([o._r(p["features_dc"]), o._r(p["features_rest"])], axis=1)
        pin, fe = self._proj(p, c, sc, rt, shs)
        packed = o.pack_gaussians(fe["means2d"], fe["conic"], pin["color"], op, fe["depths"])
        bn = o.tile_bin(fe["rectMin"], fe["rectMax"], fe["radii"], fe["depths"], W, H, tile[0], tile[1])
        color, depth, alpha, last = o.blend_forward(packed, bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], False)
        return dict(scales=sc, rot=rt, shs=shs, fe=fe, packed=packed, bin=bn, color=color, depth=depth, alpha=alpha, last=last)

    def render_backward(self, p, c, tile, fw, cotColor):
        o = self.o
        dt = o.dtype
        z = np.zeros(W * H, dt)
        bn = fw["bin"]
        gp = o.blend_backward(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, tile[0], tile[1], False, cotColor, z, z, fw["color"],
                              fw["depth"], fw["alpha"], fw["last"])
        zero = lambda *s: np.zeros(s, dt)      # noqa: E731
        col = o.projection_backward(fw["scales"], fw["rot"], p["xyz"], fw["shs"], c["camCenter"], c["view"], c["proj"], c["fovX"],
                                    c["fovY"], c["focalX"], c["focalY"], W, H, DEGREE, zero(N), zero(N, 2), zero(N, 4), gp[:, 6:9],
                                    zero(N, 4))
        live = np.abs(gp).max(axis=1) > 0
        d = np.where(live[:, None], -np.nan_to_num(col["gradCamCenterPoint"]), 0.0)      # the view-direction term of the means
        geo = F.project_vjp(fw["scales"], fw["rot"], p["xyz"], c, W, H, gp[:, 0:2], gp[:, 10], zero(N, 4), gp[:, 2:6], dt, fw["fe"])
        for k in geo:           # a row no pixel blended: exactly zero (the fused path's rule)
            geo[k] = np.where(live[:, None], geo[k], 0.0)
        do, ds, dq = o.activations_backward(p["opacity"], p["scales"], p["rotation"], gp[:, 9], geo["gradScales"], geo["gradRot"])
        return dict(xyz=geo["gradMeans3d"] + d, features_dc=col["gradShs"][:, :1, :].copy(), features_rest=col["gradShs"][:, 1:, :].copy(),
                    scales=ds, rotation=dq, opacity=do.reshape(np.shape(p["opacity"])))


def _target(r, p, cam):
    from gaussiansplattingmlx_amd.scenes import perturb
    return r.renderForward(_dev(perturb(p, 5, 0.1)), cam).render.clone()


@pytest.mark.parametrize("tile", [(16, 16), (W // 4, H // 4)])
def test_fused_render_matches_the_composed_oracle(restated, oracle32, tile):
    p, cam = restated["p"], restated["cam"]
    r = _renderer(tile)
    assert r.blockLists == (tile != (16, 16))
    target = _target(r, p, cam)
    res = r.renderForward(_dev(p), cam, want_radii=True)
    assert r.cameraModel == "fisheye"
    img, depth, alpha, radii = (_np(x).copy() for x in (res.render, res.depth, res.alpha, res.radii))
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    g = {k: _np(v) for k, v in r.renderBackward(cot).items()}
    fo = FisheyeOracle(oracle32)
    c = cam.as_dict()
    fw = fo.render_forward(p, c, tile)
    e = (np.abs(img.reshape(-1, 3) - fw["color"]).max(), np.abs(depth.reshape(-1) - fw["depth"]).max(), np.abs(alpha.reshape(-1) - fw["alpha"]).max())
    print(f"tile {tile}: image {e[0]:.3e}, depth {e[1]:.3e}, alpha {e[2]:.3e} (bar {IMG_BAR:.0e}); M = {r.stats()['M']}, "
          f"{int((radii > 0).sum())} visible, alpha max {alpha.max():.3f}")
    assert np.array_equal(radii, fw["fe"]["radii"])
    assert alpha.max() > 0.5 and e[0] <= IMG_BAR and e[2] <= IMG_BAR and e[1] <= IMG_BAR * max(1.0, float(np.abs(fw["depth"]).max()))
    want = fo.render_backward(p, c, tile, fw, _np(cot).reshape(-1, 3))
    for k in KEYS:
        err = _rel(g[k].reshape(-1), np.asarray(want[k]).reshape(-1))
        print(f"tile {tile}: grad {k} {err:.3e} of max {np.abs(want[k]).max():.3e} (bar {GRAD_BAR:.0e})")
        assert np.isfinite(g[k]).all() and np.abs(want[k]).max() > 0 and err <= GRAD_BAR, k


# ---------------------------------------------------------------------------------------------------- 3. fused backward + Adam
def _rows(model, name):
    return {k: _np(v).copy() for k, v in model._carve(getattr(model, name), model.N, model.stride).items()}


@pytest.mark.parametrize("variant", ["plain", "aa", "sparse", "mcmc"])
def test_fused_adam_matches_backward_then_adam(restated, variant):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cam = restated["p"], restated["cam"]
    r = _renderer(aa=variant == "aa")
    target = _target(r, p, cam)
    kw = dict(sparse=dict(sparse_adam=True, densify=False), mcmc=dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=N + 100, refine_start=10**6)))
    out = {}
    for fuse in (True, False):
        model = GaussModel(p, r.device)
        start = {n: _rows(model, n) for n in ("arena", "m", "v")}
        tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse, **kw.get(variant, dict(densify=False)))
        tr.trainStep(cam, target)
        assert r.cameraModel == "fisheye"
        out[fuse] = {n: _rows(model, n) for n in ("arena", "m", "v")}
    vis = restated["f32"]["radii"] > 0
    for n in ("arena", "m", "v"):
        for k in KEYS:
            a, b = out[True][n][k].astype(np.float64), out[False][n][k].astype(np.float64)
            if n == "arena":
                a, b = a - start[n][k], b - start[n][k]
            share = float(np.mean(np.abs(a - b) > SHARE_TOL * np.abs(b).max()))
            print(f"{variant} {n}.{k}: share beyond {SHARE_TOL:.0e} max|b| = {share:.2e} (bar {SHARE:.0e}), max|b| {np.abs(b).max():.3e}")
            assert np.abs(b).max() > 0 and share < SHARE, (variant, n, k)
            if variant == "sparse":      # invisible rows keep their bits
                x, y = out[True][n][k][~vis], start[n][k][~vis]
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (n, k)
    if variant == "sparse":
        assert 0 < int((~vis).sum())


# ----------------------------------------------------------------------------------------------- 4. switching leaves nothing
def _step(r, params, cam, target):
    res = r.renderForward(params, cam)
    img, alpha, depth = res.render.clone(), res.alpha.clone(), res.depth.clone()
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    return img, alpha, depth, {k: v.clone() for k, v in r.renderBackward(cot).items()}


def test_switching_models_leaves_nothing_behind(restated):
    p = restated["p"]
    fish, pin = restated["cam"], _camera("pinhole")
    params = _dev(p)
    fresh = _renderer()
    target = _target(fresh, p, pin)
    a = _step(fresh, params, pin, target)
    b = _step(fresh, params, pin, target)
    r = _renderer()
    first = _step(r, params, pin, target)
    mid = _step(r, params, fish, target)
    assert r.cameraModel == "fisheye" and float((mid[0] - first[0]).abs().max()) > 1e-2      # (the models differ on this scene)
    c = _step(r, params, pin, target)
    assert r.cameraModel == "pinhole"
    for i in range(3):
        assert torch.equal(a[i], c[i]) and torch.equal(a[i], first[i]), i
    for k in KEYS:
        if torch.equal(a[3][k], b[3][k]):
            assert torch.equal(a[3][k], c[3][k]), k
        else:
            assert float((a[3][k] - c[3][k]).abs().max()) <= RERUN_BAR * float(a[3][k].abs().max()), k


def test_backward_uses_its_forwards_model(restated):
    p, fish = restated["p"], restated["cam"]
    params = _dev(p)
    r = _renderer()
    target = torch.zeros(H, W, 3, device="cuda")
    want = _step(r, params, fish, target)[3]
    res = r.renderForward(params, fish)
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.setCameraModel("pinhole")          # between the forward and its backward: changes nothing for that pair
    got = r.renderBackward(cot)
    for k in KEYS:
        assert _rel(_np(got[k]), _np(want[k])) <= RERUN_BAR, k


# ----------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_context_usable(restated):
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd.renderer import GsplatError
    p, fish = restated["p"], restated["cam"]
    params = _dev(p)
    r = _renderer()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    good = r.renderForward(params, fish).render.clone()
    err = lambda: r.lib.gs_last_error(r.ctx).decode()      # noqa: E731
    # the setter keeps its value
    for bad in (2, -1, 255):
        assert r.lib.gs_set_camera_model(r.ctx, bad) == invalid and "gs_set_camera_model" in err()
    assert r.lib.gs_get_camera_model(r.ctx, None) == invalid
    assert torch.equal(r.renderForward(params, fish).render, good)
    # a fisheye forward under a pose correction or a 3-D filter
    delta, grad = torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda")
    r.setPoseCorrection(delta, grad)
    with pytest.raises(GsplatError, match="pose"):
        r.renderForward(params, fish)
    r.setPoseCorrection(None, None)
    r.setFilter3D(torch.zeros(N, device="cuda"))
    with pytest.raises(GsplatError, match="filter"):
        r.renderForward(params, fish)
    r.setFilter3D(None)
    assert torch.equal(r.renderForward(params, fish).render, good)
    # the data-parallel entry points and the filter's cameras, behind a fisheye forward and beside the setting
    for beside in (False, True):
        if beside:
            r.renderForward(params, _camera("pinhole"))
            r.setCameraModel("fisheye")
        calls = dict(gs_render_backward_dp_begin=lambda: r.lib.gs_render_backward_dp_begin(r.ctx, None, None, None, None),
                     gs_render_backward_dp_finish=lambda: r.lib.gs_render_backward_dp_finish(r.ctx, None, None, None, None),
                     gs_render_backward_dp_finish_geom=lambda: r.lib.gs_render_backward_dp_finish_geom(r.ctx, None, None, None, None, None),
                     gs_render_backward_dp_geom=lambda: r.lib.gs_render_backward_dp_geom(r.ctx, *([None] * 9)),
                     gs_render_backward_dp=lambda: r.lib.gs_render_backward_dp(r.ctx, *([None] * 8)),
                     gs_dp_step=lambda: r.lib.gs_dp_step(r.ctx, 0, None))
        for name, call in calls.items():
            assert call() == invalid, name
            assert "fisheye" in err() and ("gs_dp_step" if name == "gs_dp_step" else "gs_render_backward_dp") in err(), (name, err())
        with pytest.raises(GsplatError, match="fisheye"):
            r.setFilterCameras([fish])
    assert torch.equal(r.renderForward(params, fish).render, good)
    _, cot, _ = r.lossForwardBackward(r.renderForward(params, fish).render, torch.zeros(H, W, 3, device="cuda"), 0.2)
    g = r.renderBackward(cot)
    assert all(bool(torch.isfinite(v).all()) for v in g.values())


def test_trainer_refuses_what_the_model_does_not_serve(restated):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, fish = restated["p"], restated["cam"]
    r = _renderer()
    target = torch.zeros(H, W, 3, device="cuda")
    cases = dict(pose_opt=dict(pose_opt=True, n_views=1), filter_3d=dict(filter_3d=True, filter_cameras=[_camera("pinhole")]),
                 views_per_rank=dict(views_per_rank=2))
    for name, kw in cases.items():
        tr = GaussianTrainer(GaussModel(p, r.device), r, iterationCount=1000, densify=False, **kw)
        with pytest.raises(ValueError, match="fisheye"):
            tr.trainStep(fish, target, viewKey=0)
    # the data-parallel steps: the library's own exchange on a one-rank communicator, and a one-rank process group
    import socket
    import torch.distributed as dist
    from gaussiansplattingmlx_amd import _lib
    uid = C.create_string_buffer(_lib.GS_DP_UNIQUE_ID_BYTES)
    assert r.lib.gs_dp_unique_id(uid) == 0
    tr = GaussianTrainer(GaussModel(p, r.device), r, iterationCount=1000, densify=False, exchange_when_single=True,
                         exchange_impl="native", dp_bootstrap=(uid.raw, 0, 1))
    with pytest.raises(ValueError, match="fisheye"):
        tr.trainStep(fish, target, stepCameras=[fish])
    assert np.isfinite(float(tr.trainStep(_camera("pinhole"), target, stepCameras=[_camera("pinhole")])[0]))      # (a pinhole view steps)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=r.device)
    try:
        tr = GaussianTrainer(GaussModel(p, r.device), r, iterationCount=1000, densify=False, process_group=dist.group.WORLD,
                             exchange_when_single=True)
        with pytest.raises(ValueError, match="fisheye"):
            tr.trainStep(fish, target, stepCameras=[fish])
    finally:
        dist.destroy_process_group()
    # and a plain trainer still steps through the fisheye camera on the same renderer
    tr = GaussianTrainer(GaussModel(p, r.device), r, iterationCount=1000, densify=False)
    assert np.isfinite(float(tr.trainStep(fish, target)[0]))
    assert r.cameraModel == "fisheye"


# ------------------------------------------------------------------------------------------------------------------ 7. trainer
def test_trainer_trains_through_fisheye_cameras(restated):
    from gaussiansplattingmlx_amd import adc
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p = restated["p"]
    eyes = [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((-0.5, 0.3, 0.2), (1.0, 0.0, 0.0)), ((-0.3, -0.4, 0.1), (1.5, 0.0, 0.0)),
            ((0.2, 0.2, -0.3), (2.0, 0.0, 0.2))]
    cams = [_camera(c2w=look_at_c2w(e, t)) for e, t in eyes]
    r = _renderer()
    targets = [r.renderChecked(_dev(p), c).render.clone() for c in cams]
    model = GaussModel(perturb(p, 5, 0.3), r.device)
    cfg = adc.ADCConfig(scene_extent=adc.scene_extent(cams), densify_from=20, densify_interval=20, opacity_reset_interval=60,
                        densify_until=160)
    tr = GaussianTrainer(model, r, iterationCount=1000, strategy="adc", adc=cfg, densify=False)
    tr.maxGaussians = 4 * N
    n0 = model.N
    losses = [float(tr.trainStep(cams[i % 4], targets[i % 4], viewKey=i % 4)[0]) for i in range(40)]
    print(f"losses {losses[0]:.5f} -> {losses[-1]:.5f}; N {n0} -> {model.N}; ADC events {getattr(tr, 'lastADCStats', None)}")
    assert np.isfinite(losses).all() and np.mean(losses[-4:]) < np.mean(losses[:4]), losses
    assert all(bool(torch.isfinite(v).all()) for v in model.getParams().values())
    st = getattr(tr, "lastADCStats", None)
    assert st is not None and st["split"] + st["clone"] > 0 and model.N > n0, (st, n0, model.N)      # the event inside the 40 steps densified
    ev = tr.evaluate([cams[0]], [targets[0]])
    assert np.isfinite(ev.psnr).all(), ev


# ---------------------------------------------------------------------------------------------------- 6. gs_undistort_fisheye
# tests/test_gpu_undistort.py's sizes, sources and rules (`_compare`: values inside lens.remap_bar on the pixels both sides call
# valid; validity flags equal except within delta of the source's border or of the fold; a mask one level off only at a .5
# boundary; every exception set capped at 1 % of the pixels), with the fisheye lens in place of the radial-tangential one.
FE_SIMPLE = dict(k1=0.08)
FE_RADIAL = dict(k1=-0.15, k2=0.03)
FE_POS = dict(k1=0.11, k2=-0.03, k3=0.004, k4=-0.001)
FE_NEG = dict(k1=-0.12, k2=0.02, k3=-0.003, k4=0.0004)
FE_FOLD = dict(k1=-0.35)                 # d theta_d / d theta = 0 at theta^2 = 0.952: inside the 80 x 50 destination below
LENS_CASES = {
    "67x45_c3_neg": ((67, 45), 3, FE_NEG, None, None, "color", 1),
    "67x45_c3_pos": ((67, 45), 3, FE_POS, None, None, "color", 2),
    "64x4_c1_simple": ((67, 45), 1, FE_SIMPLE, (60.0, 58.0, 32.0, 2.0), (64, 4), "color", 3),
    "1x1_c4_radial": ((67, 45), 4, FE_RADIAL, (60.0, 58.0, 0.5, 0.5), (1, 1), "color", 4),
    "80x50_c4_pos": ((67, 45), 4, FE_POS, (52.0, 50.5, 41.0, 24.75), (80, 50), "color", 5),
    "80x50_c4_fold": ((67, 45), 4, FE_FOLD, (30.0, 30.0, 40.0, 25.0), (80, 50), "color", 12),
    "203x131_c4_radial": ((211, 140), 4, FE_RADIAL, (150.0, 151.0, 100.5, 66.25), (203, 131), "color", 6),
    "67x45_2d_simple": ((67, 45), 0, FE_SIMPLE, None, None, "color", 7),
    "67x45_mask_neg": ((67, 45), 0, FE_NEG, None, None, "mask", 8),
    "130x70_mask_pos": ((120, 66), 0, FE_POS, (100.0, 99.0, 66.5, 34.0), (130, 70), "mask", 9),
    "67x45_depth_radial": ((67, 45), 0, FE_RADIAL, None, None, "depth", 10),
    "90x61_depth_pos": ((67, 45), 0, FE_POS, (70.0, 69.0, 45.0, 30.5), (90, 61), "depth", 11),
}
_und = None


def _lens_case(cid):
    """(image, lens, dstK, dstSize, mode) with the float64 statement computed once and left in test_gpu_undistort's cache, where
    its `_compare` looks the case up."""
    global _und
    import importlib.util
    from gaussiansplattingmlx_amd import lens as L
    if _und is None:
        spec = importlib.util.spec_from_file_location("_fe_test_gpu_undistort", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_undistort.py"))
        _und = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_und)
    key = "fisheye_" + cid
    if key not in _und._cache:
        (sw, sh), ch, coeff, dstK, dstSize, mode, seed = LENS_CASES[cid]
        rng = np.random.default_rng(seed)
        shape = (sh, sw) if ch == 0 else (sh, sw, ch)
        if mode == "mask":
            img = rng.integers(0, 256, shape, dtype=np.uint8)
        elif mode == "depth":
            img = rng.uniform(0.5, 5.0, shape).astype(np.float32)
            img[rng.uniform(size=shape) < 0.2] = 0.0
        else:
            img = rng.uniform(0.0, 1.0, shape).astype(np.float32)
        Ksrc = _und.K_SRC if (sw, sh) == (67, 45) else (0.9 * sw, 0.91 * sw, 0.5 * sw + 3.25, 0.5 * sh - 2.5)
        lens = L.FisheyeLensModel(*Ksrc, **coeff).as_float32()
        k, w, h = L._dst(lens, dstK, dstSize, img.shape)
        value, valid = L.remap_values(img, lens, dstK, dstSize, mode)
        su, sv, fold = L.source_coords(lens, k, w, h)
        delta, fdelta = L.coord_delta(lens, k, w, h)
        near = (np.minimum(np.abs(su), np.abs(su - (sw - 1))) <= delta) | (np.minimum(np.abs(sv), np.abs(sv - (sh - 1))) <= delta) \
            | (np.abs(fold) <= fdelta)
        ref = dict(value=value, valid=valid, bar=L.remap_bar(img, lens, dstK, dstSize, mode), near=near, size=(w, h))
        _und._cache[key] = (img, lens, dstK, dstSize, mode, ref)
    return key, _und._cache[key]


@pytest.mark.parametrize("cid", sorted(LENS_CASES))
def test_undistort_fisheye_matches_the_float64_statement(cid):
    from gaussiansplattingmlx_amd import lens as L
    key, (img, lens, dstK, dstSize, mode, ref) = _lens_case(cid)
    # the case's own conditions, on the host: lens.py's float32 evaluation is held to the same rules
    out32, valid32 = L.undistort_fisheye_image(img, lens, dstK, dstSize, mode, dtype=np.float32)
    _und._compare(key, out32, valid32, "float32 host")
    if cid == "80x50_c4_fold":
        assert 0.2 < ref["valid"].mean() < 0.8
    r = _renderer()
    out, valid = r.undistortFisheyeImage(img, lens, dstK, dstSize, mode)
    out, valid = _np(out), _np(valid)
    _und._compare(key, out, valid, "kernel")
    # ... and to lens.py's float32 evaluation itself: the same operations in the same order, and lens.hip is compiled without
    # FMA contraction, so the bar is equality -- every validity flag, and every value (invalid pixels are 0 on both sides)
    flags, values = int((valid != valid32).sum()), int((out != out32).sum())
    print(f"{cid}: kernel against lens.py's float32 evaluation: {flags} validity flags and {values} values differ")
    assert out.dtype == out32.dtype and flags == 0 and values == 0, (cid, flags, values)
    out2, none = r.undistortFisheyeImage(img, lens, dstK, dstSize, mode, wantValid=False)
    assert none is None and np.array_equal(_np(out2), out)
    with pytest.raises(ValueError):
        r.undistortFisheyeImage(img, L.LensModel(*lens.K), dstK, dstSize, mode)


def test_undistort_fisheye_argument_errors():
    from gaussiansplattingmlx_amd import _lib
    r = _renderer()
    lib, ctx, INVALID = r.lib, r.ctx, 1
    src, dst = torch.zeros(8 * 8 * 4, device="cuda"), torch.zeros(8 * 8 * 4, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    mk = lambda: _lib.gs_fisheye_lens(10.0, 10.0, 4.0, 4.0, 0.1, 0.0, 0.0, 0.0, 10.0, 10.0, 4.0, 4.0)      # noqa: E731
    call = lambda lens, sw=8, sh=8, dw=8, dh=8, ch=1, mode=0: lib.gs_undistort_fisheye(ctx, C.byref(lens), sw, sh, dw, dh, ch, mode, p(src), p(dst), None)      # noqa: E731
    assert call(mk()) == 0 and call(mk(), ch=4) == 0 and call(mk(), mode=2) == 0
    for kw in (dict(ch=0), dict(ch=5), dict(ch=3, mode=1), dict(ch=2, mode=2), dict(mode=3), dict(mode=-1), dict(sw=0), dict(dh=0), dict(dw=-1)):
        assert call(mk(), **kw) == INVALID, kw
        assert b"gs_undistort_fisheye" in lib.gs_last_error(ctx)
    for field, v in (("fx", 0.0), ("fy", -1.0), ("dst_fx", 0.0), ("dst_fy", float("nan")), ("k4", float("inf"))):
        bad = mk()
        setattr(bad, field, v)
        assert call(bad) == INVALID, field
    assert lib.gs_undistort_fisheye(ctx, None, 8, 8, 8, 8, 1, 0, p(src), p(dst), None) == INVALID
    assert lib.gs_undistort_fisheye(ctx, C.byref(mk()), 8, 8, 8, 8, 1, 0, None, p(dst), None) == INVALID
    torch.cuda.synchronize()
