"""The fisheye camera model on the CPU (include/gsplat.h gs_set_camera_model / gs_undistort_fisheye): the numpy
restatement tests/fisheye_numpy.py against float64 central differences, its float32 floor, the fisheye lens map of lens.py, the
loaders' fisheye="equidistant", Camera(model=), and the ABI.

The model's float32 floor, measured by test_float32_floor_over_the_sweep (r / z in {0} and [1e-7, 30], z in {0.2, 0.7, 3, 40}, six
azimuths, the series threshold resolved by 2001 extra points over r / z in [0.15, 0.25]; per point, the largest element's error over
the largest element): J 2.64e-7, the VJP of J 1.53e-5 (its worst points lie just above the threshold, r / z = 0.20 .. 0.25, where
(z h - s) / rho has lost eps / w to cancellation and the random cotangent's terms cancel on top of it; below the threshold 4e-7,
beyond r / z = 1 1e-6).  The bars below are 1.25 x the measured values.
"""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fisheye_numpy as F  # noqa: E402

from gaussiansplattingmlx_amd import data as D  # noqa: E402
from gaussiansplattingmlx_amd import lens as L  # noqa: E402
from gaussiansplattingmlx_amd.camera import Camera, cameras_from_train_data  # noqa: E402

FX, FY = 40.0, 37.0
J_FLOOR, VJP_FLOOR = 2.64e-7, 1.53e-5


def _load(name):
    spec = importlib.util.spec_from_file_location("_fe_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mean(x, y, z):
    s = F.fisheye_map(x, y, z)[0]
    return np.stack([FX * x * s, FY * y * s], -1)


def _points(n=400, seed=0):
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.2, 3, n)
    x[:4], y[:4], z[:4] = [0.0, 1e-3, 0.19, 0.21], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]
    return x, y, z


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_jacobian_and_its_vjp_match_central_differences():
    x, y, z = _points()
    J, _ = F.jacobian(x, y, z, FX, FY)
    eps = 1e-6
    steps = ((eps, 0, 0), (0, eps, 0), (0, 0, eps))
    for a, (dx, dy, dz) in enumerate(steps):
        fd = (_mean(x + dx, y + dy, z + dz) - _mean(x - dx, y - dy, z - dz)) / (2 * eps)
        assert np.abs(fd - J[:, :, a]).max() <= 1e-8 * np.abs(J).max(), a
    rng = np.random.default_rng(1)
    dj = [rng.standard_normal(x.shape) for _ in range(6)]
    v = np.stack(F.jacobian_vjp(x, y, z, FX, FY, dj), -1)

    def under(x, y, z):
        Jq = F.jacobian(x, y, z, FX, FY)[0]
        return sum(dj[3 * r + a] * Jq[:, r, a] for r in range(2) for a in range(3))
    for a, (dx, dy, dz) in enumerate(steps):
        fd = (under(x + dx, y + dy, z + dz) - under(x - dx, y - dy, z - dz)) / (2 * eps)
        assert np.abs(fd - v[:, a]).max() <= 1e-8 * np.abs(v).max(), a


def test_full_vjp_matches_central_differences_of_the_projection():
    """means2d, depth, cov2d and conic under random cotangents, with respect to means, scales and rotations."""
    p, pv = F.scene()
    W, H = F.SCENE_W, F.SCENE_H
    c = Camera(W, H, *F.SCENE_FOCAL, F.scene_c2w(), cx=F.SCENE_PRINCIPAL[0], cy=F.SCENE_PRINCIPAL[1], model="fisheye").as_dict()
    s, q = F.activated(p, np.float64)
    m = p["xyz"].astype(np.float64)
    rng = np.random.default_rng(9)
    n = m.shape[0]
    cm, cd, cc, cn = rng.standard_normal((n, 2)), rng.standard_normal(n), rng.standard_normal((n, 2, 2)), rng.standard_normal((n, 2, 2))

    def loss(s, q, m):
        o = F.project(s, q, m, c, W, H)
        return (o["means2d"] * cm).sum(1) + o["depths"] * cd + (o["cov2d"] * cc).sum((1, 2)) + (o["conic"] * cn).sum((1, 2))
    g = F.project_vjp(s, q, m, c, W, H, cm, cd, cc, cn)
    front = pv[:, 2] >= 0.2
    eps = 1e-6
    for key, name in (("gradMeans3d", "m"), ("gradScales", "s"), ("gradRot", "q")):
        base = dict(s=s, q=q, m=m)
        for j in range(base[name].shape[1]):
            d = np.zeros_like(base[name]); d[:, j] = eps
            up, dn = dict(base), dict(base)
            up[name], dn[name] = base[name] + d, base[name] - d
            fd = (loss(**up) - loss(**dn)) / (2 * eps)
            err = np.abs(fd - g[key][:, j])[front] / np.abs(g[key][front]).max(axis=1)
            assert err.max() <= 1e-6, (key, j, err.max())


def test_on_the_axis_is_the_pinhole_and_finite():
    for dt in (np.float32, np.float64):
        for z in (0.2, 1.0, 37.5):
            J, (s, g, h, grho) = F.jacobian(np.zeros(1), np.zeros(1), np.full(1, z), FX, FY, dt)
            want = np.array([[dt(FX) / dt(z), 0, 0], [0, dt(FY) / dt(z), 0]], dt)
            assert np.array_equal(J[0], want) and np.isfinite([s, g, h, grho]).all(), (dt, z)
            assert abs(float(g[0]) * z ** 3 + 2.0 / 3.0) < 1e-6 and abs(float(grho[0]) * z ** 5 - 0.8) < 1e-6
            v = F.jacobian_vjp(np.zeros(1), np.zeros(1), np.full(1, z), FX, FY, [np.ones(1, dt)] * 6, None, dt)
            assert np.isfinite(v).all()


def test_a_point_on_the_x_axis_lands_at_focal_times_its_angle():
    W, H = 64, 48
    cam = Camera(W, H, FX, FY, F.scene_c2w(), cx=30.5, cy=25.25, model="fisheye")
    x = np.array([0.0, 1e-4, 0.05, 0.19, 0.21, 0.9, 1.0, 1.1, 5.0, 30.0])
    z = 1.3
    pv = np.stack([x * z, np.zeros_like(x), np.full_like(x, z)], -1)
    xyz = pv @ F.scene_c2w()[:3, :3].T
    ones = np.ones((len(x), 3))
    quat = np.tile([1.0, 0, 0, 0], (len(x), 1))
    # (cx - 0.5, cy - 0.5) as the float32 projection matrix holds them: 30 exactly, 24.75 to 3e-8)
    ox, oy = F.principal_offset(cam.projectionMatrix, W, H, np.float64)
    assert ox == 30.0 and abs(oy - 24.75) < 1e-6
    want = FX * np.arctan(x) + ox
    for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        o = F.project(ones * 0.01, quat, xyz, cam.as_dict(), W, H, dt)
        assert np.abs(o["means2d"][:, 0] - want).max() <= tol * (1 + np.abs(want).max()), dt
        assert np.abs(o["means2d"][:, 1] - oy).max() <= tol * 25


def test_float32_floor_over_the_sweep():
    rng = np.random.default_rng(0)
    ratios = np.concatenate([[0.0], np.logspace(-7, np.log10(30), 4000), np.linspace(0.15, 0.25, 2001)])
    worstJ = worstV = 0.0
    for z in (0.2, 0.7, 3.0, 40.0):
        for phi in (0.0, 0.3, 1.1, 2.5, 4.0, 5.5):
            r = ratios * z
            x, y, zz = (v.astype(np.float32) for v in (r * np.cos(phi), r * np.sin(phi), np.full_like(r, z)))
            x64, y64, z64 = (v.astype(np.float64) for v in (x, y, zz))
            J64 = F.jacobian(x64, y64, z64, FX, FY)[0]
            J32 = F.jacobian(x, y, zz, FX, FY, np.float32)[0]
            assert np.isfinite(J32).all()
            worstJ = max(worstJ, float((np.abs(J32 - J64).max(axis=(1, 2)) / np.abs(J64).max(axis=(1, 2))).max()))
            dj = [rng.standard_normal(x.shape) for _ in range(6)]
            v64 = np.stack(F.jacobian_vjp(x64, y64, z64, FX, FY, dj), -1)
            v32 = np.stack(F.jacobian_vjp(x, y, zz, FX, FY, [d.astype(np.float32) for d in dj], None, np.float32), -1)
            assert np.isfinite(v32).all()
            worstV = max(worstV, float((np.abs(v32 - v64).max(axis=1) / np.abs(v64).max(axis=1)).max()))
    print(f"float32 floor over the sweep: J {worstJ:.3e} (recorded {J_FLOOR:.2e}), VJP {worstV:.3e} (recorded {VJP_FLOOR:.2e})")
    assert worstJ <= 1.25 * J_FLOOR and worstV <= 1.25 * VJP_FLOOR
    # the textbook form is what the series is there for: a - b of x^2 a + y^2 b cancels away near the axis
    x, z = np.float32(1e-4), np.float32(1.0)
    r = np.sqrt(x * x)
    th = np.arctan2(r, z)
    a = z / (r * r + z * z) / (r * r)
    b = th / (r * r * r)
    assert abs(float(np.float32(a - b)) + 2.0 / 3.0) > 0.5 and abs(float(F.fisheye_map(x, np.float32(0), z, np.float32)[1]) + 2.0 / 3.0) < 1e-6


def test_the_gpu_scene_is_what_its_tests_assume():
    p, pv = F.scene()
    W, H = F.SCENE_W, F.SCENE_H
    cam = Camera(W, H, *F.SCENE_FOCAL, F.scene_c2w(), cx=F.SCENE_PRINCIPAL[0], cy=F.SCENE_PRINCIPAL[1], model="fisheye")
    assert set(np.unique(np.abs(cam.worldViewTransform))) <= {0.0, 1.0}
    c = cam.as_dict()
    s, q = F.activated(p, np.float32)
    a = F.project(s, q, p["xyz"], c, W, H, np.float32)
    b = F.project(s.astype(np.float64), q.astype(np.float64), p["xyz"].astype(np.float64), c, W, H)
    assert np.array_equal(np.stack(a["_pv"], -1), pv)                    # view space is the world's bits
    ties = int((np.ceil(np.sqrt(a["lambdaMax"])) != np.ceil(np.sqrt(b["lambdaMax"]))).sum())
    assert ties <= F.SCENE_N // 100, ties
    hand = F.HAND_ROWS
    w = (pv[:, 0].astype(np.float32) ** 2 + pv[:, 1].astype(np.float32) ** 2) / pv[:, 2].astype(np.float32) ** 2
    assert w[hand["on_axis"]] == 0 and w[hand["below_series"]] < np.float32(F.SERIES_W) < w[hand["above_series"]]
    assert abs(w[hand["below_series"]] - F.SERIES_W) < 1e-4 and abs(w[hand["above_series"]] - F.SERIES_W) < 1e-4
    assert pv[hand["z_below_near"], 2] < np.float32(0.2) == pv[hand["z_at_near"], 2] and pv[hand["behind"], 2] < 0
    assert a["radii"][hand["z_below_near"]] == 0 and a["radii"][hand["z_at_near"]] > 0 and a["radii"][hand["behind"]] == 0
    assert w[hand["steep"]] > 25 and a["radii"][hand["steep"]] > 0
    theta = np.degrees(np.arctan2(np.hypot(pv[:, 0], pv[:, 1]), pv[:, 2]))[b["radii"] > 0]
    assert theta.min() == 0 and 78 < theta.max() < 81


# ------------------------------------------------------------------------------------------------------------------ the lens
def test_fisheye_lens_without_coefficients_copies_the_image():
    rng = np.random.default_rng(0)
    img = rng.uniform(0, 1, (45, 67, 3)).astype(np.float32)
    lens = L.FisheyeLensModel(60.0, 58.0, 35.25, 21.5)
    assert lens.is_equidistant and lens.first_fold() == float("inf")
    out, valid = L.undistort_fisheye_image(img, lens)
    assert np.array_equal(out[:-1, :-1], img[:-1, :-1]) and (valid[:-1, :-1] == 255).all()
    assert not valid[-1].any() and not valid[:, -1].any()              # (the last row and column have no second tap)
    # in float32 ((i + 0.5 - cx) / fx) fx + cx - 0.5 may land an ulp below i: the tap pair moves, the blend does not
    out32, valid32 = L.undistort_fisheye_image(img, lens, dtype=np.float32)
    both = (valid == 255) & (valid32 == 255)
    assert (valid != valid32).sum() <= 0.01 * valid.size + img.shape[0] + img.shape[1]
    assert np.abs(out32 - img)[both].max() <= float(L.remap_bar(img, lens)[both].max())
    with pytest.raises(ValueError):
        L.undistort_fisheye_image(img, L.LensModel(60.0, 58.0, 35.25, 21.5))


def test_fisheye_lens_map_is_theta_d():
    lens = L.FisheyeLensModel(60.0, 58.0, 35.25, 21.5, 0.05, -0.01, 0.002, -0.0005)
    theta = np.linspace(0.0, 1.4, 50)
    xd, yd = lens.distort(theta * np.cos(0.7), theta * np.sin(0.7))
    want = F.lens_theta_d(theta, lens.coefficients)
    assert np.abs(np.hypot(xd, yd) - want).max() < 1e-14


def test_fisheye_lens_validity_guard():
    """k1 = -0.35: d theta_d / d theta = 1 - 1.05 theta^2 has its root at theta^2 = 0.952; k = (-0.5, 0.1): roots at theta^2 = 1
    and 2, positive again beyond 2 -- those pixels stay invalid."""
    rng = np.random.default_rng(2)
    img = rng.uniform(0, 1, (90, 120, 1)).astype(np.float32)
    dstK, size = (40.0, 40.0, 60.0, 45.0), (120, 90)
    i, j = np.meshgrid(np.arange(120) + 0.5, np.arange(90) + 0.5)
    t2 = ((i - 60.0) / 40.0) ** 2 + ((j - 45.0) / 40.0) ** 2
    for k, root in (((-0.35, 0.0, 0.0, 0.0), 1.0 / 1.05), ((-0.5, 0.1, 0.0, 0.0), 1.0)):
        lens = L.FisheyeLensModel(40.0, 40.0, 60.0, 45.0, *k)
        assert abs(lens.first_fold() - root) < 1e-9
        for dt in (np.float64, np.float32):
            out, valid = L.undistort_fisheye_image(img, lens, dstK, size, dtype=dt)
            inside = t2 < root - 1e-3
            assert not valid[t2 > root + 1e-3].any() and (t2 > 2.1).any(), (k, dt)
            assert (valid[inside] == 255).mean() > 0.99 and not out[valid == 0].any()


@pytest.mark.parametrize("mode", ["color", "mask", "depth"])
def test_fisheye_float32_remap_stays_inside_its_bar(mode):
    """lens.remap_bar, counted as for the radial-tangential lens with the fisheye polynomial's 38 roundings."""
    rng = np.random.default_rng(5)
    shape = (45, 67, 3) if mode == "color" else (45, 67)
    if mode == "mask":
        img = rng.integers(0, 256, shape, dtype=np.uint8)
    elif mode == "depth":
        img = rng.uniform(0.5, 5.0, shape).astype(np.float32)
        img[rng.uniform(size=shape) < 0.2] = 0.0
    else:
        img = rng.uniform(0, 1, shape).astype(np.float32)
    lens = L.FisheyeLensModel(60.0, 58.0, 35.25, 21.5, 0.11, -0.03, 0.004, -0.001).as_float32()
    v64, ok64 = L.remap_values(img, lens, mode=mode)
    v32, ok32 = L.remap_values(img, lens, mode=mode, dtype=np.float32)
    bar = L.remap_bar(img, lens, mode=mode)
    both = ok64 & ok32
    assert 0.5 < ok64.mean() < 1.0 and (ok64 != ok32).sum() <= 0.01 * ok64.size
    err = np.abs(v32.astype(np.float64) - v64)
    assert np.all(err[both] <= bar[both]) and not bar[~ok64].any()


# --------------------------------------------------------------------------------------------------------------- the loaders
FISHEYE_CAM = (88.0, 86.0, 50.5, 30.25, 0.1, -0.02, 0.003, -0.0004)


def _fisheye_set(tmp_path):
    lc = _load("test_lens_cpu")
    kw = lc.two_view_set(tmp_path)
    cams = [(1, 1, lc.SRC_W, lc.SRC_H, (90.0, 91.0, 47.0, 33.0)), (2, 5, lc.SRC_W, lc.SRC_H, FISHEYE_CAM)]
    lc._write_colmap(tmp_path / "sparse", cams, [(10, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 3.0), 1, "a.png"),
                                                 (11, (1.0, 0.0, 0.0, 0.0), (0.5, 0.0, 3.0), 2, "b.png")])
    return kw


def test_colmap_loader_resamples_fisheye_views_into_the_equidistant_camera(tmp_path):
    kw = _fisheye_set(tmp_path)
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):                     # today's behaviour, kept
        D.ColmapDataLoader(**kw, undistort=True).load()
    plain, _, _ = D.ColmapDataLoader(**kw).load()
    assert plain.cameraModelArray is None
    td, _, _ = D.ColmapDataLoader(**kw, undistort=True, fisheye="equidistant").load()
    assert td.cameraModelArray.tolist() == ["pinhole", "fisheye"]
    np.testing.assert_array_equal(td.rgbArray[0], plain.rgbArray[0])
    np.testing.assert_array_equal(td.intrinsicArray, plain.intrinsicArray)
    lens = L.FisheyeLensModel(*FISHEYE_CAM)
    rgba = np.concatenate([plain.rgbArray[1], plain.alphaArray[1][..., None]], -1)
    want, valid = L.undistort_fisheye_image(rgba, lens)
    np.testing.assert_array_equal(td.rgbArray[1], want[..., :3])
    np.testing.assert_array_equal(td.maskArray[1], valid)
    assert (td.maskArray[0] == 255).all() and 0.5 < (valid == 255).mean() < 1.0
    cams = cameras_from_train_data(td)
    assert [c.model for c in cams] == ["pinhole", "fisheye"] and "model" not in cams[0].as_dict() and cams[1].as_dict()["model"] == "fisheye"
    assert (cams[1].principalX, cams[1].principalY) == (50.5, 30.25)
    for bad in (dict(fisheye="equidistant"), dict(fisheye="equidistant", undistort=True, cameraModels="reference"),
                dict(fisheye="stereographic", undistort=True)):
        with pytest.raises(ValueError):
            D.ColmapDataLoader(**dict(kw, **bad))
    # the models that stay out of scope still raise
    lc = _load("test_lens_cpu")
    for model, n in ((10, 12), (7, 5), (6, 12)):
        lc._write_colmap(tmp_path / "sparse", [(1, 1, lc.SRC_W, lc.SRC_H, (90.0, 91.0, 47.0, 33.0)),
                                               (2, model, lc.SRC_W, lc.SRC_H, (88.0, 86.0, 50.5, 30.25) + (0.01,) * (n - 4))],
                         [(10, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 3.0), 1, "a.png"), (11, (1.0, 0.0, 0.0, 0.0), (0.5, 0.0, 3.0), 2, "b.png")])
        with pytest.raises(ValueError, match=D.COLMAP_MODELS[model][0]):
            D.ColmapDataLoader(**kw, undistort=True, fisheye="equidistant").load()


def test_colmap_loader_without_fisheye_is_unchanged(tmp_path):
    lc = _load("test_lens_cpu")
    kw = lc.two_view_set(tmp_path)
    a, _, _ = D.ColmapDataLoader(**kw, undistort=True).load()
    b, _, _ = D.ColmapDataLoader(**kw, undistort=True, fisheye="equidistant").load()       # (no fisheye camera in the set)
    assert a.cameraModelArray is None and b.cameraModelArray is None
    for k in ("rgbArray", "alphaArray", "maskArray", "intrinsicArray", "c2wArray"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))


def test_nerfstudio_loader_resamples_fisheye_frames(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    w, h = 48, 32
    for name in ("f0", "f1"):
        Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA").save(tmp_path / f"{name}.png")
    (tmp_path / "pts.ply").write_text("ply\nformat ascii 1.0\nelement vertex 1\nend_header\n0.0 0.0 0.0 1 2 3\n")
    eye = np.eye(4).tolist()
    frames = [dict(file_path="f0.png", transform_matrix=eye), dict(file_path="f1.png", transform_matrix=eye, camera_model="PINHOLE", k1=0.0, k2=0.0, p1=0.0, p2=0.0)]
    meta = dict(fl_x=44.0, fl_y=43.0, cx=25.5, cy=15.0, k1=-0.1, k2=0.02, k3=0.001, k4=0.0, camera_model="OPENCV_FISHEYE",
                ply_file_path="pts.ply", frames=frames)
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    plain, _, _ = D.NerfStudioDataLoader(str(tmp_path)).load()
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        D.NerfStudioDataLoader(str(tmp_path), undistort=True).load()
    with pytest.raises(ValueError):
        D.NerfStudioDataLoader(str(tmp_path), fisheye="equidistant")
    td, _, _ = D.NerfStudioDataLoader(str(tmp_path), undistort=True, fisheye="equidistant").load()
    assert td.cameraModelArray.tolist() == ["fisheye", "pinhole"]
    rgba = np.concatenate([plain.rgbArray[0], plain.alphaArray[0][..., None]], -1)
    want, valid = L.undistort_fisheye_image(rgba, L.FisheyeLensModel(44.0, 43.0, 25.5, 15.0, -0.1, 0.02, 0.001, 0.0))
    np.testing.assert_array_equal(td.rgbArray[0], want[..., :3])
    np.testing.assert_array_equal(td.maskArray[0], valid)
    np.testing.assert_array_equal(td.rgbArray[1], plain.rgbArray[1])


def test_split_train_data_carries_the_camera_models():
    from gaussiansplattingmlx_amd.evaluation import split_train_data
    n = 10
    td = D.TrainData(Hs=np.full(n, 4), Ws=np.full(n, 5), intrinsicArray=np.zeros((n, 3, 3)), c2wArray=np.zeros((n, 4, 4)),
                     rgbArray=np.zeros((n, 4, 5, 3)), alphaArray=np.zeros((n, 4, 5)))
    assert td.cameraModelArray is None and split_train_data(td, 8)[0].cameraModelArray is None
    td.cameraModelArray = np.array(["fisheye" if i % 3 == 0 else "pinhole" for i in range(n)])
    train, test = split_train_data(td, 8)
    assert test.cameraModelArray.tolist() == ["fisheye", "pinhole"] and len(train.cameraModelArray) == 8
    assert train.cameraModelArray.tolist() == [td.cameraModelArray[i] for i in (1, 2, 3, 4, 5, 6, 7, 9)]


def test_copies_of_train_data_keep_the_camera_models():
    import copy
    n = 3
    td = D.TrainData(Hs=np.full(n, 4), Ws=np.full(n, 5), intrinsicArray=np.tile(np.eye(3), (n, 1, 1)), c2wArray=np.tile(np.eye(4), (n, 1, 1)),
                     rgbArray=np.zeros((n, 4, 5, 3)), alphaArray=np.zeros((n, 4, 5)))
    td.cameraModelArray = np.array(["pinhole", "fisheye", "fisheye"])
    for made in (copy.copy(td), copy.deepcopy(td), td.replace(), td.replace(maskArray=np.zeros((n, 4, 5), np.uint8))):
        assert made is not td and made.cameraModelArray.tolist() == ["pinhole", "fisheye", "fisheye"]
        assert [c.model for c in cameras_from_train_data(made)] == ["pinhole", "fisheye", "fisheye"]
    assert td.replace(cameraModelArray=None).cameraModelArray is None and td.cameraModelArray is not None
    assert D.TrainData.cameraModelArray is None                                   # (a fresh TrainData: all pinhole)


# ---------------------------------------------------------------------------------------------------------------- the camera
def test_camera_model_field():
    pin = Camera(64, 48, 40.0, 41.0, np.eye(4), cx=30.0, cy=20.0)
    same = Camera(64, 48, 40.0, 41.0, np.eye(4), cx=30.0, cy=20.0, model="pinhole")
    fish = Camera(64, 48, 40.0, 41.0, np.eye(4), cx=30.0, cy=20.0, model="fisheye")
    assert pin.model == "pinhole" and set(pin.as_dict()) == set(same.as_dict()) and "model" not in pin.as_dict()
    for k, v in pin.as_dict().items():
        np.testing.assert_array_equal(v, same.as_dict()[k])
        np.testing.assert_array_equal(v, fish.as_dict()[k])
    assert fish.as_dict()["model"] == "fisheye"
    with pytest.raises(ValueError):
        Camera(64, 48, 40.0, 41.0, np.eye(4), model="orthographic")


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_and_binding_carry_the_entry_points():
    from gaussiansplattingmlx_amd import _lib
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("gs_set_camera_model", 2), ("gs_get_camera_model", 2), ("gs_undistort_fisheye", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]) and _lib._SIGS[name][0] is C.c_int, name
    assert re.search(r"#define\s+GS_CAMERA_PINHOLE\s+0\b", src) and re.search(r"#define\s+GS_CAMERA_FISHEYE\s+1\b", src)
    m = re.search(r"typedef struct gs_fisheye_lens\s*\{(.*?)\}", code, flags=re.S)
    declared = [n.strip() for names in re.findall(r"\bfloat\s+([a-z0-9_, ]+);", m.group(1)) for n in names.split(",")]
    assert declared == ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "dst_fx", "dst_fy", "dst_cx", "dst_cy"]
    assert [n for n, _ in _lib.gs_fisheye_lens._fields_] == declared and C.sizeof(_lib.gs_fisheye_lens) == 48
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+6\b", src)
    cam = re.search(r"typedef struct gs_camera\s*\{(.*?)\}\s*gs_camera", code, flags=re.S)
    assert cam and "model" not in cam.group(1)                                    # gs_camera keeps its layout


def test_library_exports_and_host_only_checks():
    from gaussiansplattingmlx_amd import build
    build.build()
    from gaussiansplattingmlx_amd import _lib
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    for model in (0, 1, 2, -1):
        assert lib.gs_set_camera_model(None, model) == invalid                    # (no context: rejected before anything else)
    got = C.c_int(7)
    assert lib.gs_get_camera_model(None, C.byref(got)) == invalid and got.value == 7
    lens = _lib.gs_fisheye_lens(10.0, 10.0, 4.0, 4.0, 0.1, 0.0, 0.0, 0.0, 10.0, 10.0, 4.0, 4.0)
    assert lib.gs_undistort_fisheye(None, C.byref(lens), 8, 8, 8, 8, 1, 0, None, None, None) == invalid
    so = open(_lib.LIB_PATH, "rb").read()
    assert b"FisheyeLensArgs" in so and so.count(b"proj_fwd_fused_kernel") > 0
