"""The principal point through the host-side camera (camera.py), on the CPU: bit compatibility of the
centred camera, the pixel convention through the oracle's projection, the loaders' cameras against the back-projection of
pointcloud.getRaysFromImages, and the 3-D filter's SEEN test for an off-centre frustum (filter3d.py).

The convention: a view-space point (x, y, z) lands at means2d = (fx x / z + cx - 0.5, fy y / z + cy - 0.5), in the renderer's
coordinates where pixel i's centre is at i; cx, cy are COLMAP's, where pixel i covers [i, i + 1).  getRaysFromImages
back-projects the image position (i, j) in COLMAP's coordinates, K^-1 (i, j, 1), so the round trip gives back the image
position means2d + 0.5 = (i, j).

Tolerance of the float32 projection: 32 x 2^-24 of the magnitudes involved, |fx x / z| + cx + W (the view transform's three
products and sums, the projection's, the division, the pixel map: below 32 roundings; fx and the matrix entries are float32
numbers, one rounding each of their own)."""
import numpy as np
import pytest

from gaussiansplattingmlx_amd import filter3d as f3
from gaussiansplattingmlx_amd.camera import (Camera, apply_pose_correction, cameras_from_train_data, focal2fov, getProjectionMatrix,
                                             look_at_c2w)
from gaussiansplattingmlx_amd.data import TrainData
from gaussiansplattingmlx_amd.pointcloud import getRaysFromImages

W, H, FX, FY, CX, CY = 64, 48, 70.0, 66.0, 39.25, 18.5
C2W = look_at_c2w([2.2, -2.6, 1.7])


def _legacy_projection(znear, zfar, fovX, fovY):
    """getProjectionMatrix as it was before the principal point, statement for statement."""
    tanHalfY, tanHalfX = np.tan(fovY / 2.0), np.tan(fovX / 2.0)
    top, right = tanHalfY * znear, tanHalfX * znear
    bottom, left = -top, -right
    P = np.zeros((4, 4), np.float64)
    P[0, 0] = 2 * znear / (right - left)
    P[1, 1] = 2 * znear / (top - bottom)
    P[2, 0] = (right + left) / (right - left)
    P[2, 1] = (top + bottom) / (top - bottom)
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = 1.0
    P[3, 2] = -znear * zfar / (zfar - znear)
    return P


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@pytest.mark.parametrize("w,h", [(64, 48), (63, 47), (800, 600)])
def test_centred_camera_is_bit_for_bit_the_reference_camera(w, h):
    fovX, fovY = focal2fov(np.float32(FX), float(w)), focal2fov(np.float32(FY), float(h))
    legacy = _legacy_projection(0.1, 100.0, float(fovX), float(fovY))
    assert _bits(getProjectionMatrix(0.1, 100.0, float(fovX), float(fovY))) == _bits(legacy)
    assert _bits(getProjectionMatrix(0.1, 100.0, float(fovX), float(fovY), 0.0, 0.0)) == _bits(legacy)
    plain, centred = Camera(w, h, FX, FY, C2W), Camera(w, h, FX, FY, C2W, cx=w / 2, cy=h / 2)
    assert _bits(plain.projectionMatrix) == _bits(legacy.astype(np.float32))
    assert _bits(plain.worldViewTransform) == _bits(np.linalg.inv(C2W).T.astype(np.float32))
    assert plain.FoVx == fovX and plain.FoVy == fovY and plain.principalX == w / 2 and plain.principalY == h / 2
    a, b = plain.as_dict(), centred.as_dict()
    assert sorted(a) == sorted(b) and {"principalX", "principalY"} <= set(a)
    for k in a:
        assert _bits(np.asarray(a[k])) == _bits(np.asarray(b[k])), k
    assert not np.signbit(plain.projectionMatrix[2, :2]).any()


def test_offsets_enter_the_third_row_only_with_the_sign_of_clip_w_plus_z():
    cam, ref = Camera(W, H, FX, FY, C2W, cx=CX, cy=CY), Camera(W, H, FX, FY, C2W)
    P, P0 = cam.projectionMatrix.reshape(16), ref.projectionMatrix.reshape(16)
    assert P[8] == np.float32((2 * CX - W) / W) and P[9] == np.float32((2 * CY - H) / H) and P[8] > 0 > P[9]
    rest = [i for i in range(16) if i not in (8, 9)]
    assert _bits(P[rest]) == _bits(P0[rest])
    assert cam.FoVx == ref.FoVx and cam.FoVy == ref.FoVy            # the EWA clamp's limX / limY stay symmetric
    assert _bits(cam.worldViewTransform) == _bits(ref.worldViewTransform)
    assert (cam.principalX, cam.principalY) == (CX, CY)


def test_pose_correction_carries_the_principal_point():
    cam = Camera(W, H, FX, FY, C2W, cx=CX, cy=CY)
    out = apply_pose_correction(cam, [0.01, -0.02, 0.005, 0.1, 0.0, -0.05])
    assert (out.principalX, out.principalY) == (CX, CY) and _bits(out.projectionMatrix) == _bits(cam.projectionMatrix)
    assert not np.array_equal(out.worldViewTransform, cam.worldViewTransform)


def _project(o, cam, xyz):
    c = cam.as_dict()
    n = xyz.shape[0]
    sc, rt = np.full((n, 3), 0.01), np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    shs = np.zeros((n, 1, 3))
    out = o.projection_forward(sc, rt, xyz, shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"], c["focalX"],
                               c["focalY"], cam.imageWidth, cam.imageHeight, 0)
    return np.asarray(out["means2d"], np.float64), np.asarray(out["radii"])


def _tol(expected_minus_c, c, size):
    return 32 * 2.0 ** -24 * (np.abs(expected_minus_c) + c + size)


@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_a_view_space_point_lands_at_fx_x_over_z_plus_cx_minus_half(oracle32, oracle64, precision):
    o = oracle32 if precision == "float32" else oracle64
    cam = Camera(W, H, FX, FY, C2W, cx=CX, cy=CY)
    rng = np.random.default_rng(3)
    # view-space points inside the off-centre frustum, taken to the world through c2w
    z = rng.uniform(1.0, 6.0, 200)
    px, py = rng.uniform(0.0, W, 200), rng.uniform(0.0, H, 200)
    pv = np.stack([(px - CX) / FX * z, (py - CY) / FY * z, z], 1)
    xyz = (pv @ C2W[:3, :3].T + C2W[:3, 3]).astype(np.float32)
    view = cam.worldViewTransform.astype(np.float64)
    p = xyz.astype(np.float64) @ view[:3, :3] + view[3, :3]          # the float32 inputs' own view-space points
    fx, fy = float(cam.focalX), float(cam.focalY)
    m2d, radii = _project(o, cam, xyz)
    assert (radii > 0).all()
    ex, ey = fx * p[:, 0] / p[:, 2], fy * p[:, 1] / p[:, 2]
    errx, erry = np.abs(m2d[:, 0] - (ex + CX - 0.5)), np.abs(m2d[:, 1] - (ey + CY - 0.5))
    print(f"{precision}: max err / tol = {(errx / _tol(ex, CX, W)).max():.3f}, {(erry / _tol(ey, CY, H)).max():.3f}")
    assert np.all(errx <= _tol(ex, CX, W)) and np.all(erry <= _tol(ey, CY, H))
    # the centred camera of the same focal lengths shows what the offset does: the whole view shifted by cx - W / 2
    m0, _ = _project(o, Camera(W, H, FX, FY, C2W), xyz)
    np.testing.assert_allclose(m2d - m0, np.broadcast_to([CX - W / 2, CY - H / 2], m0.shape), atol=2 * _tol(ex, CX, W).max())


def test_loader_cameras_return_the_pixels_the_point_cloud_was_back_projected_from(oracle64):
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.float32)
    c2ws = np.stack([C2W, look_at_c2w([-1.5, 2.0, 0.8])]).astype(np.float32)
    data = TrainData(np.array([H, H], np.float32), np.array([W, W], np.float32), np.stack([K, K]), c2ws,
                     np.zeros((2, H, W, 3), np.float32), np.ones((2, H, W), np.float32))
    stride, depth = 5, 3.25
    rays_o, rays_d = getRaysFromImages(H, W, data.intrinsicArray, data.c2wArray, stride)
    ug, vg = np.meshgrid(np.arange(0, W, stride), np.arange(0, H, stride), indexing="xy")
    pix = np.stack([ug.reshape(-1), vg.reshape(-1)], 1).astype(np.float64)
    offset = cameras_from_train_data(data)
    centred = cameras_from_train_data(data, principal_point=False)
    assert len(offset) == 2 and (offset[0].principalX, offset[0].principalY) == (CX, CY)
    assert centred[0].projectionMatrix[2, 0] == 0 and centred[0].projectionMatrix[2, 1] == 0
    assert (centred[1].principalX, centred[1].principalY) == (W / 2, H / 2)
    tol = 64 * 2.0 ** -24 * (2 * W + depth * FX)          # the float32 rays and matrices, and the projection's own roundings
    for v in range(2):
        pts = (rays_o[v] + rays_d[v] * np.float32(depth)).astype(np.float32)
        got, radii = _project(oracle64, offset[v], pts)
        assert (radii > 0).all()
        np.testing.assert_allclose(got + 0.5, pix, atol=tol)
        miss, _ = _project(oracle64, centred[v], pts)
        np.testing.assert_allclose(pix - (miss + 0.5), np.broadcast_to([CX - W / 2, CY - H / 2], pix.shape), atol=tol)
    np.testing.assert_allclose(offset[1].worldViewTransform, np.linalg.inv(c2ws[1].astype(np.float64)).T, atol=1e-6)


def _direct_width(xyz, cams, centred=False):
    """The filter's rule evaluated directly in float64: |px / pz + ox| <= lim with ox = proj[8] / proj[0]."""
    x = np.asarray(xyz, np.float64)
    best = np.full(x.shape[0], np.inf)
    seen_any = np.zeros(x.shape[0], bool)
    seen_sets = []
    for c in cams:
        view, P = c.worldViewTransform.astype(np.float64), c.projectionMatrix.astype(np.float64).reshape(16)
        p = x @ view[:3, :3] + view[3, :3]
        ox, oy = (0.0, 0.0) if centred else (P[8] / P[0], P[9] / P[5])
        limX, limY = 1.3 * np.tan(float(c.FoVx) / 2), 1.3 * np.tan(float(c.FoVy) / 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            seen = (p[:, 2] >= 0.2) & (np.abs(p[:, 0] / p[:, 2] + ox) <= limX) & (np.abs(p[:, 1] / p[:, 2] + oy) <= limY)
        T = p[:, 2] / float(c.focalX)
        best = np.where(seen & (T < best), T, best)
        seen_any |= seen
        seen_sets.append(seen)
    f = np.zeros(x.shape[0])
    f[seen_any] = np.sqrt(0.2) * best[seen_any]
    f[~seen_any] = f[seen_any].max()
    return f, np.stack(seen_sets)


def off_centre_filter_scene(N=500, seed=21):
    """Three off-centre cameras (principal points up to 0.4 W from the centre) and float32 points of a box that reaches outside
    every frustum, none within 1e-3 relative of a threshold of SEEN."""
    rng = np.random.default_rng(seed)
    cams = [Camera(200, 150, 180.0, 175.0, look_at_c2w([4.0, 0.5, 1.0]), cx=180.0, cy=75.0),
            Camera(200, 150, 220.0, 221.0, look_at_c2w([-3.0, 3.0, 0.5]), cx=100.0, cy=20.0),
            Camera(160, 120, 150.0, 150.0, look_at_c2w([0.5, -4.5, 2.0]), cx=30.5, cy=95.25)]
    cand = rng.uniform(-4.0, 4.0, (2 * N, 3)).astype(np.float32)
    d = np.full(cand.shape[0], np.inf)
    for fold in (True, False):          # (away from the centred cameras' thresholds too: both tables are compared)
        for c in cams:
            _, _, p, lim = f3.camera_terms(cand, c, fold)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.minimum(d, np.minimum(np.abs(p[:, 2] - f3.Z_NEAR) / f3.Z_NEAR,
                                             np.minimum(np.abs(np.abs(p[:, 0] / p[:, 2]) - lim[0]) / lim[0],
                                                        np.abs(np.abs(p[:, 1] / p[:, 2]) - lim[1]) / lim[1])))
    cand = cand[d >= 1e-3]
    assert cand.shape[0] >= N
    return cand[:N], cams


def test_filter_width_of_off_centre_cameras_is_the_direct_rule():
    x, cams = off_centre_filter_scene()
    assert f3.threshold_distance(x, cams) >= 1e-3
    want, sets = _direct_width(x, cams)
    _, sets0 = _direct_width(x, cams, centred=True)
    changed = (sets != sets0).any(axis=0)
    print(f"seen share {sets.any(axis=0).mean():.3f}; points whose seen set differs from the centred cameras': {int(changed.sum())}")
    assert changed.sum() >= 10 and (sets & ~sets0).any() and (~sets & sets0).any()
    got, seen, arg = f3.filter_width(x, cams, details=True)
    np.testing.assert_array_equal(seen, sets.any(axis=0))
    np.testing.assert_allclose(got, want, rtol=1e-14)
    assert (got != f3.filter_width(x, cams, fold=False)).any()
    # a centred camera's terms keep their bits: no fold is applied
    plain = [Camera(c.imageWidth, c.imageHeight, c.focalX, c.focalY, c.c2w) for c in cams]
    np.testing.assert_array_equal(f3.filter_width(x, plain), f3.filter_width(x, cams, fold=False))
    np.testing.assert_array_equal(f3.filter_width(x, [c.as_dict() for c in cams]), got)
