"""Camera pose refinement without a device: the float64 composition (camera.apply_pose_correction) against an independent
numpy restatement, the trainer's refusals, and the header's declaration (include/gsplat.h gs_set_pose_correction)."""
import os

import numpy as np
import pytest

from gaussiansplattingmlx_amd.camera import Camera, apply_pose_correction, look_at_c2w, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rot_closed(w):
    """Rodrigues in its closed form through the unit axis (the restatement: no series)."""
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    k = w / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _cam():
    return Camera(96, 80, 90.0, 88.0, look_at_c2w([3.0, -2.5, 2.0]))


def test_zero_delta_is_the_camera():
    cam = _cam()
    out = apply_pose_correction(cam, np.zeros(6))
    assert np.array_equal(rodrigues(np.zeros(3)), np.eye(3))
    assert np.array_equal(out.worldViewTransform, cam.worldViewTransform)
    assert np.array_equal(out.projectionMatrix, cam.projectionMatrix)
    assert np.array_equal(out.cameraCenter, cam.cameraCenter)
    assert (out.FoVx, out.FoVy, out.focalX, out.focalY) == (cam.FoVx, cam.FoVy, cam.focalX, cam.focalY)


@pytest.mark.parametrize("t", [1e-6, 1e-4, 0.02, 0.0316, 0.04, 0.5, 2.0])
def test_series_against_closed_form(t):
    # the series is used below |w| = sqrt(1e-3) ~ 0.0316; its first omitted terms are ~t^6 / 5040 there: 1e-12 is the bar
    w = t * np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
    assert np.abs(rodrigues(w) - _rot_closed(w)).max() <= 1e-12


def test_composition_restated():
    cam = _cam()
    d = np.array([0.02, -0.015, 0.03, 0.05, -0.04, 0.08])
    out = apply_pose_correction(cam, d)
    c2w = look_at_c2w([3.0, -2.5, 2.0])
    T = np.eye(4); T[:3, :3] = _rot_closed(d[:3]); T[:3, 3] = d[3:]
    want = c2w @ T
    # view' = inv(c2w')^T (float32), cam' = c2w'[:3, 3]; the translation acts along the camera's own axes
    assert np.abs(out.worldViewTransform - np.linalg.inv(want).T.astype(np.float32)).max() <= 1e-6
    assert np.abs(out.cameraCenter - (c2w[:3, 3] + c2w[:3, :3] @ d[3:])).max() <= 1e-12
    # cam_center' from the view matrix alone
    assert np.abs(np.linalg.inv(out.worldViewTransform.astype(np.float64).T)[:3, 3] - out.cameraCenter).max() <= 1e-5


def test_round_trip():
    cam = _cam()
    d = np.array([0.1, 0.2, -0.3, 0.5, 0.1, -0.2])
    T = np.eye(4); T[:3, :3] = _rot_closed(d[:3]); T[:3, 3] = d[3:]
    Ti = np.linalg.inv(T)
    # the inverse correction as a twist: w' = -w (R(-w) = R(w)^T), tau' = -R^T tau
    back = apply_pose_correction(apply_pose_correction(cam, d), np.concatenate([-d[:3], Ti[:3, 3]]))
    assert np.abs(back.c2w - cam.c2w).max() <= 1e-12
    assert np.abs(back.worldViewTransform - cam.worldViewTransform).max() <= 1e-6


@pytest.mark.parametrize("kw", [dict(views_per_rank=2), dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)),
                                dict(exchange_impl="native"), dict(n_views=None), dict(n_views=0)])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(pose_opt=True, n_views=4)
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_header_declares_entry():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "int gs_set_pose_correction(gs_ctx* ctx, const float* delta" in src
    from gaussiansplattingmlx_amd import _lib
    assert "gs_set_pose_correction" in _lib.exported_symbols()
