"""The anti-aliased mode without a device (include/gsplat.h gs_set_antialiasing): the float64 opacity
compensation rho = sqrt(det Sigma / det Sigma_b) and its VJP against central differences, the composed oracle this file
defines for the GPU tests (the reference's ops with sigma(o) rho packed) against central differences of its own loss, and
the entry point's declaration, export and null-context refusal.

Bars.  rho's VJP: central differences in float64 at a step of 1e-6 of the entry's scale (1e-9 for the needle, whose
det Sigma is 4e-4 of its entries' product): truncation is O(h^2) of rho's third derivative, well below the 1e-6 relative bar.
The composed oracle: 2 % of the largest component -- the oracle's 3-sigma tile cull and integer radii make its loss piecewise
smooth (the pose test's 5 % at h = 1e-4 with the same cause; here the steps are in raw parameters, see _FD_H).
"""
import ctypes as C
import os

import numpy as np
import pytest

from gaussiansplattingmlx_amd.antialias import BLUR, opacity_scale, opacity_scale_vjp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")


# ------------------------------------------------------------------------------------- the composed oracle (float64 rho)
class AAOracle:
    """Oracle.render_forward / render_backward of the anti-aliased mode, composed from the reference's ops: projection_forward
    -> rho in float64 -> pack_gaussians with sigma(o) rho (radius 0 where rho = 0) -> tile_bin -> blend_forward; blend_backward
    -> dL/d sigma = c rho, cotCov2d = VJP of rho at c sigma -> projection_backward(cotCov2d=...) -> activations_backward.
    Everything else is the wrapped Oracle's."""

    def __init__(self, o):
        self.o, self.dtype = o, o.dtype

    def __getattr__(self, k):
        return getattr(self.o, k)

    def render_forward(self, params, cam, W, H, tileW, tileH, degree, whiteBg=False):
        o = self.o
        op, sc, rt = o.activations_forward(params["opacity"], params["scales"], params["rotation"])
        shs = np.concatenate([o._r(params["features_dc"]), o._r(params["features_rest"])], axis=1)
        pr = o.projection_forward(sc, rt, params["xyz"], shs, cam["camCenter"], cam["view"], cam["proj"], cam["fovX"],
                                  cam["fovY"], cam["focalX"], cam["focalY"], W, H, degree)
        rho = opacity_scale(pr["cov2d"])
        radii = np.where(rho > 0, pr["radii"], 0).astype(self.dtype)
        packed = o.pack_gaussians(pr["means2d"], pr["conic"], pr["color"], (op.astype(np.float64) * rho).astype(self.dtype),
                                  pr["depths"])
        bn = o.tile_bin(pr["rectMin"], pr["rectMax"], radii, pr["depths"], W, H, tileW, tileH)
        color, depth, alpha, last = o.blend_forward(packed, bn.sortedIdx, bn.tileRanges, W, H, tileW, tileH, whiteBg)
        return dict(opacity=op, scales=sc, rot=rt, shs=shs, proj=pr, rho=rho, radii=radii, packed=packed, bin=bn, color=color,
                    depth=depth, alpha=alpha, last=last)

    def render_backward(self, params, cam, W, H, tileW, tileH, degree, fwd, cotColor, cotDepth, cotAlpha, whiteBg=False):
        o, bn = self.o, fwd["bin"]
        gp = o.blend_backward(fwd["packed"], bn.sortedIdx, bn.tileRanges, W, H, tileW, tileH, whiteBg, cotColor, cotDepth,
                              cotAlpha, fwd["color"], fwd["depth"], fwd["alpha"], fwd["last"])
        N = gp.shape[0]
        c = gp[:, 9].astype(np.float64)
        cotCov = opacity_scale_vjp(fwd["proj"]["cov2d"], c * fwd["opacity"].astype(np.float64)).reshape(N, 4)
        pb = o.projection_backward(fwd["scales"], fwd["rot"], params["xyz"], fwd["shs"], cam["camCenter"], cam["view"],
                                   cam["proj"], cam["fovX"], cam["fovY"], cam["focalX"], cam["focalY"], W, H, degree,
                                   gp[:, 10], gp[:, 0:2], cotCov.astype(self.dtype), gp[:, 6:9], gp[:, 2:6])
        do, ds, dq = o.activations_backward(params["opacity"], params["scales"], params["rotation"],
                                            (c * fwd["rho"]).astype(self.dtype), pb["gradScales"], pb["gradRot"])
        return dict(xyz=pb["gradMeans3d"], features_dc=pb["gradShs"][:, :1, :].copy(),
                    features_rest=pb["gradShs"][:, 1:, :].copy(), scales=ds, rotation=dq,
                    opacity=do.reshape(np.shape(params["opacity"])), gradPacked=gp)


def aa_loss(o, p, cam, W, H, target, tile=(16, 16), lam=0.2):
    fw = o.render_forward(p, cam, W, H, tile[0], tile[1], 4)
    loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), target, lam)
    return float(loss), fw, cot


# ------------------------------------------------------------------------------------------------------- rho and its VJP
def _cov(sx, sy, theta):
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    return R @ np.diag([sx * sx, sy * sy]) @ R.T + BLUR * np.eye(2)


CASES = {
    "sub_pixel": (_cov(0.3, 0.2, 0.4), 1e-6),
    "needle": (np.array([[100.0, 9.99], [9.99, 1.0]]) + BLUR * np.eye(2), 1e-9),     # det Sigma = 0.1999
    "large": (_cov(80.0, 45.0, -1.1), 1e-2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_rho_vjp_against_central_differences(case):
    cb, h = CASES[case]
    cb = cb.copy()
    cb[0, 1] += 0.013 * np.sqrt(cb[0, 0] * cb[1, 1]) if case != "needle" else 0.0       # four independent entries: asymmetric
    rho = float(opacity_scale(cb[None])[0])
    assert 0 < rho < 1
    if case == "large":
        assert rho > 0.9999
    if case == "sub_pixel":
        assert rho < 0.4
    got = opacity_scale_vjp(cb[None], 1.0)[0]
    fd = np.zeros((2, 2))
    for i in range(2):
        for j in range(2):
            e = np.zeros((2, 2)); e[i, j] = h
            fd[i, j] = (opacity_scale((cb + e)[None])[0] - opacity_scale((cb - e)[None])[0]) / (2 * h)
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max() + 1e-15, (got, fd)
    # the closed form: (rho / 2) (Sigma^-T - Sigma_b^-T)
    u = cb - BLUR * np.eye(2)
    assert np.allclose(got, 0.5 * rho * (np.linalg.inv(u).T - np.linalg.inv(cb).T), rtol=1e-12, atol=0)


def test_rho_degenerate_is_zero():
    cb = np.array([[[4.0 + BLUR, 2.0], [2.0, 1.0 + BLUR]],        # det Sigma = 0
                   [[1.0 + BLUR, 3.0], [3.0, 1.0 + BLUR]],        # det Sigma < 0
                   [[np.inf, 0.0], [0.0, 1.0]],
                   [[np.nan, 0.0], [0.0, 1.0]]])
    assert np.array_equal(opacity_scale(cb), np.zeros(4))
    g = opacity_scale_vjp(cb, 1.0)
    assert np.array_equal(g, np.zeros_like(g))


def test_rho_energy():
    """rho sigma(o) 2 pi sqrt(det Sigma_b) = sigma(o) 2 pi sqrt(det Sigma): the blurred splat carries the unblurred one's mass."""
    cb = _cov(0.3, 0.3, 0.0)
    rho = float(opacity_scale(cb[None])[0])
    assert abs(rho * np.sqrt(np.linalg.det(cb)) - np.sqrt(np.linalg.det(cb - BLUR * np.eye(2)))) <= 1e-15


# ------------------------------------------------------------------------------------------------ the composed oracle
_FD_H = 1e-4


def _fd_scene():
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    W = H = 64
    p = make_gaussians(60, "trained_like", 3)
    p["scales"] = (p["scales"] + 0.4).astype(np.float32)
    cam = Camera(W, H, 60.0, 60.0, look_at_c2w([3.0, -2.5, 2.0]))
    return p, cam, W, H


def test_composed_oracle_chain_rule_against_central_differences(oracle64):
    """The hand-written chain rule of AAOracle.render_backward against float64 central differences of its own loss, on raw
    scale, rotation, opacity and xyz elements of visible splats with rho well below 1 (where the compensation matters)."""
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    o = AAOracle(oracle64)
    p, cam, W, H = _fd_scene()
    c = cam.as_dict()
    tgt = oracle64.render_forward(make_gaussians(60, "trained_like", 4), c, W, H, 16, 16, 4)["color"].reshape(H, W, 3)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    _, fw, cot = aa_loss(o, p64, c, W, H, tgt)
    z = np.zeros(W * H)
    g = o.render_backward(p64, c, W, H, 16, 16, 4, fw, cot.reshape(-1, 3), z, z)
    vis = np.nonzero((fw["radii"] > 0) & (fw["rho"] < 0.8))[0]
    assert len(vis) >= 3
    pick = vis[np.argsort(-np.abs(g["opacity"][vis]))[:3]]
    for k, cols in (("scales", (0, 2)), ("rotation", (0, 3)), ("opacity", (None,)), ("xyz", (0, 1))):
        for i in pick:
            for j in cols:
                idx = (i,) if j is None else (i, j)

                def L(d):
                    q = dict(p64); q[k] = p64[k].copy(); q[k][idx] += d
                    return aa_loss(o, q, c, W, H, tgt)[0]
                fd = (L(_FD_H) - L(-_FD_H)) / (2 * _FD_H)
                gk = float(g[k][idx])
                assert abs(gk - fd) <= 2e-2 * max(abs(fd), abs(gk)) + 1e-9, (k, idx, gk, fd)


# ------------------------------------------------------------------------------------------------------- the entry point
def test_header_declares_entry():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "int gs_set_antialiasing(gs_ctx* ctx, int enable);" in src
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import _lib
    assert "gs_set_antialiasing" in _lib.exported_symbols()


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import _lib
    lib = _lib.load()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    assert lib.gs_set_antialiasing(None, 1) == invalid
    assert lib.gs_set_antialiasing(None, 0) == invalid
    assert lib.gs_set_pose_correction(None, None, None) == invalid       # (the convention it follows)
