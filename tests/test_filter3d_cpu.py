"""The 3-D smoothing filter without a device (include/gsplat.h gs_set_filter3d): the float64 width rule on
hand-built cases, the filtered activations and their VJP against central differences, the composed oracle this file defines
for the GPU tests (the reference's ops on s_eff with sigma kappa (rho) packed) against central differences of its own loss,
the bake, and the entry points' declaration, export and null-context refusal.

Bars.  The activations' VJP: central differences in float64 at a step of 1e-6 of the entry's scale (raw scales of order 1:
h = 1e-6); truncation is O(h^2) of the third derivative, well below the 1e-6 relative bar (test_antialiasing_cpu's bar and
step rule).  The composed oracle: 2 % of the larger of the two values at h = 1e-4 in raw parameters -- the oracle's 3-sigma
tile cull and integer radii make its loss piecewise smooth (that file's bar, _FD_H and cause).  Mass: 1e-15 relative.  Bake:
the oracle's render of the baked parameters against its filtered render at 1e-12 (exp(log s_eff) is s_eff to 2 ulp).
"""
import os

import numpy as np
import pytest

from gaussiansplattingmlx_amd import filter3d as f3
from gaussiansplattingmlx_amd.antialias import opacity_scale, opacity_scale_vjp
from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
ENTRIES = ("gs_set_filter3d_cameras", "gs_compute_filter3d", "gs_set_filter3d", "gs_filter3d_bake")


# ---------------------------------------------------------------------------------------------------- the composed oracle
class Filter3DOracle:
    """Oracle.render_forward / render_backward under a fixed filter `filt` [N] (float64), composed from the reference's ops:
    activations_forward -> the filter on ITS sigma and s (filter3d.filter_scales, in the oracle's own precision: the float64
    oracle is the statement the kernels are held to, the float32 one their arithmetic in a float32 loop) -> projection_forward(s_eff)
    (-> rho in float64 if aa) -> pack_gaussians with sigma kappa (rho) (radius 0 where rho = 0) -> tile_bin -> blend_forward;
    blend_backward -> (aa: cotCov2d = VJP of rho at c sigma kappa) -> projection_backward(s_eff) -> the filter's chain rule
    (filter3d.filter_vjp) for the raw scales and opacity, activations_backward for the rotation.  Everything else is the wrapped
    Oracle's."""

    def __init__(self, o, filt, aa=False):
        self.o, self.dtype, self.aa = o, o.dtype, bool(aa)
        self.filt = np.asarray(filt, np.float64).reshape(-1)

    def __getattr__(self, k):
        return getattr(self.o, k)

    def render_forward(self, params, cam, W, H, tileW, tileH, degree, whiteBg=False):
        o = self.o
        N = np.shape(params["xyz"])[0]
        f = self.filt[:N]
        op, sc, rt = o.activations_forward(params["opacity"], params["scales"], params["rotation"])
        se, kappa = f3.filter_scales(sc, f, self.dtype)
        shs = np.concatenate([o._r(params["features_dc"]), o._r(params["features_rest"])], axis=1)
        pr = o.projection_forward(se.astype(self.dtype), rt, params["xyz"], shs, cam["camCenter"], cam["view"], cam["proj"],
                                  cam["fovX"], cam["fovY"], cam["focalX"], cam["focalY"], W, H, degree)
        rho = opacity_scale(pr["cov2d"]) if self.aa else np.ones(N)
        radii = np.where(rho > 0, pr["radii"], 0).astype(self.dtype)
        sig = op.astype(np.float64).reshape(-1)
        packed = o.pack_gaussians(pr["means2d"], pr["conic"], pr["color"],
                                  (sig * kappa.astype(np.float64) * rho).astype(self.dtype), pr["depths"])
        bn = o.tile_bin(pr["rectMin"], pr["rectMax"], radii, pr["depths"], W, H, tileW, tileH)
        color, depth, alpha, last = o.blend_forward(packed, bn.sortedIdx, bn.tileRanges, W, H, tileW, tileH, whiteBg)
        return dict(opacity=op, sigma=sig, s=sc, scales=se, kappa=kappa.astype(np.float64), rot=rt, shs=shs, proj=pr, rho=rho, radii=radii, packed=packed,
                    bin=bn, color=color, depth=depth, alpha=alpha, last=last)

    def render_backward(self, params, cam, W, H, tileW, tileH, degree, fwd, cotColor, cotDepth, cotAlpha, whiteBg=False):
        o, bn = self.o, fwd["bin"]
        gp = o.blend_backward(fwd["packed"], bn.sortedIdx, bn.tileRanges, W, H, tileW, tileH, whiteBg, cotColor, cotDepth,
                              cotAlpha, fwd["color"], fwd["depth"], fwd["alpha"], fwd["last"])
        N = gp.shape[0]
        f = self.filt[:N]
        c = gp[:, 9].astype(np.float64)
        cotCov = np.zeros((N, 4))
        if self.aa:
            cotCov = opacity_scale_vjp(fwd["proj"]["cov2d"], c * fwd["sigma"] * fwd["kappa"]).reshape(N, 4)
        pb = o.projection_backward(fwd["scales"].astype(self.dtype), fwd["rot"], params["xyz"], fwd["shs"], cam["camCenter"],
                                   cam["view"], cam["proj"], cam["fovX"], cam["fovY"], cam["focalX"], cam["focalY"], W, H, degree,
                                   gp[:, 10], gp[:, 0:2], cotCov.astype(self.dtype), gp[:, 6:9], gp[:, 2:6])
        ds, do = f3.filter_vjp(fwd["s"], fwd["sigma"], f, pb["gradScales"], c, fwd["rho"])
        _, _, dq = o.activations_backward(params["opacity"], params["scales"], params["rotation"], np.zeros(N, self.dtype),
                                          np.zeros((N, 3), self.dtype), pb["gradRot"])
        return dict(xyz=pb["gradMeans3d"], features_dc=pb["gradShs"][:, :1, :].copy(),
                    features_rest=pb["gradShs"][:, 1:, :].copy(), scales=ds.astype(self.dtype), rotation=dq,
                    opacity=do.astype(self.dtype).reshape(np.shape(params["opacity"])), gradPacked=gp)


def f3d_loss(o, p, cam, W, H, target, tile=(16, 16), lam=0.2):
    fw = o.render_forward(p, cam, W, H, tile[0], tile[1], 4)
    loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), target, lam)
    return float(loss), fw, cot


# -------------------------------------------------------------------------------------------------------- the width rule
def _axis_cam(eye, target, W=200, H=100, focal=100.0):
    return Camera(W, H, focal, focal, look_at_c2w(eye, target, up=(0.0, 0.0, 1.0)))


def test_width_one_camera_one_point_on_the_axis():
    cam = _axis_cam([0.0, -5.0, 0.0], [0.0, 0.0, 0.0])
    f = f3.filter_width(np.array([[0.0, -2.0, 0.0]]), [cam])
    assert abs(f[0] - np.sqrt(0.2) * 3.0 / 100.0) <= 1e-6 * f[0]      # (the view matrix is float32)


def test_width_takes_the_near_cameras_interval():
    near, far = _axis_cam([0.0, -2.0, 0.0], [0.0, 0.0, 0.0]), _axis_cam([0.0, -9.0, 0.0], [0.0, 0.0, 0.0])
    x = np.array([[0.1, 0.0, 0.05]])
    for cams in ([near, far], [far, near]):
        f, seen, arg = f3.filter_width(x, cams, details=True)
        assert seen[0] and cams[arg[0]] is near
        assert abs(f[0] - np.sqrt(0.2) * 2.0 / 100.0) <= 1e-6 * f[0]
    # a camera with a longer focal samples more finely at the same depth: it sets the width
    tele = _axis_cam([0.0, -2.0, 0.0], [0.0, 0.0, 0.0], focal=400.0)
    assert abs(f3.filter_width(x, [near, tele])[0] - np.sqrt(0.2) * 2.0 / 400.0) <= 1e-8


def test_width_of_a_point_behind_every_camera_is_the_max_over_the_seen():
    cams = [_axis_cam([0.0, -5.0, 0.0], [0.0, 0.0, 0.0]), _axis_cam([0.0, -4.0, 0.5], [0.0, 0.0, 0.0])]
    x = np.array([[0.0, 0.0, 0.0], [0.0, -3.0, 0.1], [0.0, -30.0, 0.0], [0.2, 1.5, 0.0]])      # row 2: behind both
    f, seen, _ = f3.filter_width(x, cams, details=True)
    assert seen.tolist() == [True, True, False, True]
    assert f[2] == f[[0, 1, 3]].max() and f[2] > 0
    assert f[3] == f[2]            # (the furthest seen point is the widest)


def test_width_nothing_seen_gives_zeros():
    cams = [_axis_cam([0.0, -5.0, 0.0], [0.0, 0.0, 0.0])]
    x = np.array([[0.0, -30.0, 0.0], [0.0, -5.1, 0.0], [50.0, 0.0, 0.0]])
    f, seen, arg = f3.filter_width(x, cams, details=True)
    assert not seen.any() and (arg == -1).all() and np.array_equal(f, np.zeros(3))
    assert np.array_equal(f3.filter_width(np.zeros((0, 3)), cams), np.zeros(0))


def test_width_margin_just_inside_and_just_outside():
    W, H, focal, z = 200, 100, 100.0, 4.0
    cam = _axis_cam([0.0, -z, 0.0], [0.0, 0.0, 0.0], W, H, focal)
    limx, limy = 1.3 * np.tan(float(cam.FoVx) / 2), 1.3 * np.tan(float(cam.FoVy) / 2)
    assert abs(limx - 0.65 * W / focal) < 1e-6 and abs(limy - 0.65 * H / focal) < 1e-6      # Mip-Splatting's 15 % margin
    # look_at_c2w: x right, y down, z forward; at world y = 0 the depth is z.  The image's x axis is the world's x axis up to sign.
    for axis, lim in ((0, limx), (2, limy)):
        x = np.zeros((2, 3))
        x[0, axis], x[1, axis] = z * lim * (1 - 1e-3), z * lim * (1 + 1e-3)
        f, seen, _ = f3.filter_width(x, [cam], details=True)
        assert seen.tolist() == [True, False], axis
        assert f[1] == f[0]
    # ... and the depth threshold
    x = np.array([[0.0, -z + 0.2 * (1 + 1e-3), 0.0], [0.0, -z + 0.2 * (1 - 1e-3), 0.0]])
    assert f3.filter_width(x, [cam], details=True)[1].tolist() == [True, False]
    assert f3.threshold_distance(x, [cam]) < 2e-3 < f3.threshold_distance(np.zeros((1, 3)), [cam])


# ------------------------------------------------------------------------------------------------------ the activations
def test_zero_filter_is_the_identity():
    raw = np.random.default_rng(1).normal(-3.0, 1.5, (50, 3))
    se, kappa = f3.activations(raw, np.zeros(50))
    assert np.array_equal(se, np.exp(raw)) and np.array_equal(kappa, np.ones(50))
    # ... in float32 too: sqrt(s s) = s under correct rounding (what the kernels rely on)
    s = np.exp(raw.astype(np.float32))
    assert np.array_equal(np.sqrt(s * s), s)


def test_wide_filter_limit():
    raw = np.log(np.array([[1e-3, 2e-3, 5e-4]]))
    f = np.array([0.5])
    se, kappa = f3.activations(raw, f)
    want = np.prod(np.exp(raw) / f[:, None], axis=1)
    # s_a / s_eff_a = (s_a / f) (1 + (s_a / f)^2)^-1/2: the product falls short of prod s_a / f by sum (s_a / f)^2 / 2 to first order
    short = 0.5 * ((np.exp(raw) / 0.5) ** 2).sum()
    # (second order: 3/8 sum x_a^2 + 1/4 sum_{a<b} x_a x_b <= (sum x_a)^2 = 4 short^2, x_a = (s_a / f)^2)
    assert abs(kappa[0] / want[0] - (1 - short)) <= 4 * short ** 2 and short < 2e-5
    assert np.all(se >= 0.5) and np.all(se - 0.5 <= 1e-5)


def test_mass_is_preserved():
    """kappa sqrt(det Sigma3_eff) = sqrt(det Sigma3): the widened Gaussian carries the unwidened one's mass."""
    rng = np.random.default_rng(2)
    raw, f = rng.normal(-3.0, 1.0, (200, 3)), np.exp(rng.normal(-3.0, 1.0, 200))
    se, kappa = f3.activations(raw, f)
    lhs, rhs = kappa * np.prod(se, axis=1), np.prod(np.exp(raw), axis=1)
    assert np.abs(lhs - rhs).max() <= 1e-15 * np.abs(rhs).max() and np.all(np.abs(lhs / rhs - 1) <= 1e-15)


def test_activation_vjp_against_central_differences():
    rng = np.random.default_rng(3)
    n = 40
    raw, op = rng.normal(-3.0, 1.0, (n, 3)), rng.normal(0.0, 2.0, n)
    f = np.exp(rng.normal(-3.0, 1.0, n))
    f[:4] = 0.0
    w, c, rho = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, n), rng.uniform(0.2, 1.0, n)

    def L(raw_, op_):
        se, kappa = f3.activations(raw_, f)
        sg = 1.0 / (1.0 + np.exp(-op_))
        return (w * se).sum(axis=1) + c * sg * rho * kappa           # per row: the rows are independent
    ds, do = f3.activations_vjp(raw, op, f, w, c, rho)
    h = 1e-6
    for a in range(3):
        e = np.zeros((n, 3)); e[:, a] = h
        fd = (L(raw + e, op) - L(raw - e, op)) / (2 * h)
        assert np.abs(ds[:, a] - fd).max() <= 1e-6 * np.abs(fd).max() + 1e-15, a
        assert np.all(np.abs(ds[:, a] - fd) <= 1e-6 * np.maximum(np.abs(fd), np.abs(fd).max() * 1e-3)), a
    fd = (L(raw, op + h) - L(raw, op - h)) / (2 * h)
    assert np.abs(do - fd).max() <= 1e-6 * np.abs(fd).max() + 1e-15
    # f = 0: the plain activations' VJP, g s and c rho sigma (1 - sigma)
    sg = 1.0 / (1.0 + np.exp(-op[:4]))
    assert np.allclose(ds[:4], w[:4] * np.exp(raw[:4]), rtol=1e-15, atol=0)
    assert np.allclose(do[:4], c[:4] * rho[:4] * sg * (1 - sg), rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------- the composed oracle
_FD_H = 1e-4


def _fd_scene():
    """test_antialiasing_cpu's scene; the filter of its one camera: 0.45 x 4.4 / 60 = 0.033 against scales of ~0.03."""
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    W = H = 64
    p = make_gaussians(60, "trained_like", 3)
    p["scales"] = (p["scales"] + 0.4).astype(np.float32)
    cam = Camera(W, H, 60.0, 60.0, look_at_c2w([3.0, -2.5, 2.0]))
    return p, cam, W, H


@pytest.mark.parametrize("aa", [False, True])
def test_composed_oracle_chain_rule_against_central_differences(oracle64, aa):
    """The hand-written chain rule of Filter3DOracle.render_backward against float64 central differences of its own loss, on raw
    scale, rotation, opacity and xyz elements of visible splats with kappa < 0.8 (where the filter matters)."""
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    p, cam, W, H = _fd_scene()
    filt = f3.filter_width(p["xyz"], [cam])
    o = Filter3DOracle(oracle64, filt, aa)
    c = cam.as_dict()
    tgt = oracle64.render_forward(make_gaussians(60, "trained_like", 4), c, W, H, 16, 16, 4)["color"].reshape(H, W, 3)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    _, fw, cot = f3d_loss(o, p64, c, W, H, tgt)
    z = np.zeros(W * H)
    g = o.render_backward(p64, c, W, H, 16, 16, 4, fw, cot.reshape(-1, 3), z, z)
    vis = np.nonzero((fw["radii"] > 0) & (fw["kappa"] < 0.8))[0]
    assert len(vis) >= 3
    pick = vis[np.argsort(-np.abs(g["opacity"][vis]))[:3]]
    for k, cols in (("scales", (0, 2)), ("rotation", (0, 3)), ("opacity", (None,)), ("xyz", (0, 1))):
        for i in pick:
            for j in cols:
                idx = (i,) if j is None else (i, j)

                def L(d):
                    q = dict(p64); q[k] = p64[k].copy(); q[k][idx] += d
                    return f3d_loss(o, q, c, W, H, tgt)[0]
                fd = (L(_FD_H) - L(-_FD_H)) / (2 * _FD_H)
                gk = float(g[k][idx])
                assert abs(gk - fd) <= 2e-2 * max(abs(fd), abs(gk)) + 1e-9, (k, idx, gk, fd)


@pytest.mark.parametrize("aa", [False, True])
def test_baked_parameters_render_as_the_filtered_model(oracle64, aa):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_f3d_aa_cpu", os.path.join(ROOT, "tests", "test_antialiasing_cpu.py"))
    aa_cpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aa_cpu)
    AAOracle = aa_cpu.AAOracle
    p, cam, W, H = _fd_scene()
    filt = f3.filter_width(p["xyz"], [cam])
    c = cam.as_dict()
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    want = Filter3DOracle(oracle64, filt, aa).render_forward(p64, c, W, H, 16, 16, 4)
    baked = dict(p64)
    baked["scales"], baked["opacity"] = f3.bake(p64["scales"], p64["opacity"], filt)
    plain = AAOracle(oracle64) if aa else oracle64
    got = plain.render_forward(baked, c, W, H, 16, 16, 4)
    assert want["kappa"].min() < 0.8 and np.abs(want["color"]).max() > 0.1
    for k in ("color", "alpha", "depth"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12, k
    # the bake's own statements
    se, kappa = f3.activations(p64["scales"], filt)
    sg = 1 / (1 + np.exp(-p64["opacity"].reshape(-1)))
    assert np.allclose(np.exp(baked["scales"]), se, rtol=1e-14, atol=0)
    assert np.allclose(1 / (1 + np.exp(-baked["opacity"])), sg * kappa, rtol=1e-13, atol=0)
    z = f3.bake(p64["scales"], p64["opacity"], np.zeros(60))
    assert np.allclose(z[0], p64["scales"], rtol=0, atol=1e-15) and np.allclose(z[1], p64["opacity"].reshape(-1), rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------------ the entry points
def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    for decl in ("int gs_set_filter3d_cameras(gs_ctx* ctx, int V, const gs_camera* cams",
                 "int gs_compute_filter3d(gs_ctx* ctx, int N, const float* xyz",
                 "int gs_set_filter3d(gs_ctx* ctx, const float* filter",
                 "int gs_filter3d_bake(gs_ctx* ctx, int N, const float* scales_raw"):
        assert decl in src, decl
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import _lib
    for name in ENTRIES:
        assert name in _lib.exported_symbols(), name


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import _lib
    lib = _lib.load()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    assert lib.gs_set_filter3d_cameras(None, 0, None) == invalid
    assert lib.gs_compute_filter3d(None, 0, None, None) == invalid
    assert lib.gs_set_filter3d(None, None) == invalid
    assert lib.gs_filter3d_bake(None, 0, None, None, None, None, None) == invalid
    assert lib.gs_set_antialiasing(None, 1) == invalid       # (the convention they follow)

