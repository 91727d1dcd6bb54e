"""Normal regularisation, host side: the numpy restatement of gs_normal_loss against central differences
of its own float64 loss, the normals of a plane, max_jump, NormalConfig, the trainer's refusals, the loaders' normal priors, the
header / binding agreement.

Finite differences.  The loss is smooth in (D, a) as long as no pixel changes its validity, its max_jump verdict or the sign of
a component n_c - Nt_c.  h = 1e-8: 1 / (2 z / fx) amplifies a depth step into the normal, so a larger step crosses the L1
term's kinks (at 1e-6 it does), while the thresholds (alpha at least 0.5 above alpha_min, the 0.01 block far below it) are
never near.  A direction is zero on the stencil of a pixel within 1e-5 of a kink (_near_a_kink: at most 1.1 % of the pixels): at
152 x 200 one such pixel otherwise changes the sign its L1 term takes inside the step, which a central difference reads as 1e-4 of
error.  The error of a central difference is then the float64 rounding of a total of order 1 divided by 2 h, about 1e-8
absolute, beside a truncation term far below it.

The bar is 1e-6 of the derivative g . d itself, along random directions in depth, in alpha and in both whose derivative does
not cancel: d_i = |r_i| sign(g_i) with r normal ("aligned"), and the same with the sign left to chance on a random half of the
pixels ("half").  Along a direction with signs all left to chance g . d is a sum of terms of either sign and now and then
cancels to a small fraction of its usual size, while the 1e-8 of rounding stays: of |g . d| that was up to 3e-6 here, which says
nothing about the cotangents.  Such directions are checked as well, as an addition and against the size such a derivative has,
max(|g . d|, sqrt(sum (g_i d_i)^2)); the printed lines give every figure both ways.  Measured: at most 4.2e-9 of g . d along the
aligned and half directions, at most 6.2e-8 of that size along the directions left to chance."""
import ctypes as C
import importlib.util
import os
import re
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FD_H, FD_BAR = 1e-8, 1e-6


def _load(name):
    spec = importlib.util.spec_from_file_location("_nlc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


nln = _load("normal_loss_numpy")
TERMS = {"l1": (0.7, 0.0, 0.0), "cos": (0.0, 0.6, 0.0), "smooth": (0.0, 0.0, 0.9), "all": (0.7, 0.6, 0.9)}


# ------------------------------------------------------------------------------------------------------------ the restatement
def _near_a_kink(s, r, max_jump, eps=1e-5):
    """The pixels a direction leaves alone: the stencil (the pixel and its four neighbours) of every pixel whose prior has a
    component |n_c - Nt_c| < eps, or whose depth differences are within eps of the max_jump threshold.  A step of h = 1e-8 moves
    a normal by about h fx / z, a few 1e-7: such a pixel may change the sign its L1 term takes, or its verdict, inside the step."""
    near = r["prior"] & (np.abs(r["n"] - r["Nt"]) < eps).any(-1)
    if max_jump > 0:
        z = np.where(r["valid"], s["D"].astype(np.float64) / np.where(r["valid"], s["a"], 1), 0.0)
        jump = np.maximum(np.abs(z[1:-1, 2:] - z[1:-1, :-2]), np.abs(z[2:, 1:-1] - z[:-2, 1:-1]))
        near[1:-1, 1:-1] |= np.abs(jump - np.float64(np.float32(max_jump)) * z[1:-1, 1:-1]) < eps
    out = near.copy()
    out[:, 1:] |= near[:, :-1]
    out[:, :-1] |= near[:, 1:]
    out[1:] |= near[:-1]
    out[:-1] |= near[1:]
    return out


@pytest.mark.parametrize("H,W", [(37, 53), (152, 200)])
@pytest.mark.parametrize("term", list(TERMS))
def test_cotangents_are_the_derivatives_of_the_float64_loss(H, W, term):
    s = nln.scene(H, W)
    D, a = s["D"].astype(np.float64), s["a"].astype(np.float64)
    mj, gap, dropped = nln.pick_max_jump(s)
    kw = dict(target=s["target"], mask=s["mask"], edge=s["edge"], lam=TERMS[term], gamma=2.0, max_jump=mj if term == "all" else 0.0)
    r = nln.normal_loss(s["K"], D, a, **kw)
    if term == "all":
        assert dropped >= 10 and int(nln.depth_normals(s["K"], D, a)[1].sum()) - int(r["has"].sum()) == dropped
    cd, ca = r["cot_depth"], r["cot_alpha"]
    assert r["has"].any() and r["prior"].any() and not r["valid"].all()
    assert np.isfinite(cd).all() and np.isfinite(ca).all() and not cd[~r["valid"]].any() and not ca[~r["valid"]].any()
    assert cd[0, 1:-1].any() and cd[1:-1, 0].any()            # border pixels have no normal but do receive cotangents
    free = ~_near_a_kink(s, r, kw["max_jump"])
    print(f"{H}x{W} {term}: {int((~free).sum())} of {H * W} pixels held still (a stencil with a near tie or a near edge)")
    assert free.mean() > 0.97
    rng = np.random.default_rng(3)
    worst = {"aligned": 0.0, "half": 0.0, "chance": 0.0}
    for which in ("depth", "alpha", "both"):
        for kind in ("aligned", "half", "chance"):
            rD, rA = rng.normal(size=(H, W)), rng.normal(size=(H, W)) * 0.1
            if kind != "chance":
                keep = np.ones((H, W), bool) if kind == "aligned" else rng.uniform(size=(H, W)) < 0.5
                rD = np.where(keep, np.abs(rD) * np.sign(cd), rD)
                rA = np.where(keep, np.abs(rA) * np.sign(ca), rA)
            vD, vA = rD * (which != "alpha") * free, rA * (which != "depth") * free
            fd = (nln.total(s["K"], D + FD_H * vD, a + FD_H * vA, **kw) - nln.total(s["K"], D - FD_H * vD, a - FD_H * vA, **kw)) / (2 * FD_H)
            want = float((cd * vD).sum() + (ca * vA).sum())
            scale = max(abs(want), float(np.sqrt(((cd * vD) ** 2).sum() + ((ca * vA) ** 2).sum())))
            print(f"{H}x{W} {term} {which} {kind}: finite difference {fd:.12g}, cotangents {want:.12g}, "
                  f"|diff| / |cotangents| {abs(fd - want) / abs(want):.3g}, |diff| / scale {abs(fd - want) / scale:.3g}")
            if kind == "chance":
                worst[kind] = max(worst[kind], abs(fd - want) / scale)
                assert abs(fd - want) <= FD_BAR * scale, (term, which, kind, fd, want, scale)
            else:
                worst[kind] = max(worst[kind], abs(fd - want) / abs(want))
                assert abs(want) >= 0.5 * scale                       # (the derivative did not cancel)
                assert abs(fd - want) <= FD_BAR * abs(want), (term, which, kind, fd, want)
    print(f"{H}x{W} {term}: worst {worst}")


def test_float32_restatement_and_edges():
    H, W = 37, 53
    s = nln.scene(H, W)
    kw = dict(target=s["target"], mask=s["mask"], edge=s["edge"], lam=TERMS["all"], gamma=2.0)
    r64 = nln.normal_loss(s["K"], s["D"], s["a"], **kw)
    r32 = nln.normal_loss(s["K"], s["D"], s["a"], dtype=np.float32, **kw)
    assert r32["cot_depth"].dtype == np.float32 and r32["n"].dtype == np.float32
    assert np.array_equal(r32["has"], r64["has"]) and r32["counts"] == r64["counts"]
    assert np.abs(r32["n"] - r64["n"]).max() <= 2e-4 and np.abs(np.subtract(r32["terms"], r64["terms"])).max() <= 2e-6
    # a target of all holes, and none at all: the prior terms are 0 and the rest is the smoothness term's
    sm = nln.normal_loss(s["K"], s["D"], s["a"], edge=s["edge"], lam=TERMS["all"], gamma=2.0)
    holes = nln.normal_loss(s["K"], s["D"], s["a"], target=0.4 * s["target"], edge=s["edge"], lam=TERMS["all"], gamma=2.0)
    only = nln.normal_loss(s["K"], s["D"], s["a"], edge=s["edge"], lam=TERMS["smooth"], gamma=2.0)
    for x in (sm, holes):
        assert x["terms"][:2] == (0.0, 0.0) and x["terms"][2] == only["terms"][2] and np.array_equal(x["cot_depth"], only["cot_depth"])
    # no edge image, or gamma = 0: every pair weighs exactly 1
    flat = nln.normal_loss(s["K"], s["D"], s["a"], lam=TERMS["smooth"])
    assert flat["terms"][2] == nln.normal_loss(s["K"], s["D"], s["a"], edge=s["edge"], lam=TERMS["smooth"], gamma=0.0)["terms"][2]
    assert flat["terms"][2] > only["terms"][2] > 0
    # images without an interior, and without a depth-valid pixel: zeros, nothing NaN
    for h, w in ((2, 64), (64, 2), (1, 1)):
        t = nln.scene(h, w)
        e = nln.normal_loss(t["K"], t["D"], t["a"], target=t["target"], edge=t["edge"], lam=TERMS["all"], gamma=2.0, dtype=np.float32)
        assert e["terms"] == (0.0, 0.0, 0.0) and not e["cot_depth"].any() and not e["cot_alpha"].any() and not e["has"].any()
    e = nln.normal_loss(s["K"], s["D"], 0 * s["a"], **kw)
    assert e["terms"] == (0.0, 0.0, 0.0) and not e["cot_depth"].any() and not e["cot_alpha"].any()
    # one depth-valid island smaller than the stencil: no normal
    a = np.zeros((H, W), np.float32)
    a[10:12, 20:23] = 0.9
    e = nln.normal_loss(s["K"], s["D"], a, **kw)
    assert not e["has"].any() and e["valid"].sum() == 6 and not e["cot_depth"].any()


def _plane(H, W, n0, d, K):
    fx, fy, cx, cy = K
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    rx, ry = ((i + 0.5) - cx) / fx, ((j + 0.5) - cy) / fy
    return d / (n0[0] * rx + n0[1] * ry + n0[2]), np.stack([rx, ry, np.ones_like(rx)], -1)


def test_the_normals_of_a_plane_are_the_planes_and_face_the_camera():
    H, W = 29, 41
    K = tuple(float(np.float32(v)) for v in (0.9 * W, 0.8 * W, W / 2 + 1.7, H / 2 - 2.3))      # (as the C ABI takes them)
    rng = np.random.default_rng(1)
    for n0 in ((0.0, 0.0, -1.0), (0.3, -0.2, -1.0), (-0.5, 0.4, -1.0)):
        n0 = np.asarray(n0) / np.linalg.norm(n0)
        z, rays = _plane(H, W, n0, -4.0, K)              # n0 . P = -4: the plane lies in front of the camera
        assert (z > 1).all()
        a = rng.uniform(0.3, 1.0, (H, W))
        n, has = nln.depth_normals(K, z * a, a)
        assert has[1:-1, 1:-1].all() and not has[0].any() and not has[-1].any() and not has[:, 0].any() and not has[:, -1].any()
        assert not n[~has].any()
        print(f"plane {n0}: max |n - n0| {np.abs(n[has] - n0).max():.3g}")
        assert np.abs(n[has] - n0).max() <= 1e-9
        assert ((n * rays).sum(-1)[has] < 0).all()
        n32, has32 = nln.depth_normals(K, (z * a).astype(np.float32), a.astype(np.float32), dtype=np.float32)
        assert np.array_equal(has32, has) and ((n32 * rays).sum(-1)[has] < 0).all()


def test_max_jump_drops_the_pixels_along_a_depth_step_and_nothing_else():
    H, W = 21, 30
    K = (0.9 * W, 0.9 * W, W / 2, H / 2)
    z = np.where(np.arange(W)[None, :] < W // 2, 4.0, 5.0) * np.ones((H, 1))
    a = np.full((H, W), 0.8)
    interior = np.zeros((H, W), bool)
    interior[1:-1, 1:-1] = True
    _, has = nln.depth_normals(K, z * a, a, max_jump=0.0)
    assert np.array_equal(has, interior)
    _, has = nln.depth_normals(K, z * a, a, max_jump=0.1)
    step = np.zeros((H, W), bool)
    step[:, W // 2 - 1: W // 2 + 1] = True
    assert np.array_equal(has, interior & ~step)
    _, has = nln.depth_normals(K, z * a, a, max_jump=0.3)       # 1 <= 0.3 x 4: the step is no edge at this setting
    assert np.array_equal(has, interior)
    zr = z.T.copy()                                              # the same step between two rows
    _, has = nln.depth_normals((0.9 * H, 0.9 * H, H / 2, W / 2), zr * 0.8, np.full((W, H), 0.8), max_jump=0.1)
    assert np.array_equal(has, (interior & ~step).T)


# ------------------------------------------------------------------------------------------------------------ the settings
def test_normal_config():
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    c = NormalConfig().validate()
    assert (c.l1_weight, c.cos_weight, c.smooth_weight, c.alpha_min, c.max_jump, c.edge_gamma, c.start) == (0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0)
    assert not c.wants_prior and NormalConfig(cos_weight=0.1).wants_prior
    c = NormalConfig(l1_weight=0.25, cos_weight=(1.0, 0.01), smooth_weight=[2.0, 0.5], start=7).validate()
    assert c.weights_at(0, 30000) == pytest.approx((0.25, 1.0, 2.0), rel=1e-12)
    assert c.weights_at(15000, 30000) == pytest.approx((0.25, 0.1, 1.0), rel=1e-12)
    assert c.weights_at(10 ** 6, 30000) == pytest.approx((0.25, 0.01, 0.5), rel=1e-12)
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    assert c.weights_at(1234, 7000)[1] == DepthConfig(weight=(1.0, 0.01)).weight_at(1234, 7000)
    for name in ("l1_weight", "cos_weight", "smooth_weight"):
        for bad in (-1.0, float("nan"), True, (1.0,), (1.0, 0.0), (1.0, float("inf")), "1", (1.0, "x"), None):
            with pytest.raises(ValueError, match=name):
                NormalConfig(**{name: bad}).validate()
    for bad in (dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=float("nan")), dict(alpha_min=None), dict(alpha_min=True),
                dict(max_jump=-1.0), dict(max_jump=float("inf")), dict(max_jump="0"), dict(edge_gamma=-2.0),
                dict(edge_gamma=float("nan")), dict(start=-1), dict(start=1.5), dict(start=True), dict(start=None)):
        with pytest.raises(ValueError):
            NormalConfig(**bad).validate()
    assert "tuned" in NormalConfig.__doc__


# ------------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(normal="smooth"), dict(normal=True), dict(normal=1.0),
                                dict(normal="config:bad-weight"), dict(normal="config:bad-start")])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(normal=NormalConfig(smooth_weight=0.1))
    args.update(kw)
    if args["normal"] == "config:bad-weight":
        args["normal"] = NormalConfig(smooth_weight=(1.0, -1.0))
    elif args["normal"] == "config:bad-start":
        args["normal"] = NormalConfig(start=-3)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_train_step_refuses_a_prior_without_the_config_and_a_fisheye_camera_with_it():
    from gaussiansplattingmlx_amd.camera import Camera
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)         # (the checks come before anything else of the trainer is touched)
    tr.background = tr.depth = tr.normal = tr.pg = None
    tr.pose_opt = tr.filter_3d = False
    tr.exchange_impl, tr.viewsPerRank = "torch", 1
    with pytest.raises(ValueError, match="targetNormal"):
        tr.trainStep(None, None, targetNormal=np.zeros((2, 2, 3), np.float32))
    with pytest.raises(ValueError, match="normalMask"):
        tr.trainStep(None, None, normalMask=np.ones((2, 2), np.uint8))
    tr.normal = NormalConfig(smooth_weight=0.1)
    fish = Camera(8, 6, 7.0, 7.0, np.eye(4), model="fisheye")
    with pytest.raises(ValueError, match="pinhole"):
        tr.trainStep(fish, None)
    r = GaussianRenderer.__new__(GaussianRenderer)         # (the camera is looked at before the context is)
    r.W, r.H = 8, 6
    for call in (lambda: r.depthNormals((np.zeros((6, 8)), np.zeros((6, 8))), fish),
                 lambda: r.normalLossParams(fish, smooth_weight=0.1),
                 lambda: r.normalLoss(None, None, fish.as_dict(), None, None, None, dict(smooth_weight=0.1))):
        with pytest.raises(ValueError, match="fisheye"):
            call()
    p = r.normalLossParams(Camera(8, 6, 7.0, 7.5, np.eye(4), cx=4.5, cy=2.5), 0.1, 0.2, 0.3, 0.04, 0.5, 2.0, True)
    assert [getattr(p, n) for n, _ in p._fields_] == pytest.approx([7.0, 7.5, 4.5, 2.5, 6, 8, 0.1, 0.2, 0.3, 0.04, 0.5, 2.0, 1])
    assert r.normalLossParams((7.0, 7.5, 4.5, 2.5)).fx == 7.0 and r.normalLossParams(Camera(8, 6, 7.0, 7.5, np.eye(4))).cy == 3.0
    # a gs_camera (what renderForward is handed by callers that build their cameras once): the principal point from its matrix
    cam = Camera(8, 6, 7.0, 7.5, np.eye(4), cx=4.5, cy=2.5)
    g = r._camera(cam.worldViewTransform, cam.projectionMatrix, cam.cameraCenter, cam.FoVx, cam.FoVy, cam.focalX, cam.focalY)
    q = r.normalLossParams(g)
    assert (q.fx, q.fy) == (7.0, 7.5) and (q.cx, q.cy) == pytest.approx((4.5, 2.5), abs=1e-5)


# ------------------------------------------------------------------------------------------------------------- the loaders
def _colmap(root, names, W=8, H=6):
    from PIL import Image
    sparse, images = os.path.join(root, "sparse"), os.path.join(root, "images")
    os.makedirs(sparse, exist_ok=True)
    os.makedirs(images, exist_ok=True)
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<Ii", 1, 1) + struct.pack("<QQ", W, H) + struct.pack("<dddd", 10, 10, 4, 3))
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(names)))
        for i, n in enumerate(names):
            f.write(struct.pack("<I", i + 1) + struct.pack("<dddd", 1, 0, 0, 0) + struct.pack("<ddd", 0, 0, 0) +
                    struct.pack("<I", 1) + n.encode() + b"\x00" + struct.pack("<Q", 0))
            Image.fromarray(np.full((H, W, 3), 40 * i, np.uint8)).save(os.path.join(images, n))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<QdddBBBdQ", 1, 0.0, 0.0, 0.0, 255, 0, 0, 0.0, 0))
    return sparse, images


def _normal_png(path, n):
    """A unit normal image as an 8-bit RGB PNG: v = round(255 (n + 1) / 2)."""
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    v = np.rint(255.0 * (np.asarray(n, np.float64) + 1.0) / 2.0).astype(np.uint8)
    Image.fromarray(v).save(path)
    return np.float32(2.0) * (v.astype(np.float32) / np.float32(255.0)) - np.float32(1.0)


def _unit_normals(rng, H, W):
    n = rng.normal(size=(H, W, 3))
    n[..., 2] = -1.0 - np.abs(n[..., 2])
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def test_loaders_read_normal_priors(tmp_path):
    import json
    from PIL import Image
    from gaussiansplattingmlx_amd.data import ColmapDataLoader, NerfStudioDataLoader, TrainData, readNormalMap
    from gaussiansplattingmlx_amd.evaluation import split_train_data
    root = str(tmp_path / "colmap")
    sparse, images = _colmap(root, ["a.png", "b.png", "c.png"])
    nroot = os.path.join(root, "normals")
    rng = np.random.default_rng(4)
    na, nb = _unit_normals(rng, 6, 8), _unit_normals(rng, 6, 8)
    qa = _normal_png(os.path.join(nroot, "a.png"), na)
    qb = _normal_png(os.path.join(nroot, "b.png"), nb)
    data, _, _ = ColmapDataLoader(sparse, images, normalRoot=nroot).load()
    assert data.normalArray.dtype == np.float32 and data.normalArray.shape == (3, 6, 8, 3)
    assert np.array_equal(data.normalArray[0], qa) and np.array_equal(data.normalArray[1], qb)
    assert np.abs(data.normalArray[0] - na).max() <= 1.0 / 255.0 + 1e-6 and (data.normalArray[0][..., 2] < 0).all()
    assert not data.normalArray[2].any()                                  # c has no prior: all holes (squared norm < 0.25)
    gl, _, _ = ColmapDataLoader(sparse, images, normalRoot=nroot, normalConvention="opengl").load()
    assert np.array_equal(gl.normalArray[0], qa * np.float32([1, -1, -1])) and not gl.normalArray[2].any()
    # a 16-bit file reads as the same normals, to the precision the decoder keeps (PIL hands on a 16-bit RGB file's high bytes:
    # a component is at most 2 / 255 off)
    v16 = np.rint(65535.0 * (na + 1.0) / 2.0).astype(np.uint16)
    raw = b"".join(b"\x00" + v16[j].astype(">u2").tobytes() for j in range(6))
    import zlib

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))
    with open(os.path.join(nroot, "c.png"), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 8, 6, 16, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    n16 = readNormalMap(os.path.join(nroot, "c.png"))
    assert n16.shape == (6, 8, 3) and np.abs(n16 - na).max() <= 2.0 / 255.0 + 1e-6
    # resized with the images, on the float components
    half, _, _ = ColmapDataLoader(sparse, images, normalRoot=nroot).load(resizeFactor=0.5)
    assert half.normalArray.shape == (3, 3, 4, 3) and np.array_equal(half.normalArray[1], readNormalMap(os.path.join(nroot, "b.png"), 0.5))
    # the attribute is no dataclass field; replace and split_train_data carry it
    import dataclasses
    assert "normalArray" not in [f.name for f in dataclasses.fields(TrainData)]
    assert ColmapDataLoader(sparse, images).load()[0].normalArray is None
    assert data.replace(depthArray=None).normalArray is data.normalArray
    assert data.replace(normalArray=None).normalArray is None
    train, test = split_train_data(data, test_every=2)
    assert np.array_equal(test.normalArray, data.normalArray[[0, 2]]) and np.array_equal(train.normalArray, data.normalArray[[1]])
    plain = split_train_data(ColmapDataLoader(sparse, images).load()[0], test_every=2)
    assert plain[0].normalArray is None and plain[1].normalArray is None
    # refusals: undistort, an unknown convention, a file that is no RGB image
    with pytest.raises(ValueError, match="undistort"):
        ColmapDataLoader(sparse, images, normalRoot=nroot, cameraModels="colmap", undistort=True)
    with pytest.raises(ValueError, match="normalConvention"):
        ColmapDataLoader(sparse, images, normalRoot=nroot, normalConvention="directx")
    with pytest.raises(ValueError, match="undistort"):
        NerfStudioDataLoader(root, undistort=True, normalRoot=nroot)
    Image.fromarray(np.zeros((6, 8), np.uint8)).save(os.path.join(nroot, "b.png"))
    with pytest.raises(ValueError, match="RGB"):
        ColmapDataLoader(sparse, images, normalRoot=nroot).load()
    # nerfstudio: <normalRoot>/<the stem of the frame's file name>.png
    ns = str(tmp_path / "ns")
    os.makedirs(os.path.join(ns, "images"))
    Image.fromarray(np.full((6, 8, 3), 90, np.uint8)).save(os.path.join(ns, "images", "f0.png"))
    Image.fromarray(np.full((6, 8, 3), 30, np.uint8)).save(os.path.join(ns, "images", "f1.png"))
    with open(os.path.join(ns, "pts.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n0 0 0 255 0 0\n")
    frames = [dict(file_path=f"images/f{i}.png", transform_matrix=np.eye(4).tolist()) for i in range(2)]
    json.dump(dict(fl_x=10, fl_y=10, cx=4, cy=3, ply_file_path="pts.ply", frames=frames), open(os.path.join(ns, "transforms.json"), "w"))
    q1 = _normal_png(os.path.join(ns, "normals", "f1.png"), nb)
    nd, _, _ = NerfStudioDataLoader(ns, normalRoot=os.path.join(ns, "normals"), normalConvention="opengl").load()
    assert nd.normalArray.shape == (2, 6, 8, 3) and not nd.normalArray[0].any()
    assert np.array_equal(nd.normalArray[1], q1 * np.float32([1, -1, -1]))
    assert NerfStudioDataLoader(ns).load()[0].normalArray is None


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_and_binding_agree_on_the_new_entry_points():
    from gaussiansplattingmlx_amd import _lib
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("gs_normal_loss", 11), ("gs_depth_normals", 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]) and _lib._SIGS[name][0] is C.c_int
    m = re.search(r"typedef struct gs_normal_loss_params\s*\{(.*?)\}", code, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+([A-Za-z0-9_, ]+);", m.group(1))
    declared = [(t, n.strip()) for t, names in fields for n in names.split(",")]
    assert declared == [("float", "fx"), ("float", "fy"), ("float", "cx"), ("float", "cy"), ("int", "H"), ("int", "W"),
                        ("float", "lambda_l1"), ("float", "lambda_cos"), ("float", "lambda_smooth"), ("float", "alpha_min"),
                        ("float", "max_jump"), ("float", "edge_gamma"), ("int", "accumulate")]
    bound = [(("int" if t is C.c_int else "float" if t is C.c_float else "?"), n) for n, t in _lib.gs_normal_loss_params._fields_]
    assert bound == declared and C.sizeof(_lib.gs_normal_loss_params) == 52
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import build
    assert build.SOURCES["normal_loss.hip"] == ["-ffp-contract=off"]


def test_library_exports_and_refuses_without_a_context():
    from gaussiansplattingmlx_amd import build
    build.build()
    from gaussiansplattingmlx_amd import _lib
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    p = _lib.gs_normal_loss_params(10.0, 10.0, 4.0, 3.0, 6, 8, 0.1, 0.1, 0.1, 0.05, 0.0, 0.0, 0)
    assert _lib.STATUS.get(lib.gs_normal_loss(None, C.byref(p), *([None] * 9))) == "GS_ERR_INVALID_ARG"
    K = (C.c_float * 4)(10.0, 10.0, 4.0, 3.0)
    assert _lib.STATUS.get(lib.gs_depth_normals(None, K, 6, 8, None, None, C.c_float(0.05), C.c_float(0.0), None)) == "GS_ERR_INVALID_ARG"
    so = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"normals_kernel", b"nl_reduce_kernel", b"nl_final_kernel", b"nl_q_kernel", b"nl_gather_kernel"):
        assert kernel in so
