"""Depth supervision, host side: the numpy restatement of gs_depth_loss against finite differences of its
own float64 loss, DepthConfig, the trainer's argument checks, the COLMAP loader's depth priors, the header / binding agreement.

Finite differences: the loss lambda Ld is piecewise linear in D (accumulated), and smooth in (D, a) elsewhere, as long as no
pixel changes its validity or the sign of x - t.  The directions are therefore zero on pixels at the alpha threshold and on
ties; with |x - t| >= 5 % of x and a step of 1e-6 no other pixel gets near either.  Central differences of a function with
second derivatives of order x / a^2 <= 20 / 0.05^2 / n per pixel leave h^2 / 6 of the third derivative -- below 1e-8 relative
here --, and the float64 rounding of a loss of order 1 to 10 divided by 2 h = 2e-6 about 1e-9: the bar is 1e-6 of the analytic
value."""
import importlib.util
import json
import os
import re
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FD_H, FD_BAR = 1e-6, 1e-6


def _load(name):
    spec = importlib.util.spec_from_file_location("_dlc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dln = _load("depth_loss_numpy")


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("align", [(1.0, 0.0), (0.75, 0.125)])
def test_cotangents_are_the_derivatives_of_the_float64_loss(mode, align):
    H, W, lam, am = 23, 31, 0.3, 0.05
    D, a, target, mask = dln.inputs(H, W, mode, am)
    D64, a64 = D.astype(np.float64), a.astype(np.float64)
    scale, offset = align
    Ld, cd, ca, valid = dln.depth_loss(mode, D64, a64, target, mask, lam, am, scale, offset)
    assert valid.any() and not valid.all() and np.isfinite(cd).all() and np.isfinite(ca).all()
    assert not cd[~valid].any() and not ca[~valid].any()
    _, x = dln.valid_and_x(mode, D64, a64, mask, am)
    t = np.float64(np.float32(scale)) * target.astype(np.float64) + np.float64(np.float32(offset))
    free = valid & (np.abs(a64 - np.float64(np.float32(am))) > 1e-4 if mode else valid) & (x != t)
    if mode == 0 and align == (1.0, 0.0):
        assert (valid & (x == t)).any() and not cd[valid & (x == t)].any()      # the ties: cotangent 0
    rng = np.random.default_rng(3)
    f = lambda Dp, ap: dln.total(mode, Dp, ap, target, mask, lam, am, scale, offset)
    for k in range(6):
        vD, vA = rng.normal(size=(H, W)) * free, rng.normal(size=(H, W)) * free * 0.01
        if k < 2:
            vA = 0 * vA           # depth alone
        elif k < 4:
            vD = 0 * vD           # alpha alone
        fd = (f(D64 + FD_H * vD, a64 + FD_H * vA) - f(D64 - FD_H * vD, a64 - FD_H * vA)) / (2 * FD_H)
        want = float((cd * vD).sum() + (ca * vA).sum())
        if mode == 0 and k in (2, 3):
            assert fd == 0.0 and want == 0.0        # the accumulated depth does not see alpha
            continue
        print(f"mode {mode} direction {k}: finite difference {fd:.12g}, cotangents {want:.12g}")
        assert abs(fd - want) <= FD_BAR * abs(want), (mode, k, fd, want)
    # one pixel at a time
    ys, xs = np.nonzero(free)
    for j in rng.choice(len(ys), 5, replace=False):
        e = np.zeros((H, W))
        e[ys[j], xs[j]] = 1.0
        fd = (f(D64 + FD_H * e, a64) - f(D64 - FD_H * e, a64)) / (2 * FD_H)
        assert abs(fd - cd[ys[j], xs[j]]) <= 1e-5 * abs(cd[ys[j], xs[j]]), (fd, cd[ys[j], xs[j]])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_float32_restatement_and_edges(mode):
    H, W, lam, am = 23, 31, 0.3, 0.05
    D, a, target, mask = dln.inputs(H, W, mode, am)
    L64, cd64, ca64, v64 = dln.depth_loss(mode, D, a, target, mask, lam, am)
    L32, cd32, ca32, v32 = dln.depth_loss(mode, D, a, target, mask, lam, am, dtype=np.float32)
    assert cd32.dtype == np.float32 and np.array_equal(v32, v64)
    assert abs(float(L32) - float(L64)) <= 2e-6 * max(1.0, float(L64))
    for c32, c64 in ((cd32, cd64), (ca32, ca64)):
        nz = c64 != 0
        assert np.array_equal(c32 != 0, nz) and (np.abs(c32[nz] - c64[nz]) <= 1e-5 * np.abs(c64[nz])).all()
    if mode:       # the block exactly at alpha_min counts, the block of zeros does not
        assert v64[H // 5: 2 * (H // 5), : W // 4][mask[H // 5: 2 * (H // 5), : W // 4] != 0].all()
        assert not v64[: H // 5, : W // 4].any()
    # nothing valid: Ld = 0 and zero cotangents, nothing NaN -- a mask of zeros; alpha of zeros; depth of zeros (disparity)
    for Dz, az, mz in ((D, a, np.zeros((H, W), np.uint8)), (D, 0 * a, mask), (0 * D, a, mask)):
        if (mode == 0 and mz is mask) or (mode == 1 and Dz is not D):
            continue
        L, cd, ca, v = dln.depth_loss(mode, Dz, az, target, mz, lam, am, dtype=np.float32)
        assert float(L) == 0.0 and not v.any() and not cd.any() and not ca.any()
    # alpha_min = 0 does not divide by an alpha of zero
    L, cd, ca, v = dln.depth_loss(mode, D, a, target, None, lam, 0.0, dtype=np.float32)
    assert np.isfinite(L) and np.isfinite(cd).all() and np.isfinite(ca).all() and (mode == 0 or not v[: H // 5, : W // 4].any())
    e = dln.expected_depth(D, a, am)
    ok = (a >= np.float32(am)) & (a > 0)
    assert e.dtype == np.float32 and np.array_equal(e[ok], D[ok] / a[ok]) and not e[~ok].any()


# ------------------------------------------------------------------------------------------------------------ the settings
def test_depth_config():
    from gaussiansplattingmlx_amd.depth_loss import MODES, DepthConfig
    c = DepthConfig().validate()
    assert (c.mode, c.weight, c.alpha_min) == ("accumulated", 1.0, 0.05) and MODES == dln.MODES
    assert [DepthConfig(mode=m).validate().mode_id for m in MODES] == [dln.ACCUMULATED, dln.EXPECTED, dln.DISPARITY]
    assert all(DepthConfig(weight=0.25).weight_at(t, 1000) == 0.25 for t in (0, 1, 500, 999, 1000, 5000))
    inria = DepthConfig(mode="disparity", weight=(1.0, 0.01)).validate()
    assert inria.weight_at(0, 30000) == pytest.approx(1.0, rel=1e-12)
    assert inria.weight_at(30000, 30000) == pytest.approx(0.01, rel=1e-12)
    assert inria.weight_at(15000, 30000) == pytest.approx(0.1, rel=1e-12)            # the geometric midpoint
    assert inria.weight_at(10 ** 6, 30000) == pytest.approx(0.01, rel=1e-12)         # held behind the end
    from gaussiansplattingmlx_amd.trainer import exposureLearningRate
    assert DepthConfig(weight=(0.01, 0.001)).weight_at(1234, 7000) == exposureLearningRate(1234, 7000)
    assert DepthConfig(weight=[2.0, 0.5]).validate().weight_at(0, 10) == pytest.approx(2.0)
    for bad in (dict(mode="inverse"), dict(mode=1), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=True),
                dict(weight=(1.0,)), dict(weight=(1.0, 0.0)), dict(weight=(1.0, float("inf"))), dict(weight="1"),
                dict(weight=(1.0, "x")), dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=float("nan")),
                dict(alpha_min=None), dict(alpha_min=True)):
        with pytest.raises(ValueError):
            DepthConfig(**bad).validate()
    assert "tuned" in DepthConfig.__doc__


# ------------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(depth="expected"), dict(depth=True), dict(depth=1.0),
                                dict(depth="config:bad-mode"), dict(depth="config:bad-weight")])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(depth=DepthConfig(mode="expected"))
    args.update(kw)
    if args["depth"] == "config:bad-mode":
        args["depth"] = DepthConfig(mode="median")
    elif args["depth"] == "config:bad-weight":
        args["depth"] = DepthConfig(weight=(1.0, -1.0))
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_train_step_wants_a_depth_map_with_the_config_and_only_then():
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)         # (the checks come before anything else of the trainer is touched)
    tr.background = None
    tr.depth = None
    with pytest.raises(ValueError, match="targetDepth"):
        tr.trainStep(None, None, targetDepth=np.ones((2, 2), np.float32))
    with pytest.raises(ValueError, match="depthMask"):
        tr.trainStep(None, None, depthMask=np.ones((2, 2), np.uint8))
    tr.depth = DepthConfig()
    with pytest.raises(ValueError, match="targetDepth"):
        tr.trainStep(None, None)


# ------------------------------------------------------------------------------------------------------------- the loader
def _png16(path, values):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(values, np.uint16)).save(path)


def _colmap(root, names, W=8, H=6):
    from PIL import Image
    sparse, images = os.path.join(root, "sparse"), os.path.join(root, "images")
    os.makedirs(sparse, exist_ok=True)
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<Ii", 1, 1) + struct.pack("<QQ", W, H) + struct.pack("<dddd", 10, 10, 4, 3))
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(names)))
        for i, n in enumerate(names):
            f.write(struct.pack("<I", i + 1) + struct.pack("<dddd", 1, 0, 0, 0) + struct.pack("<ddd", 0, 0, 0) +
                    struct.pack("<I", 1) + n.encode() + b"\x00" + struct.pack("<Q", 0))
            os.makedirs(os.path.dirname(os.path.join(images, n)), exist_ok=True)
            Image.fromarray(np.full((H, W, 3), 40 * i, np.uint8)).save(os.path.join(images, n))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<QdddBBBdQ", 1, 0.0, 0.0, 0.0, 255, 0, 0, 0.0, 0))
    return sparse, images


def test_colmap_loader_reads_inverse_depth_priors(tmp_path):
    from gaussiansplattingmlx_amd.data import ColmapDataLoader, TrainData, readInverseDepth
    root = str(tmp_path / "colmap")
    sparse, images = _colmap(root, ["a.jpg.png", "b.png", "c.png"])
    droot = os.path.join(root, "depths")
    rng = np.random.default_rng(2)
    da, db = rng.integers(0, 65536, (6, 8)), rng.integers(256, 65536, (6, 8))        # (values that need all sixteen bits)
    da[0, :3] = 0                                                                      # holes
    _png16(os.path.join(droot, "a.jpg.png"), da)                                       # <image stem>.png: the stem of a.jpg.png is a.jpg
    _png16(os.path.join(droot, "b.png"), db)
    params = {"a.jpg": dict(scale=2.5, offset=-0.125, med_scale=9.0), "c": dict(scale=0.5, offset=0.25)}
    data, _, _ = ColmapDataLoader(sparse, images, depthRoot=droot, depthParams=params).load()
    assert data.depthArray.dtype == np.float32 and data.depthArray.shape == (3, 6, 8)
    assert np.array_equal(data.depthArray[0], da.astype(np.float32) / np.float32(65536.0))
    assert np.array_equal(data.depthArray[1], db.astype(np.float32) / np.float32(65536.0))
    assert float(data.depthArray.max()) < 1.0 and not data.depthArray[0, 0, :3].any()
    assert not data.depthArray[2].any()                                                 # c has no prior: all holes
    assert data.depthAlign.dtype == np.float32 and np.array_equal(data.depthAlign, np.asarray([[2.5, -0.125], [1, 0], [0.5, 0.25]], np.float32))
    # the params from a file; resized with the images, on the float values
    pj = os.path.join(root, "depth_params.json")
    json.dump(params, open(pj, "w"))
    half, _, _ = ColmapDataLoader(sparse, images, depthRoot=droot, depthParams=pj).load(resizeFactor=0.5)
    assert half.depthArray.shape == (3, 3, 4) == half.rgbArray.shape[:3] and np.array_equal(half.depthAlign, data.depthAlign)
    assert np.array_equal(half.depthArray[1], readInverseDepth(os.path.join(droot, "b.png"), 0.5))
    assert float(half.depthArray[1].min()) >= float(data.depthArray[1].min()) and float(half.depthArray[1].max()) <= float(data.depthArray[1].max())
    assert abs(float(half.depthArray[1].mean()) - float(data.depthArray[1].mean())) < 0.1
    # without a depthRoot nothing changes; without params every view is (1, 0)
    plain = ColmapDataLoader(sparse, images).load()[0]
    assert plain.depthArray is None and plain.depthAlign is None
    assert np.array_equal(ColmapDataLoader(sparse, images, depthRoot=droot).load()[0].depthAlign, np.tile(np.float32([1, 0]), (3, 1)))
    with pytest.raises(ValueError):
        ColmapDataLoader(sparse, images, depthParams=params)
    from PIL import Image
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(os.path.join(droot, "c.png"))     # not a depth map
    with pytest.raises(ValueError):
        ColmapDataLoader(sparse, images, depthRoot=droot).load()
    # the field is trailing and optional
    t = TrainData(data.Hs, data.Ws, data.intrinsicArray, data.c2wArray, data.rgbArray, data.alphaArray, None, None)
    assert t.depthAlign is None


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_and_binding_agree_on_the_new_entry_points():
    import ctypes as C
    from gaussiansplattingmlx_amd import _lib
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("gs_depth_loss", 9), ("gs_depth_normalize", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][1]) and _lib._SIGS[name][0] is C.c_int
    m = re.search(r"typedef struct gs_depth_loss_params\s*\{(.*?)\}", code, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+([a-z_, ]+);", m.group(1))
    declared = [(t, n.strip()) for t, names in fields for n in names.split(",")]
    assert declared == [("int", "mode"), ("float", "lambda"), ("float", "alpha_min"), ("float", "scale"), ("float", "offset")]
    bound = [(("int" if t is C.c_int else "float" if t is C.c_float else "?"), n.rstrip("_")) for n, t in _lib.gs_depth_loss_params._fields_]
    assert bound == declared and C.sizeof(_lib.gs_depth_loss_params) == 20
    assert re.search(r"GS_DEPTH_ACCUMULATED = 0, GS_DEPTH_EXPECTED = 1, GS_DEPTH_DISPARITY = 2", code)
    assert (_lib.GS_DEPTH_ACCUMULATED, _lib.GS_DEPTH_EXPECTED, _lib.GS_DEPTH_DISPARITY) == (0, 1, 2)
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import build
    assert "depth_loss.hip" in build.SOURCES


def test_library_exports_and_refuses_without_a_context():
    from gaussiansplattingmlx_amd import build
    build.build()
    from gaussiansplattingmlx_amd import _lib
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    p = _lib.gs_depth_loss_params(1, 1.0, 0.05, 1.0, 0.0)
    import ctypes as C
    assert _lib.STATUS.get(lib.gs_depth_loss(None, C.byref(p), None, None, None, None, None, None, None)) == "GS_ERR_INVALID_ARG"
    assert _lib.STATUS.get(lib.gs_depth_normalize(None, 4, None, None, C.c_float(0.05), None)) == "GS_ERR_INVALID_ARG"
    so = open(_lib.LIB_PATH, "rb").read()
    assert b"depth_loss_reduce_kernel" in so and b"depth_loss_cot_kernel" in so and b"depth_normalize_kernel" in so
