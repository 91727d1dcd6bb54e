"""Per-pixel loss masks without a GPU (include/gsplat.h gs_set_loss_mask): the ABI surface, the weight
rule (gaussiansplattingmlx_amd/loss_mask.py), the numpy mirror of the masked loss (tests/loss_mask_numpy.py) against the
oracle and against finite differences, and the loaders' mask files.

Finite differences.  The mirror's cotangent is checked against central differences of the mirror's own loss in float64
along eight random directions (unit max norm) at h = 1e-6, on test_gpu_exposure._images(37, 53) under three masks (random
binary, random soft, a zeroed rectangle inside tiles); bar 1e-4 relative to the analytic directional derivative.  Step-size
study on the float64 oracle alone, with this file's masks and directions (worst case over the three masks and eight
directions): h = 1e-3 5.7, h = 1e-4 0.81, h = 1e-5 4.0e-7, h = 1e-6 1.3e-6, h = 1e-7 8.6e-5 (the study that set the bar
measured 1.9e-6 at h = 1e-6 and 3e-7 at 1e-5 with other draws).  From h = 1e-4 up the L1 term's kinks (|wR - wG| at R = G)
take over, below 1e-6 the loss's rounding grows as 1 / h.  The bar sits some eighty times above the worst case at the step
used and far below any error of the chain rule itself: a missing factor w changes the derivative by O(1)."""
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FD_H, FD_BAR, FD_DIRECTIONS = 1e-6, 1e-4, 8


def _load(name):
    spec = importlib.util.spec_from_file_location("_lmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lmn = _load("loss_mask_numpy")


def _images(H, W):
    return _load("test_gpu_exposure")._images(H, W)[:2]


def _masks(H, W):
    rng = np.random.default_rng(7)
    rect = np.full((H, W), 255, np.uint8)
    rect[10:30, 20:45] = 0
    return dict(binary=(rng.uniform(size=(H, W)) > 0.5).astype(np.uint8) * np.uint8(255),
                soft=rng.integers(0, 256, (H, W)).astype(np.uint8), rect=rect)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_abi_version():
    from gaussiansplattingmlx_amd import _lib, build
    build.build()
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert re.search(r"int\s+gs_set_loss_mask\s*\(\s*gs_ctx\s*\*\s*ctx\s*,\s*const\s+unsigned\s+char\s*\*\s*mask", src)
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+6\b", src)
    assert "gs_set_loss_mask" in _lib.exported_symbols()
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    assert _lib.STATUS.get(lib.gs_set_loss_mask(None, None)) == "GS_ERR_INVALID_ARG"      # a NULL ctx


# ------------------------------------------------------------------------------------------------------------ the weights
def test_weights():
    from gaussiansplattingmlx_amd.loss_mask import validate, weights
    w = weights(np.arange(256, dtype=np.uint8).reshape(16, 16))
    assert w.dtype == np.float32 and w[0, 0] == 0.0 and w[15, 15] == 1.0
    assert np.array_equal(w.reshape(-1), (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32))   # correctly rounded
    assert (np.diff(w.reshape(-1)) > 0).all()
    b = np.array([[True, False], [False, True]])
    assert np.array_equal(weights(b), np.array([[1, 0], [0, 1]], np.float32))
    assert np.array_equal(weights(b), weights(b.astype(np.uint8) * np.uint8(255)))
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int8)):
        with pytest.raises(ValueError):
            weights(bad)
        with pytest.raises(ValueError):
            validate(bad, 4, 4)
    with pytest.raises(ValueError):
        weights(np.zeros((4, 4, 1), np.uint8))
    for shape in ((4, 5), (5, 4), (4, 4, 1), (16,)):
        with pytest.raises(ValueError):
            validate(np.zeros(shape, np.uint8), 4, 4)
    with pytest.raises(ValueError):
        validate([[255] * 4] * 4, 4, 4)                 # not an array
    validate(np.zeros((4, 6), np.uint8), 4, 6)
    validate(np.zeros((4, 6), bool), 4, 6)
    import torch
    validate(torch.zeros(4, 6, dtype=torch.uint8), 4, 6)
    validate(torch.zeros(4, 6, dtype=torch.bool), 4, 6)
    with pytest.raises(ValueError):
        validate(torch.zeros(4, 6), 4, 6)
    with pytest.raises(ValueError):
        validate(torch.zeros(6, 4, dtype=torch.uint8), 4, 6)


# ------------------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("which", ["oracle32", "oracle64"])
def test_mirror_all_255_is_the_plain_loss_and_all_0_is_nothing(request, which):
    o = request.getfixturevalue(which)
    H, W = 37, 53
    ren, tgt = _images(H, W)
    loss, cot, _, l1, ss = o.loss_forward_backward(ren, tgt, 0.2)
    got = lmn.masked_loss(o, ren, tgt, np.full((H, W), 255, np.uint8), 0.2)
    assert got[0] == loss and got[2] == l1 and got[3] == ss
    assert np.array_equal(got[1], cot)
    got = lmn.masked_loss(o, ren, tgt, np.ones((H, W), bool), 0.2)
    assert got[0] == loss and np.array_equal(got[1], cot)
    z = lmn.masked_loss(o, ren, tgt, np.zeros((H, W), np.uint8), 0.2)
    assert z[0] == 0.0 and z[2] == 0.0 and z[3] == 1.0          # L1 exactly 0, ssim exactly 1: it costs nothing ...
    assert not z[1].any()                                       # ... and pushes nothing


@pytest.mark.parametrize("mask", ["binary", "soft", "rect"])
def test_mirror_cotangent_against_finite_differences(oracle64, mask):
    H, W = 37, 53
    ren, tgt = _images(H, W)
    m = _masks(H, W)[mask]
    ren64 = ren.astype(np.float64)
    _, cot, _, _ = lmn.masked_loss(oracle64, ren64, tgt, m, 0.2)
    assert not cot[m == 0].any() and np.isfinite(cot).all()
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(FD_DIRECTIONS):
        d = rng.uniform(-1, 1, ren.shape)
        lp = lmn.masked_loss(oracle64, ren64 + FD_H * d, tgt, m, 0.2)[0]
        lm = lmn.masked_loss(oracle64, ren64 - FD_H * d, tgt, m, 0.2)[0]
        fd, an = (lp - lm) / (2 * FD_H), float((cot * d).sum())
        worst = max(worst, abs(fd - an) / abs(an))
    print(f"mask {mask}: worst relative deviation {worst:.3g}")
    assert worst <= FD_BAR, worst


# ------------------------------------------------------------------------------------------------------------ the loaders
def _png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _rgb(seed):
    return np.random.default_rng(seed).integers(0, 256, (6, 8, 3)).astype(np.uint8)       # 8 x 6 pixels


def _grey(seed):
    m = np.random.default_rng(100 + seed).integers(0, 256, (6, 8)).astype(np.uint8)
    m[0, 0], m[0, 1] = 0, 255
    return m


def _write_ply(path):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n0 0 0 255 0 0\n1 1 1 0 255 0\n")


def _nerfstudio(root, masks):
    """Three frames; masks: {frame index: grey image} written under masks/ and named by the frame's mask_path."""
    import json
    frames = []
    for i in range(3):
        _png(os.path.join(root, "images", f"f{i}.png"), _rgb(i))
        fr = dict(file_path=f"images/f{i}.png", transform_matrix=np.eye(4).tolist())
        if i in masks:
            _png(os.path.join(root, "masks", f"m{i}.png"), masks[i])
            fr["mask_path"] = f"masks/m{i}.png"
        frames.append(fr)
    _write_ply(os.path.join(root, "points.ply"))
    with open(os.path.join(root, "transforms.json"), "w") as f:
        json.dump(dict(fl_x=10.0, fl_y=10.0, cx=4.0, cy=3.0, ply_file_path="points.ply", frames=frames), f)


def test_nerfstudio_loader_reads_mask_path(tmp_path):
    from gaussiansplattingmlx_amd.data import NerfStudioDataLoader, TrainData, readMask
    root = str(tmp_path / "ns")
    masks = {0: _grey(0), 2: _grey(2)}
    _nerfstudio(root, masks)
    data, _, _ = NerfStudioDataLoader(root).load()
    assert data.maskArray.dtype == np.uint8 and data.maskArray.shape == (3, 6, 8)
    assert np.array_equal(data.maskArray[0], masks[0]) and np.array_equal(data.maskArray[2], masks[2])    # grey levels kept
    assert (data.maskArray[1] == 255).all()                                                              # a missing mask keeps all
    half, _, _ = NerfStudioDataLoader(root).load(resizeFactor=0.5)
    assert half.maskArray.shape == (3, 3, 4) == half.rgbArray.shape[:3]                                  # resized with the images
    assert np.array_equal(half.maskArray[0], readMask(os.path.join(root, "masks", "m0.png"), 0.5))
    assert (half.maskArray[1] == 255).all()
    from PIL import Image
    want = np.asarray(Image.fromarray(masks[0]).resize((4, 3), Image.BILINEAR))
    assert np.array_equal(half.maskArray[0], want)
    bare = str(tmp_path / "ns_bare")
    _nerfstudio(bare, {})
    assert NerfStudioDataLoader(bare).load()[0].maskArray is None
    # the field is trailing and optional: the positional constructions of before keep working
    t = TrainData(data.Hs, data.Ws, data.intrinsicArray, data.c2wArray, data.rgbArray, data.alphaArray, None)
    assert t.maskArray is None and TrainData(data.Hs, data.Ws, data.intrinsicArray, data.c2wArray, data.rgbArray,
                                             data.alphaArray).maskArray is None


def _colmap(root, names):
    import struct
    sparse, images = os.path.join(root, "sparse"), os.path.join(root, "images")
    os.makedirs(sparse, exist_ok=True)
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<Ii", 1, 1) + struct.pack("<QQ", 8, 6) + struct.pack("<dddd", 10, 10, 4, 3))
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(names)))
        for i, n in enumerate(names):
            f.write(struct.pack("<I", i + 1) + struct.pack("<dddd", 1, 0, 0, 0) + struct.pack("<ddd", 0, 0, 0) +
                    struct.pack("<I", 1) + n.encode() + b"\x00" + struct.pack("<Q", 0))
            _png(os.path.join(images, n), _rgb(i))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<QdddBBBdQ", 1, 0.0, 0.0, 0.0, 255, 0, 0, 0.0, 0))
    return sparse, images


def test_colmap_loader_finds_masks_by_both_naming_rules(tmp_path):
    from gaussiansplattingmlx_amd.data import ColmapDataLoader
    root = str(tmp_path / "colmap")
    sparse, images = _colmap(root, ["a.png", "b.png", "c.png", "d.png"])
    mroot = os.path.join(root, "masks")
    ma, mb, mc_full, mc_stem = _grey(0), _grey(1), _grey(2), _grey(3)
    _png(os.path.join(mroot, "a.png.png"), ma)          # COLMAP's own convention: <image file name>.png
    _png(os.path.join(mroot, "b.png"), mb)              # <stem>.png
    _png(os.path.join(mroot, "c.png.png"), mc_full)     # both exist: the full name wins
    _png(os.path.join(mroot, "c.png"), mc_stem)
    data, _, _ = ColmapDataLoader(sparse, images, maskRoot=mroot).load()
    assert data.maskArray.dtype == np.uint8 and data.maskArray.shape == (4, 6, 8)
    assert np.array_equal(data.maskArray[0], ma) and np.array_equal(data.maskArray[1], mb)
    assert np.array_equal(data.maskArray[2], mc_full)
    assert (data.maskArray[3] == 255).all()             # d has no mask
    half, _, _ = ColmapDataLoader(sparse, images, maskRoot=mroot).load(resizeFactor=0.5)
    assert half.maskArray.shape == (4, 3, 4) == half.rgbArray.shape[:3]
    from PIL import Image
    assert np.array_equal(half.maskArray[1], np.asarray(Image.fromarray(mb).resize((4, 3), Image.BILINEAR)))
    assert ColmapDataLoader(sparse, images).load()[0].maskArray is None                  # no maskRoot
    empty = os.path.join(root, "no_masks")
    os.makedirs(empty)
    assert ColmapDataLoader(sparse, images, maskRoot=empty).load()[0].maskArray is None  # a root without any mask
