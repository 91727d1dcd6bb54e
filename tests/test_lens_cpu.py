"""Lens undistortion on the CPU (gaussiansplattingmlx_amd/lens.py, include/gsplat.h gs_undistort): the
model against hand-computed values, the resampling against an affine image (which bilinear interpolation reproduces exactly),
validity, the hole-aware depth mode, the mask's rounding, and the loaders' camera-model tables and undistort=True pass
(data.py), with the files written here as test_loaders.py does."""
import json
import struct

import numpy as np
import pytest

from gaussiansplattingmlx_amd import data as D
from gaussiansplattingmlx_amd import lens as L


# --------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("coeff,xd,yd", [(dict(k1=0.1), 0.515625, 0.2578125), (dict(k2=0.2), 0.509765625, 0.2548828125),
                                         (dict(p1=0.01), 0.5025, 0.254375), (dict(p2=0.02), 0.51625, 0.255)])
def test_distort_matches_hand_computed_values(coeff, xd, yd):
    """(x, y) = (0.5, 0.25): r2 = 0.3125, r4 = 0.09765625.  k1: radial 1.03125.  k2: radial 1.01953125.  p1: xd = x + 2 p1 x y,
    yd = y + p1 (r2 + 2 y^2) = 0.25 + 0.01 x 0.4375.  p2: xd = x + p2 (r2 + 2 x^2) = 0.5 + 0.02 x 0.8125, yd = y + 2 p2 x y."""
    lens = L.LensModel(100.0, 100.0, 50.0, 50.0, **coeff)
    got = lens.distort(0.5, 0.25)
    np.testing.assert_allclose(got, (xd, yd), rtol=1e-15)
    got32 = lens.distort(np.float32(0.5), np.float32(0.25), np.float32)
    assert got32[0].dtype == np.float32 and got32[1].dtype == np.float32
    np.testing.assert_allclose(got32, (xd, yd), rtol=4 * 2.0 ** -24)
    assert not lens.is_pinhole and L.LensModel(1.0, 1.0, 0.0, 0.0).is_pinhole


def test_an_affine_image_is_resampled_exactly():
    """S(u, v) = a u + b v + c at the pixel centres (u, v) = (x + 0.5, y + 0.5): bilinear interpolation reproduces an affine
    function, so every valid pixel holds a u(i, j) + b v(i, j) + c with (u, v) the distorted position of (i, j)."""
    sw, sh, a, b, c = 67, 45, 0.5, -0.25, 3.0
    xs, ys = np.meshgrid(np.arange(sw) + 0.5, np.arange(sh) + 0.5, indexing="xy")
    S = (a * xs + b * ys + c).astype(np.float32)            # (dyadic coefficients: exact in float32)
    lens = L.LensModel(60.0, 58.0, 35.25, 21.5, k1=0.12, k2=-0.03, p1=0.004, p2=-0.006)
    for dstK, size in ((None, None), ((40.0, 41.0, 30.0, 20.0), (50, 38))):
        w, h = (sw, sh) if size is None else size
        su, sv, _ = L.source_coords(lens, lens.K if dstK is None else dstK, w, h)
        want = a * (su + 0.5) + b * (sv + 0.5) + c
        for img in (S, np.stack([S, 2 * S, -S], -1)):
            got, valid = L.remap_values(img, lens, dstK, size)
            assert 0.3 < valid.mean() < 1.0 and got.shape == (h, w) + img.shape[2:]
            g = got if got.ndim == 2 else got[..., 1] / 2
            np.testing.assert_allclose(g[valid], want[valid], rtol=1e-13)
        out, v8 = L.undistort_image(S, lens, dstK, size)
        assert out.dtype == np.float32 and out.shape == (h, w) and v8.dtype == np.uint8 and v8.shape == (h, w)
        np.testing.assert_array_equal(v8 == 255, valid)
        np.testing.assert_allclose(out[valid], want[valid], rtol=2.0 ** -23)


def test_validity_taps_and_the_fold_back_guard():
    """k1 = -0.35, a 64 x 48 source of focal 60 seen by a destination of focal 20 (three times the source's field of view).
    r radial(r) peaks at r^2 = 1 / 1.05: beyond it the radial map folds back and far destination pixels land INSIDE the source
    again -- only the guard 1 + 3 k1 r^2 > 0 keeps them out.  Short of the fold, the destination's border samples outside the
    source and is invalid by its taps."""
    sw, sh = 64, 48
    rng = np.random.default_rng(0)
    S = rng.uniform(0.5, 1.0, (sh, sw, 3)).astype(np.float32)
    lens, dstK = L.LensModel(60.0, 60.0, 32.0, 24.0, k1=-0.35), (20.0, 20.0, 32.0, 24.0)
    su, sv, fold = L.source_coords(lens, dstK, sw, sh)
    inside = (np.floor(su) >= 0) & (np.floor(su) + 1 <= sw - 1) & (np.floor(sv) >= 0) & (np.floor(sv) + 1 <= sh - 1)
    out, valid = L.undistort_image(S, lens, dstK)
    assert set(np.unique(valid)) == {0, 255}
    np.testing.assert_array_equal(valid == 255, inside & (fold > 0))
    folded = inside & (fold <= 0)
    assert folded.sum() >= 20 and not valid[folded].any()            # the guard fires, and nothing else excludes these
    assert folded[24, 60] and folded[24, 3]
    outside = ~inside & (fold > 0)
    assert outside.sum() >= 20 and not valid[outside].any()          # the barrel border: taps outside the source
    assert valid[24, 32] == 255 and (valid[0] == 0).all() and (valid[:, 0] == 0).all()
    assert not out[valid == 0].any() and (out[valid == 255] >= 0.5 - 1e-6).all()
    # the same K on both sides: a barrel lens pulls every sample inwards, the whole view is valid up to the fold
    _, same = L.undistort_image(S, lens)
    assert (same == 255).all()
    # a pincushion lens pushes samples outwards: the border is empty
    _, pin = L.undistort_image(S, L.LensModel(60.0, 60.0, 32.0, 24.0, k1=0.2))
    assert pin[24, 32] == 255 and not pin[0].any() and not pin[:, -1].any()
    # a one-pixel source has no four taps anywhere
    assert not L.undistort_image(S[:1, :1], L.LensModel(60.0, 60.0, 0.5, 0.5))[1].any()


def _shift_lens(dx, dy, cx=2.0, cy=2.0):
    """A pinhole pair whose sample positions are (i + dx, j + dy): focal 8 (a power of two: every step is exact)."""
    return L.LensModel(8.0, 8.0, cx, cy), (8.0, 8.0, cx - dx, cy - dy)


def test_depth_mode_never_averages_a_hole_into_a_depth():
    lens, dstK = _shift_lens(0.3, 0.6)
    S = np.zeros((5, 5), np.float32)
    S[2, 2] = 7.5
    out, valid = L.undistort_image(S, lens, dstK, mode="depth")
    assert (valid[:4, :4] == 255).all() and not valid[4].any() and not valid[:, 4].any()
    want = np.zeros((5, 5), np.float32)
    want[1:3, 1:3] = 7.5            # the four cells that have the live pixel among their taps: one live tap, that tap
    np.testing.assert_allclose(out, want, rtol=1e-7)
    # colour mode on the same image shows what a plain bilinear blend would have done
    plain, _ = L.undistort_image(S, lens, dstK, mode="color")
    np.testing.assert_allclose(plain[1, 1], 7.5 * 0.3 * 0.6, rtol=1e-6)
    # two live taps: their weights renormalised
    S[2, 3] = 2.5
    out, _ = L.undistort_image(S, lens, dstK, mode="depth")
    np.testing.assert_allclose(out[2, 2], 0.7 * 7.5 + 0.3 * 2.5, rtol=1e-6)
    np.testing.assert_allclose(out[1, 2], 0.7 * 7.5 + 0.3 * 2.5, rtol=1e-6)
    assert out[0, 0] == 0 and out[3, 3] == 0


def test_mask_mode_rounds_half_up():
    lens, dstK = _shift_lens(0.5, 0.0)
    S = np.array([[0, 1, 2, 3, 10]] * 3, np.uint8)
    out, valid = L.undistort_image(S, lens, dstK, mode="mask")
    assert out.dtype == np.uint8
    # 0.5 -> 1, 1.5 -> 2, 2.5 -> 3 (round-half-even would give 0, 2, 2), 6.5 -> 7; the last column and row have no taps
    np.testing.assert_array_equal(out[:2, :4], [[1, 2, 3, 7]] * 2)
    assert (valid[:2, :4] == 255).all() and not valid[2].any() and not valid[:, 4].any() and not out[2].any()
    value, _ = L.remap_values(S, lens, dstK, mode="mask")
    np.testing.assert_array_equal(value[:2, :4], [[0.5, 1.5, 2.5, 6.5]] * 2)
    with pytest.raises(ValueError):
        L.undistort_image(S.astype(np.float32), lens, dstK, mode="mask")
    with pytest.raises(ValueError):
        L.undistort_image(S, lens, dstK, mode="nearest")


def test_float32_evaluation_stays_inside_the_derived_bar():
    """remap_bar against the module's own float32 evaluation (the kernel's arithmetic, operation for operation)."""
    rng = np.random.default_rng(5)
    S = rng.uniform(0, 1, (45, 67, 3)).astype(np.float32)
    lens = L.LensModel(60.0, 58.0, 35.25, 21.5, k1=-0.2, k2=0.05, p1=0.003, p2=-0.002).as_float32()
    v64, ok64 = L.remap_values(S, lens)
    v32, ok32 = L.remap_values(S, lens, dtype=np.float32)
    assert v32.dtype == np.float32
    bar = L.remap_bar(S, lens)
    both = ok64 & ok32
    assert both.mean() > 0.5 and (ok64 != ok32).mean() <= 0.01
    err = np.abs(v32.astype(np.float64) - v64)
    print(f"float32 evaluation: max err / bar = {(err[both] / bar[both]).max():.3f}, max err {err[both].max():.2e}")
    # (the bar itself stays small: delta is 23 x 2^-24 x ~100 px = 1.4e-4 px, the noise's slopes are below 2 per pixel)
    assert np.all(err[both] <= bar[both]) and bar[both].max() < 3e-4 and not bar[~ok64].any()


# --------------------------------------------------------------------------------------------------------------- the loaders
def _write_colmap(root, cams, images):
    with open(root / "cameras.bin", "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, model, w, h, params in cams:
            f.write(struct.pack("<IiQQ", cid, model, w, h) + struct.pack("<%dd" % len(params), *params))
    with open(root / "images.bin", "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name in images:
            f.write(struct.pack("<I4d3dI", iid, *q, *t, cid) + name.encode() + b"\x00" + struct.pack("<Q", 0))
    with open(root / "points3D.bin", "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<Q3d3BdQ", 7, 0.1, 0.2, 0.3, 255, 128, 0, 0.5, 0))


def test_colmap_own_model_table_keeps_the_file_in_step(tmp_path):
    cams = [(1, 0, 640, 480, (450.0, 320.0, 240.0)), (2, 1, 800, 600, (500.0, 510.0, 400.0, 300.0)),
            (3, 2, 640, 480, (451.0, 321.0, 241.0, 0.01)), (4, 3, 640, 480, (452.0, 322.0, 242.0, 0.02, -0.03)),
            (5, 4, 64, 48, (50.0, 51.0, 32.0, 24.0, 0.1, 0.2, 0.3, 0.4)),
            (6, 5, 64, 48, (40.0, 41.0, 31.0, 23.0, 0.5, 0.6, 0.7, 0.8)), (7, 1, 32, 24, (20.0, 21.0, 16.0, 12.0))]
    _write_colmap(tmp_path, cams, [(10, (1.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 7, "a.png")])
    C = D.ColmapCamera
    camMap, poses = D.colmapReadCamerasAndPoses(str(tmp_path), "/img", cameraModels="colmap")
    assert camMap[1] == C(1, 640, 480, 450.0, 450.0, 320.0, 240.0, None, None, None, None, "SIMPLE_PINHOLE")
    assert camMap[2] == C(2, 800, 600, 500.0, 510.0, 400.0, 300.0, None, None, None, None, "PINHOLE")
    assert camMap[3] == C(3, 640, 480, 451.0, 451.0, 321.0, 241.0, 0.01, None, None, None, "SIMPLE_RADIAL")
    assert camMap[4] == C(4, 640, 480, 452.0, 452.0, 322.0, 242.0, 0.02, -0.03, None, None, "RADIAL")
    assert camMap[5] == C(5, 64, 48, 50.0, 51.0, 32.0, 24.0, 0.1, 0.2, 0.3, 0.4, "OPENCV")
    assert camMap[6] == C(6, 64, 48, 40.0, 41.0, 31.0, 23.0, None, None, None, None, "OPENCV_FISHEYE")
    assert camMap[7] == C(7, 32, 24, 20.0, 21.0, 16.0, 12.0, None, None, None, None, "PINHOLE")      # intact after the fisheye one
    assert poses[0].cameraId == 7
    # the default is the reference app's table: id 3 is 8 doubles, so THIS file goes out of step there (RADIAL has 5) ...
    ref, _ = D.colmapReadCamerasAndPoses(str(tmp_path), "/img")
    assert ref[4].fy == 322.0 and ref[4].k1 == -0.03
    # ... and a file written for it reads as before
    _write_colmap(tmp_path, [(4, 3, 64, 48, (50.0, 51.0, 32.0, 24.0, .1, .2, .3, .4)), (9, 1, 8, 6, (5.0, 6.0, 4.0, 3.0))],
                  [(10, (1.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 9, "a.png")])
    ref, _ = D.colmapReadCamerasAndPoses(str(tmp_path), "/img")
    assert ref[4][:11] == (4, 64, 48, 50.0, 51.0, 32.0, 24.0, .1, .2, .3, .4) and ref[9].fy == 6.0
    assert D.ColmapDataLoader(str(tmp_path), "/img").cameraModels == "reference"
    # an unknown id raises under COLMAP's table
    _write_colmap(tmp_path, [(1, 11, 8, 6, (5.0, 6.0, 4.0, 3.0))], [(10, (1.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 1, "a.png")])
    with pytest.raises(ValueError, match="unknown model"):
        D.colmapReadCamerasAndPoses(str(tmp_path), "/img", cameraModels="colmap")
    with pytest.raises(ValueError):
        D.ColmapDataLoader(str(tmp_path), "/img", cameraModels="opencv")


SRC_W, SRC_H = 96, 64
OPENCV = (88.0, 86.0, 50.5, 30.25, 0.18, -0.04, 0.003, -0.002)        # (pincushion: the undistorted view's border is empty)


def two_view_set(root, seed=0):
    """A COLMAP set of two 96 x 64 RGBA views, the first a PINHOLE camera and the second OPENCV, with a loss mask for the second
    and Inria-style depth priors (about 20 % holes) for both.  Returns the loader's keyword arguments."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    (root / "sparse").mkdir(); (root / "images").mkdir(); (root / "masks").mkdir(); (root / "depths").mkdir()
    cams = [(1, 1, SRC_W, SRC_H, (90.0, 91.0, 47.0, 33.0)), (2, 4, SRC_W, SRC_H, OPENCV)]
    _write_colmap(root / "sparse", cams, [(10, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 3.0), 1, "a.png"),
                                          (11, (1.0, 0.0, 0.0, 0.0), (0.5, 0.0, 3.0), 2, "b.png")])
    for name in ("a", "b"):
        Image.fromarray(rng.integers(0, 256, (SRC_H, SRC_W, 4), dtype=np.uint8), "RGBA").save(root / "images" / f"{name}.png")
        d = rng.integers(1, 65536, (SRC_H, SRC_W)).astype(np.uint16)
        d[rng.uniform(size=d.shape) < 0.2] = 0
        Image.fromarray(d).save(root / "depths" / f"{name}.png")
    Image.fromarray(rng.integers(0, 256, (SRC_H, SRC_W), dtype=np.uint8)).save(root / "masks" / "b.png")
    return dict(binRoot=str(root / "sparse"), imageRoot=str(root / "images"), cameraModels="colmap")


@pytest.mark.parametrize("resize", [1.0, 0.5])
def test_colmap_undistort_resamples_only_the_distorted_view_after_the_resize(tmp_path, resize):
    kw = two_view_set(tmp_path)
    plain, _, _ = D.ColmapDataLoader(**kw).load(resize)
    assert plain.maskArray is None and plain.depthArray is None
    und, _, tile = D.ColmapDataLoader(**kw, undistort=True).load(resize)
    h, w = int(SRC_H * resize), int(SRC_W * resize)
    assert und.rgbArray.shape == (2, h, w, 3) and tile == D.TILE_SIZE_H_W(w=w // 4, h=h // 4)
    np.testing.assert_array_equal(und.intrinsicArray, plain.intrinsicArray)              # K is kept, and scaled
    np.testing.assert_array_equal(und.rgbArray[0], plain.rgbArray[0])                     # the pinhole view: not resampled at all
    np.testing.assert_array_equal(und.alphaArray[0], plain.alphaArray[0])
    assert und.maskArray is not None and und.maskArray.dtype == np.uint8 and (und.maskArray[0] == 255).all()
    # the second view by hand: the RESIZED image through the lens of the SCALED K, RGBA in one four-channel call
    K = plain.intrinsicArray[1]
    lens = L.LensModel(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *OPENCV[4:])
    assert lens.K == tuple(float(np.float32(v) * np.float32(resize)) for v in OPENCV[:4])
    rgba = np.concatenate([plain.rgbArray[1], plain.alphaArray[1][..., None]], -1)
    want, valid = L.undistort_image(rgba, lens)
    assert 0.5 < (valid == 255).mean() < 1.0
    np.testing.assert_array_equal(und.rgbArray[1], want[..., :3])
    np.testing.assert_array_equal(und.alphaArray[1], want[..., 3])
    np.testing.assert_array_equal(und.maskArray[1], valid)
    assert not np.array_equal(und.rgbArray[1], plain.rgbArray[1])
    # (remapping first and resizing after is something else: the order is part of the result)
    if resize != 1.0:
        full, _, _ = D.ColmapDataLoader(**kw).load(1.0)
        lens1 = L.LensModel(*OPENCV)
        first = L.undistort_image(np.concatenate([full.rgbArray[1], full.alphaArray[1][..., None]], -1), lens1)[0]
        assert not np.allclose(first[::2, ::2, :3], und.rgbArray[1], atol=1e-3)

    # with a mask and depth priors: the mask in mask mode under the validity, the depth in depth mode
    kw2 = dict(kw, maskRoot=str(tmp_path / "masks"), depthRoot=str(tmp_path / "depths"))
    plain2, _, _ = D.ColmapDataLoader(**kw2).load(resize)
    und2, _, _ = D.ColmapDataLoader(**kw2, undistort=True).load(resize)
    np.testing.assert_array_equal(und2.maskArray[0], plain2.maskArray[0])
    np.testing.assert_array_equal(und2.depthArray[0], plain2.depthArray[0])
    np.testing.assert_array_equal(und2.maskArray[1], np.minimum(L.undistort_image(plain2.maskArray[1], lens, mode="mask")[0], valid))
    np.testing.assert_array_equal(und2.depthArray[1], L.undistort_image(plain2.depthArray[1], lens, mode="depth")[0])
    np.testing.assert_array_equal(und2.depthAlign, plain2.depthAlign)
    live = und2.depthArray[1][valid == 255]
    assert (live > 0).mean() > 0.9          # holes do not spread: a result is a hole only where all four taps are

    # an undistorter of the caller's is what resamples: here one that records its calls
    calls = []

    def spy(img, lens, dstK=None, dstSize=None, mode="color"):
        calls.append((mode, np.asarray(img).shape, lens.coefficients))
        return L.undistort_image(img, lens, dstK, dstSize, mode)
    und3, _, _ = D.ColmapDataLoader(**kw2, undistort=True).load(resize, undistorter=spy)
    assert calls == [("color", (h, w, 4), OPENCV[4:]), ("mask", (h, w), OPENCV[4:]), ("depth", (h, w), OPENCV[4:])]
    np.testing.assert_array_equal(und3.rgbArray, und2.rgbArray)


def test_a_fisheye_camera_raises_only_under_undistort(tmp_path):
    kw = two_view_set(tmp_path)
    cams = [(1, 1, SRC_W, SRC_H, (90.0, 91.0, 47.0, 33.0)), (2, 5, SRC_W, SRC_H, (88.0, 86.0, 50.5, 30.25, 0.1, 0.0, 0.0, 0.0))]
    _write_colmap(tmp_path / "sparse", cams, [(10, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 3.0), 1, "a.png"),
                                              (11, (1.0, 0.0, 0.0, 0.0), (0.5, 0.0, 3.0), 2, "b.png")])
    td, _, _ = D.ColmapDataLoader(**kw).load()
    np.testing.assert_array_equal(td.intrinsicArray[1], [[88.0, 0, 50.5], [0, 86.0, 30.25], [0, 0, 1]])
    assert td.maskArray is None
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        D.ColmapDataLoader(**kw, undistort=True).load()


def test_nerfstudio_takes_the_coefficients_from_the_frame_first_and_the_header_second(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    w, h = 48, 32
    for name in ("f0", "f1", "f2"):
        Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA").save(tmp_path / f"{name}.png")
    (tmp_path / "pts.ply").write_text("ply\nformat ascii 1.0\nelement vertex 1\nend_header\n0.0 0.0 0.0 1 2 3\n")
    eye = np.eye(4).tolist()
    frames = [dict(file_path="f0.png", transform_matrix=eye),                                        # the header's coefficients
              dict(file_path="f1.png", transform_matrix=eye, k1=0.2, p2=0.01),                      # its own: k2 = p1 = 0
              dict(file_path="f2.png", transform_matrix=eye, k1=0.0, k2=0.0, p1=0.0, p2=0.0)]       # its own: a pinhole
    meta = dict(fl_x=44.0, fl_y=43.0, cx=25.5, cy=15.0, k1=-0.1, k2=0.02, p1=0.001, p2=0.0, camera_model="OPENCV",
                ply_file_path="pts.ply", frames=frames)
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    plain, _, _ = D.NerfStudioDataLoader(str(tmp_path)).load()
    und, _, _ = D.NerfStudioDataLoader(str(tmp_path), undistort=True).load()
    assert plain.maskArray is None and und.maskArray.shape == (3, h, w)
    for i, coeff in enumerate([(-0.1, 0.02, 0.001, 0.0), (0.2, 0.0, 0.0, 0.01)]):
        rgba = np.concatenate([plain.rgbArray[i], plain.alphaArray[i][..., None]], -1)
        want, valid = L.undistort_image(rgba, L.LensModel(44.0, 43.0, 25.5, 15.0, *coeff))
        np.testing.assert_array_equal(und.rgbArray[i], want[..., :3])
        np.testing.assert_array_equal(und.maskArray[i], valid)
    np.testing.assert_array_equal(und.rgbArray[2], plain.rgbArray[2])
    assert (und.maskArray[2] == 255).all()
    np.testing.assert_array_equal(und.intrinsicArray, plain.intrinsicArray)
    meta["camera_model"] = "OPENCV_FISHEYE"
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    D.NerfStudioDataLoader(str(tmp_path)).load()
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        D.NerfStudioDataLoader(str(tmp_path), undistort=True).load()
