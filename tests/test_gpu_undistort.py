"""The undistortion kernel (csrc/lens.hip, include/gsplat.h gs_undistort) against the float64 statement in lens.py, within
lens.remap_bar -- a bound derived by counting float32 roundings, no constant of which is fitted to the kernel's output -- and
the loaders' undistort=True pass through the kernel against the same pass on the host.

The comparison's rules (`_compare`), applied alike to the kernel and, on the CPU, to lens.py's own float32 evaluation:
  * values are compared on the pixels both sides call valid, each within its bar;
  * validity flags must agree, except where a float64 tap coordinate is within delta (lens.coord_delta) of the source's border
    or the fold-back expression is within its rounding of 0;
  * a mask may differ by one level, and only where the float64 value is within the bar of a .5 boundary;
  * each exception set is counted and capped at 1 % of the pixels: a condition of the test, not a measurement.  The CPU test
    below holds the seeds to it with the float64 and float32 host evaluations alone.
Sources are uniform noise: [0, 1] colours, levels 0 .. 255 for a mask, depths in [0.5, 5] with about 20 % holes.  Lens
parameters are float32 numbers (LensModel.as_float32): both sides are handed the same inputs."""
import importlib.util
import os

import numpy as np
import pytest

from gaussiansplattingmlx_amd import data as D
from gaussiansplattingmlx_amd import lens as L

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 0.01

SIMPLE_RADIAL = dict(k1=0.11)
RADIAL = dict(k1=-0.21, k2=0.05)
OPENCV_NEG = dict(k1=-0.17, k2=0.03, p1=0.004, p2=-0.003)
OPENCV_POS = dict(k1=0.14, k2=-0.02, p1=-0.002, p2=0.005)
K_SRC = (60.0, 58.0, 35.25, 21.5)                # of the 67 x 45 source: neither side is a multiple of the 64 x 4 block

# id: (source (w, h), channels (0: a [H, W] image), coefficients, dstK, dstSize, mode, seed)
CASES = {
    "67x45_c3_opencv_neg": ((67, 45), 3, OPENCV_NEG, None, None, "color", 1),
    "67x45_c3_opencv_pos": ((67, 45), 3, OPENCV_POS, None, None, "color", 2),
    "64x4_c1_simple_radial": ((67, 45), 1, SIMPLE_RADIAL, (60.0, 58.0, 32.0, 2.0), (64, 4), "color", 3),
    "1x1_c4_radial": ((67, 45), 4, RADIAL, (60.0, 58.0, 0.5, 0.5), (1, 1), "color", 4),
    "80x50_c4_opencv_pos": ((67, 45), 4, OPENCV_POS, (52.0, 50.5, 41.0, 24.75), (80, 50), "color", 5),
    "203x131_c4_radial": ((211, 140), 4, RADIAL, (150.0, 151.0, 100.5, 66.25), (203, 131), "color", 6),
    "67x45_2d_simple_radial": ((67, 45), 0, SIMPLE_RADIAL, None, None, "color", 7),
    "67x45_mask_opencv_neg": ((67, 45), 0, OPENCV_NEG, None, None, "mask", 8),
    "130x70_mask_opencv_pos": ((120, 66), 0, OPENCV_POS, (100.0, 99.0, 66.5, 34.0), (130, 70), "mask", 9),
    "67x45_depth_radial": ((67, 45), 0, RADIAL, None, None, "depth", 10),
    "90x61_depth_opencv_pos": ((67, 45), 0, OPENCV_POS, (70.0, 69.0, 45.0, 30.5), (90, 61), "depth", 11),
}
_cache = {}


def _load(name):
    spec = importlib.util.spec_from_file_location("_und_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(cid):
    """(image, lens, dstK, dstSize, mode, reference) -- the float64 statement computed once per case and left unchanged."""
    if cid in _cache:
        return _cache[cid]
    (sw, sh), ch, coeff, dstK, dstSize, mode, seed = CASES[cid]
    rng = np.random.default_rng(seed)
    shape = (sh, sw) if ch == 0 else (sh, sw, ch)
    if mode == "mask":
        img = rng.integers(0, 256, shape, dtype=np.uint8)
    elif mode == "depth":
        img = rng.uniform(0.5, 5.0, shape).astype(np.float32)
        img[rng.uniform(size=shape) < 0.2] = 0.0
    else:
        img = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    K = K_SRC if (sw, sh) == (67, 45) else (0.9 * sw, 0.91 * sw, 0.5 * sw + 3.25, 0.5 * sh - 2.5)
    lens = L.LensModel(*K, **coeff).as_float32()
    k, w, h = L._dst(lens, dstK, dstSize, img.shape)
    value, valid = L.remap_values(img, lens, dstK, dstSize, mode)
    su, sv, fold = L.source_coords(lens, k, w, h)
    delta, fdelta = L.coord_delta(lens, k, w, h)
    near = (np.minimum(np.abs(su), np.abs(su - (sw - 1))) <= delta) | (np.minimum(np.abs(sv), np.abs(sv - (sh - 1))) <= delta) \
        | (np.abs(fold) <= fdelta)
    ref = dict(value=value, valid=valid, bar=L.remap_bar(img, lens, dstK, dstSize, mode), near=near, size=(w, h))
    _cache[cid] = (img, lens, dstK, dstSize, mode, ref)
    return _cache[cid]


def _compare(cid, out, valid8, what):
    img, lens, dstK, dstSize, mode, ref = _case(cid)
    w, h = ref["size"]
    out, npix = np.asarray(out), w * h
    assert out.shape == ref["value"].shape and out.dtype == (np.uint8 if mode == "mask" else np.float32)
    valid8 = np.asarray(valid8)
    assert valid8.shape == (h, w) and valid8.dtype == np.uint8 and set(np.unique(valid8)) <= {0, 255}
    ok = valid8 == 255
    differ = ok != ref["valid"]
    assert not (differ & ~ref["near"]).any(), f"{what} {cid}: validity differs away from the border and the fold"
    flips = int(differ.sum())
    assert flips <= CAP * npix, (cid, flips)
    assert not out[~ok].any(), f"{what} {cid}: an invalid pixel is not 0"
    both = ok & ref["valid"]
    v64, bar = ref["value"], ref["bar"]
    if mode == "mask":
        want = np.floor(v64 + 0.5)
        d = np.abs(out.astype(np.float64) - want)
        frac = v64 - np.floor(v64)
        excused = np.abs(frac - 0.5) <= bar
        bad = both & (d > 0) & ~((d == 1) & excused)
        assert not bad.any(), f"{what} {cid}: {int(bad.sum())} mask levels differ away from a .5 boundary"
        levels = int((both & (d > 0)).sum())
        assert levels <= CAP * npix, (cid, levels)
        print(f"{what} {cid}: {int(both.sum())} of {npix} valid, {flips} validity flips, {levels} levels off by one (cap {CAP * npix:.1f})")
        return
    err = np.abs(out.astype(np.float64) - v64)
    sel = both if err.ndim == 2 else np.broadcast_to(both[..., None], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(err[sel] > 0, err[sel] / bar[sel], 0.0).max()) if sel.any() else 0.0
    print(f"{what} {cid}: {int(both.sum())} of {npix} valid, {flips} validity flips, max err / bar = {ratio:.3f}, "
          f"max err {float(err[sel].max()) if sel.any() else 0.0:.2e}")
    assert np.all(err[sel] <= bar[sel]), f"{what} {cid}: max err / bar = {ratio:.3f}"


@pytest.mark.parametrize("cid", sorted(CASES))
def test_the_cases_hold_their_conditions_on_the_host(cid):
    """The seeds' condition, on the CPU: lens.py's float32 evaluation (the kernel's arithmetic, operation for operation)
    against its float64 one stays inside the bar and inside the 1 % caps; and the cases cover what they are meant to."""
    img, lens, dstK, dstSize, mode, ref = _case(cid)
    out, valid = L.undistort_image(img, lens, dstK, dstSize, mode, dtype=np.float32)
    _compare(cid, out, valid, "float32 host")
    share = ref["valid"].mean()
    if ref["size"] != (1, 1):
        assert 0.3 < share <= 1.0
    if mode == "depth":
        assert 0.15 < (img == 0).mean() < 0.25 and (ref["value"][ref["valid"]] > 0).mean() > 0.9


def test_the_cases_cover_both_signs_and_an_empty_border():
    signs = {np.sign(CASES[c][2]["k1"]) for c in CASES}
    assert signs == {-1.0, 1.0}
    assert any(not _case(c)[5]["valid"].all() for c in CASES) and _case("1x1_c4_radial")[5]["valid"].all()


def _renderer():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(0, 32, 32, (16, 16), False)         # (the entry point is independent of the context's W, H)


@pytest.fixture(scope="module")
def renderer():
    r = _renderer()
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_kernel_matches_the_float64_statement(renderer, cid):
    img, lens, dstK, dstSize, mode, ref = _case(cid)
    out, valid = renderer.undistortImage(img, lens, dstK, dstSize, mode)
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    _compare(cid, out, valid, "kernel")
    # valid = NULL: the same image
    out2, none = renderer.undistortImage(img, lens, dstK, dstSize, mode, wantValid=False)
    assert none is None
    np.testing.assert_array_equal(out2.cpu().numpy(), out)


@pytest.mark.gpu
def test_argument_errors(renderer):
    import ctypes as C
    import torch
    from gaussiansplattingmlx_amd import _lib
    lib, ctx, INVALID = renderer.lib, renderer.ctx, 1
    src = torch.zeros(8 * 8 * 4, device="cuda")
    dst = torch.zeros(8 * 8 * 4, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = _lib.gs_lens(10.0, 10.0, 4.0, 4.0, 0.1, 0.0, 0.0, 0.0, 10.0, 10.0, 4.0, 4.0)
    call = lambda lens, sw=8, sh=8, dw=8, dh=8, ch=1, mode=0: lib.gs_undistort(ctx, C.byref(lens), sw, sh, dw, dh, ch, mode, p(src), p(dst), None)      # noqa: E731
    assert call(good) == 0 and call(good, ch=4) == 0 and call(good, mode=2) == 0
    for kw in (dict(ch=0), dict(ch=5), dict(ch=3, mode=1), dict(ch=2, mode=2), dict(mode=3), dict(mode=-1), dict(sw=0), dict(dh=0),
               dict(dw=-1)):
        assert call(good, **kw) == INVALID, kw
        assert b"gs_undistort" in lib.gs_last_error(ctx)
    for field, v in (("fx", 0.0), ("fy", -1.0), ("dst_fx", 0.0), ("dst_fy", float("nan")), ("k1", float("inf"))):
        bad = _lib.gs_lens(10.0, 10.0, 4.0, 4.0, 0.1, 0.0, 0.0, 0.0, 10.0, 10.0, 4.0, 4.0)
        setattr(bad, field, v)
        assert call(bad) == INVALID, field
    assert lib.gs_undistort(ctx, None, 8, 8, 8, 8, 1, 0, p(src), p(dst), None) == INVALID
    assert lib.gs_undistort(ctx, C.byref(good), 8, 8, 8, 8, 1, 0, None, p(dst), None) == INVALID
    assert lib.gs_undistort(None, C.byref(good), 8, 8, 8, 8, 1, 0, p(src), p(dst), None) == INVALID
    with pytest.raises(ValueError):
        renderer.undistortImage(np.zeros((8, 8), np.float32), L.LensModel(10.0, 10.0, 4.0, 4.0), mode="mask")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_loader_through_the_kernel_matches_the_loader_on_the_host(renderer, tmp_path):
    cpu = _load("test_lens_cpu")
    kw = dict(cpu.two_view_set(tmp_path), maskRoot=str(tmp_path / "masks"), depthRoot=str(tmp_path / "depths"), undistort=True)
    host, _, _ = D.ColmapDataLoader(**kw).load()
    dev, _, _ = D.ColmapDataLoader(**kw).load(undistorter=renderer.undistortImage)
    plain, _, _ = D.ColmapDataLoader(**dict(kw, undistort=False)).load()
    for k in ("rgbArray", "alphaArray", "maskArray", "depthArray"):
        a, b = getattr(host, k), getattr(dev, k)
        assert a.shape == b.shape and a.dtype == b.dtype, k
        np.testing.assert_array_equal(b[0], getattr(plain, k)[0], err_msg=k)           # the pinhole view is not resampled
    K = host.intrinsicArray[1]
    lens = L.LensModel(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *cpu.OPENCV[4:])
    npix = cpu.SRC_W * cpu.SRC_H
    # validity: no mask file here would make maskArray the validity itself; with one, compare the validity through the alpha of a
    # second load without masks
    kw0 = dict(kw, maskRoot=None)
    vh = D.ColmapDataLoader(**kw0).load()[0].maskArray[1]
    vd = D.ColmapDataLoader(**kw0).load(undistorter=renderer.undistortImage)[0].maskArray[1]
    flips = int((vh != vd).sum())
    print(f"loader: {flips} validity flips of {npix} (cap {CAP * npix:.0f})")
    assert set(np.unique(vd)) <= {0, 255} and flips <= CAP * npix
    both = (vh == 255) & (vd == 255)
    rgba = np.concatenate([plain.rgbArray[1], plain.alphaArray[1][..., None]], -1)
    bar = L.remap_bar(rgba, lens)
    got = np.concatenate([dev.rgbArray[1], dev.alphaArray[1][..., None]], -1).astype(np.float64)
    want, _ = L.remap_values(rgba, lens)
    err = np.abs(got - want)
    print(f"loader images: max err / bar = {(err[both] / bar[both]).max():.3f}")
    assert np.all(err[both] <= bar[both])
    # the mask: one level at most, on few pixels; the depth inside its bar
    dm = np.abs(host.maskArray[1].astype(int) - dev.maskArray[1].astype(int))[both]
    assert dm.max() <= 1 and (dm > 0).sum() <= CAP * npix
    dbar = L.remap_bar(plain.depthArray[1], lens, mode="depth")
    dwant, _ = L.remap_values(plain.depthArray[1], lens, mode="depth")
    derr = np.abs(dev.depthArray[1].astype(np.float64) - dwant)
    with np.errstate(divide="ignore", invalid="ignore"):        # (four holes: err 0 under a bar of 0)
        print(f"loader depth: max err / bar = {np.where(derr[both] > 0, derr[both] / dbar[both], 0.0).max():.3f}")
    assert np.all(derr[both] <= dbar[both])
