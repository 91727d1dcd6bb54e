"""The evaluation kernels on the device (include/gsplat.h gs_image_metrics / gs_colour_moments, GaussianRenderer.imageMetrics /
colourMoments) against the float64 restatement (tests/metrics_numpy.py) on the same float32 inputs.

Bars, fixed before the first run on the card:
  - wsum: equal to the float64 sum for no mask and {0, 255} masks (whole numbers: a dropped or double-counted pixel shows),
    within 1e-12 relative for soft masks (float32 weights summed in double, in another order); out[3] == 3 out[2];
  - sse: 1e-6 relative (three float32 roundings per term, at most 4 * 2^-24, under double sums), so the PSNR within 1e-5 dB
    wherever mse >= 1e-8; exactly 0 under an all-zero mask;
  - mean SSIM: no further from float64 than the float32 mirror's worst pixel (where w > 0) is from float64 on that very case,
    floor 1e-6 -- computed here from the two mirrors, not a constant;
  - the 22 moments: 1e-6 relative, 1e-12 absolute where the truth is 0;
  - two calls give identical bits; a mask of all 255 gives the bits of no mask; the error codes of the header.

Shapes, for the kernel's 32 x 32 tiles: 1 x 1; 5 x 7 (smaller than the window); 32 x 32 (exactly one tile); 33 x 33 (one tile
plus one pixel each way); 67 x 45 and 97 x 131 (several tiles, ragged edges; the latter 20 tiles on 24 blocks a channel group:
bands of three tiles per XCD and empty blocks behind the last)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (5, 7), (32, 32), (33, 33), (67, 45), (97, 131)]
SSE_BAR, PSNR_BAR, SSIM_FLOOR, MOMENT_REL, MOMENT_ABS = 1e-6, 1e-5, 1e-6, 1e-6, 1e-12


def _load(name):
    spec = importlib.util.spec_from_file_location("_gm_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("metrics_numpy")
_state = {}


@pytest.fixture(scope="module")
def r():
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    rr = GaussianRenderer(4, 64, 64, (16, 16), False)      # (the calls take their own H, W: any context measures any size)
    yield rr
    _state.clear()
    rr.close()


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _case(H, W, image, kind):
    """Host and device inputs of one case with both mirrors: computed once, never written."""
    key = (H, W, image, kind)
    if key not in _state:
        a, b = mn.IMAGES[image](H, W, 100 + H + W)
        mask = mn.make_mask(kind, H, W, H * W)
        _state[key] = dict(a=a, b=b, mask=mask, dev=(_dev(a), _dev(b), _dev(mask)), m64=mn.image_metrics(a, b, mask),
                           m32=mn.image_metrics(a, b, mask, np.float32), moments=mn.colour_moments(a, b, mask))
    return _state[key]


@pytest.mark.parametrize("image", list(mn.IMAGES))
@pytest.mark.parametrize("H,W", SHAPES)
def test_image_metrics_against_float64(r, H, W, image):
    for kind in mn.MASKS:
        c = _case(H, W, image, kind)
        got = r.imageMetrics(*c["dev"]).cpu().numpy()
        want, m64, m32 = c["m64"]["sums"], c["m64"], c["m32"]
        seen = m64["w"] > 0
        bar = max(SSIM_FLOOR, float(np.abs(m32["map"].astype(np.float64) - m64["map"])[seen].max()) if seen.any() else 0.0)
        psnr, ssim = mn.from_sums(got)
        print(f"{H}x{W} {image} {kind}: sse {got[0]:.9e} ({want[0]:.9e}) ssim {ssim:.9f} ({m64['ssim']:.9f}, mirror32 "
              f"{m32['ssim']:.9f}, bar {bar:.2e}) wsum {got[2]} ({want[2]}) psnr {psnr:.6f} ({m64['psnr']:.6f})")
        assert got.dtype == np.float64 and got[3] == 3.0 * got[2]
        if kind == "soft":
            assert abs(got[2] - want[2]) <= 1e-12 * want[2]
        else:
            assert got[2] == want[2], (kind, got[2], want[2])
        if kind == "zeros":
            assert got[0] == 0.0 and got[1] == 0.0 and np.isnan(psnr) and np.isnan(ssim)
            continue
        assert abs(got[0] - want[0]) <= SSE_BAR * want[0], (kind, got[0], want[0])
        if want[0] / want[3] >= 1e-8:
            assert abs(psnr - m64["psnr"]) <= PSNR_BAR, (kind, psnr, m64["psnr"])
        assert abs(ssim - m64["ssim"]) <= bar, (kind, ssim, m64["ssim"], bar)


@pytest.mark.parametrize("image", ["noise", "ramp"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_colour_moments_against_float64(r, H, W, image):
    for kind in mn.MASKS:
        c = _case(H, W, image, kind)
        got = r.colourMoments(*c["dev"]).cpu().numpy()
        want = c["moments"]
        err = np.abs(got - want)
        print(f"{H}x{W} {image} {kind}: worst relative {float((err / np.maximum(np.abs(want), 1e-300)).max()):.2e}")
        assert got.shape == (22,) and got.dtype == np.float64
        assert (err <= np.where(want == 0, MOMENT_ABS, MOMENT_REL * np.abs(want))).all(), (kind, got, want)
        assert got[9] == c["m64"]["sums"][2] or kind == "soft"


def test_large_grid_wraps_the_moment_loop(r):
    """300 x 450: more pixels than 512 blocks x 256 threads, so colour_moments_kernel's grid-stride loop wraps."""
    a, b = mn.noise_pair(300, 450, 5)
    mask = mn.make_mask("binary", 300, 450, 5)
    got = r.colourMoments(_dev(a), _dev(b), _dev(mask)).cpu().numpy()
    want = mn.colour_moments(a, b, mask)
    assert (np.abs(got - want) <= MOMENT_REL * np.abs(want)).all() and got[9] == want[9]


@pytest.mark.parametrize("H,W", [(5, 7), (67, 45), (97, 131)])
def test_bits(r, H, W):
    """Two calls give the same bits; a mask of all 255 gives the bits of no mask."""
    for image in ("noise", "ramp"):
        plain, ones, soft = (_case(H, W, image, k)["dev"] for k in ("none", "ones", "soft"))
        for fn in (r.imageMetrics, r.colourMoments):
            x, y = fn(*soft), fn(*soft)
            assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
            assert torch.equal(fn(*plain), fn(*ones))


def test_out_rows_and_host_masks(r):
    """out= writes a row of a [V, 4] buffer and nothing else; a host bool mask means 0 / 255."""
    c = _case(67, 45, "noise", "binary")
    buf = torch.full((3, 4), float("nan"), dtype=torch.float64, device="cuda")
    back = r.imageMetrics(*c["dev"], out=buf[1])
    assert back.data_ptr() == buf[1].data_ptr()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[2]).all())
    assert torch.equal(buf[1], r.imageMetrics(*c["dev"]))
    assert torch.equal(buf[1], r.imageMetrics(c["a"], c["b"], c["mask"] != 0))
    with pytest.raises(ValueError):
        r.imageMetrics(c["a"], c["b"][:-1])
    with pytest.raises(ValueError):
        r.imageMetrics(c["a"], c["b"], c["mask"][:-1])
    with pytest.raises(ValueError):
        r.colourMoments(c["a"], c["b"], out=torch.zeros(22, device="cuda"))


def test_error_codes_and_empty_images(r):
    from gaussiansplattingmlx_amd import _lib
    a, b, m = _case(5, 7, "noise", "soft")["dev"]
    pa, pb, pm = (C.c_void_p(t.data_ptr()) for t in (a, b, m))
    out = torch.full((22,), float("nan"), dtype=torch.float64, device="cuda")
    po = C.c_void_p(out.data_ptr())
    bad = "GS_ERR_INVALID_ARG"
    for args in ((-1, 7, pa, pb, pm, po), (5, -1, pa, pb, pm, po), (5, 7, None, pb, pm, po), (5, 7, pa, None, pm, po),
                 (5, 7, pa, pb, pm, None)):
        assert _lib.STATUS.get(r.lib.gs_image_metrics(r.ctx, *args)) == bad, args
        assert b"gs_image_metrics" in r.lib.gs_last_error(r.ctx)
    for args in ((-1, pa, pb, pm, po), (35, None, pb, pm, po), (35, pa, None, pm, po), (35, pa, pb, pm, None)):
        assert _lib.STATUS.get(r.lib.gs_colour_moments(r.ctx, *args)) == bad, args
        assert b"gs_colour_moments" in r.lib.gs_last_error(r.ctx)
    r.sync()
    assert bool(torch.isnan(out).all())                    # a refused call writes nothing
    for H, W in ((0, 7), (5, 0), (0, 0)):
        out.fill_(float("nan"))
        assert r.lib.gs_image_metrics(r.ctx, H, W, pa, pb, None, po) == 0
        assert out[:4].tolist() == [0.0] * 4 and bool(torch.isnan(out[4:]).all())
    assert r.lib.gs_colour_moments(r.ctx, 0, pa, pb, None, po) == 0
    assert out.tolist() == [0.0] * 22


def test_workspace_is_allocated_once_and_regrown_for_a_larger_image():
    """The partials live in the context: allocated at the first call (512 x 22 doubles), untouched by a repeated call and by any
    image that needs no more, regrown when a larger image does -- 1216 x 1216 is 1444 tiles, 4344 blocks of three doubles.  That
    image is all zeros against itself: sse 0, every ssim value C1 C2 / (C1 C2) = 1, so the sums are whole numbers."""
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    rr = GaussianRenderer(4, 64, 64, (16, 16), False)
    try:
        ws = lambda: int(rr.lib.gs_workspace_bytes(rr.ctx))      # noqa: E731
        a, b, m = _case(67, 45, "noise", "soft")["dev"]
        before = ws()
        first = rr.imageMetrics(a, b, m)
        assert ws() == before + 512 * 22 * 8
        for _ in range(2):
            assert torch.equal(rr.imageMetrics(a, b, m), first)
            rr.colourMoments(a, b, m)
        assert ws() == before + 512 * 22 * 8
        z = torch.zeros(1216, 1216, 3, device="cuda")
        got = rr.imageMetrics(z, z).cpu().numpy()
        assert ws() == before + 3 * 4344 * 8
        P = 1216.0 * 1216.0
        assert got.tolist() == [0.0, 3.0 * P, P, 3.0 * P]
        assert torch.equal(rr.imageMetrics(a, b, m), first) and ws() == before + 3 * 4344 * 8
    finally:
        rr.close()
