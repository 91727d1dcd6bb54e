"""The bilateral grid without a device: the numpy restatement's VJPs against central differences of the float64 composed loss
(tests/bilateral_grid_numpy.py), the TV gradient, the identity and constant-grid properties in float32, the trainer's
learning-rate schedule and refusals, and the header's declarations (include/gsplat.h gs_set_bilateral_grid,
gs_apply_bilateral_grid)."""
import importlib.util
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_bgc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bg = _load("bilateral_grid_numpy")
en = _load("exposure_numpy")
SHAPE = (4, 3, 5)


def _images(H, W, seed):
    rng = np.random.default_rng(seed)
    ren = rng.uniform(0.05, 0.95, (H, W, 3))
    tgt = np.clip(ren + rng.normal(0, 0.15, ren.shape), 0, 1)
    return ren, tgt


def _boundary_pixel(ren, p, gl):
    """Nudges pixel p's red channel until its guidance lands exactly on a z-cell boundary (w an integer in (0, gl - 1))."""
    r = ren[p].copy()
    r[1] = r[2] = 0.5
    r[0] = (0.5 - 0.587 * 0.5 - 0.114 * 0.5) / 0.299            # gray = 0.5 -> w = (gl - 1) / 2, an integer for odd gl
    for _ in range(200):
        ren[p] = r
        w = bg.place(ren, SHAPE, np.float64)[5][p]
        if w == 0.0:
            return
        r[0] = np.nextafter(r[0], -np.inf if w > 0.5 else np.inf)
    raise AssertionError("no exact boundary found")


@pytest.mark.parametrize("depth", [False, True])
def test_vjp_against_central_differences(oracle64, depth):
    """dL/dr and dL/dG of the restatement against float64 central differences of the composed loss (+ tv_weight TV for the
    grid).  h = 1e-6: the loss is smooth in G away from the L1 kink and in r away from the kinks of the slice (a z-cell
    boundary, the clamp at 0 and 1), which a random image meets with probability ~0.  Pixels on those kinks are tested on the
    side the VJP takes: a clamped pixel (dgray = 0) by central differences, a pixel exactly on a z boundary (the VJP takes
    the cell above) by a forward difference.  Bars: 1e-6 of the largest component for central differences; 1e-4 for the
    forward difference (its O(h) truncation)."""
    H, W = 14, 17
    ren, tgt = _images(H, W, 11)
    ren[2, 3] = (1.3, 1.2, 1.1)                 # guidance clamped at 1
    ren[5, 6] = (-0.2, -0.1, -0.3)              # ... and at 0
    _boundary_pixel(ren, (7, 8), SHAPE[2])
    kw = {}
    if depth:
        rng = np.random.default_rng(3)
        kw = dict(renderDepth=rng.uniform(1, 4, (H, W)), targetDepth=rng.uniform(1, 4, (H, W)),
                  depthMask=rng.uniform(size=(H, W)) > 0.5, lambdaDepth=0.3)
    G = bg.random_grid(np.random.default_rng(5), SHAPE, 0.3).astype(np.float64)
    tvw = 0.5
    _, dr, dG, _ = bg.composed(oracle64, ren, tgt, G, SHAPE, tvw, **kw)

    def L(r, Gx):
        return bg.composed(oracle64, r, tgt, Gx, SHAPE, 0.0, **kw)[0] + tvw * bg.tv(Gx, SHAPE)
    h = 1e-6
    rng = np.random.default_rng(8)
    idx = [tuple(rng.integers(0, n) for n in G.shape) for _ in range(24)] + [(1, 2, 2, k) for k in range(12)]
    for i in idx:
        Gp, Gm = G.copy(), G.copy()
        Gp[i] += h
        Gm[i] -= h
        fd = (L(ren, Gp) - L(ren, Gm)) / (2 * h)
        assert abs(fd - dG[i]) <= 1e-6 * np.abs(dG).max(), (i, fd, dG[i])
    for p in [(0, 0), (4, 9), (13, 16), (2, 3), (5, 6)]:
        for j in range(3):
            rp, rm = ren.copy(), ren.copy()
            rp[p][j] += h
            rm[p][j] -= h
            fd = (L(rp, G) - L(rm, G)) / (2 * h)
            assert abs(fd - dr[p][j]) <= 1e-6 * np.abs(dr).max(), (p, j, fd, dr[p][j])
    p = (7, 8)
    for j in range(3):
        rp = ren.copy()
        rp[p][j] += h
        fd = (L(rp, G) - L(ren, G)) / h
        assert abs(fd - dr[p][j]) <= 1e-4 * np.abs(dr).max(), (p, j, fd, dr[p][j])


def test_tv_gradient_against_differences():
    G = bg.random_grid(np.random.default_rng(2), SHAPE, 0.5).astype(np.float64)
    g = bg.tv_grad(G, SHAPE)
    h = 1e-6
    for i in [(0, 0, 0, 0), (2, 3, 4, 11), (1, 1, 2, 5), (0, 3, 1, 3), (2, 0, 0, 7)]:
        Gp, Gm = G.copy(), G.copy()
        Gp[i] += h
        Gm[i] -= h
        assert abs((bg.tv(Gp, SHAPE) - bg.tv(Gm, SHAPE)) / (2 * h) - g[i]) <= 1e-7, i
    assert bg.tv(bg.constant(en.random_exposure(np.random.default_rng(1)), SHAPE), SHAPE) == 0.0
    n_x = 12 * SHAPE[2] * SHAPE[1] * (SHAPE[0] - 1)
    G1 = bg.identity(SHAPE).astype(np.float64)
    G1[0, 1, 0, 0] += 1.0                        # one step along x (and y, z) from the identity
    assert math.isclose(bg.tv(G1, SHAPE), 2.0 / n_x + 1.0 / (12 * SHAPE[2] * SHAPE[0] * (SHAPE[1] - 1))
                        + 1.0 / (12 * SHAPE[0] * SHAPE[1] * (SHAPE[2] - 1)), rel_tol=1e-12)


def test_identity_and_constant_grids_in_float32():
    rng = np.random.default_rng(1)
    img = rng.uniform(-0.1, 1.1, (9, 13, 3)).astype(np.float32)
    assert np.array_equal(bg.apply(bg.identity(SHAPE), img, SHAPE), img)
    g = rng.normal(0, 1, img.shape).astype(np.float32)
    dr, dG = bg.vjp(bg.identity(SHAPE), g, img, SHAPE)
    assert np.array_equal(dr, g)
    M = en.random_exposure(rng)
    Gc = bg.constant(M, SHAPE)
    a, dP, _ = bg.slice_grid(Gc, img, SHAPE)
    assert np.array_equal(a, np.broadcast_to(M, a.shape)) and not dP.any()
    dr, dG = bg.vjp(Gc, g, img, SHAPE, tv_weight=10.0)
    want_dr, want_dM = en.vjp(M, g, img)
    assert np.abs(dr - want_dr).max() <= 1e-6 * np.abs(want_dr).max()
    # to rounding: the trilinear weights and g r are float32 products (measured 2.6e-8 of the largest component)
    assert np.abs(dG.sum((0, 1, 2)) - want_dM).max() <= 1e-6 * np.abs(want_dM).max()


def test_cells_partition_the_image():
    """Every pixel lies in exactly one cell, and small images leave cells empty (the device's chunked backward relies on it)."""
    for (W, H), shape in [((37, 11), (16, 16, 8)), ((800, 800), (16, 16, 8)), ((5, 3), (2, 2, 2)), ((200, 152), (5, 3, 4))]:
        x0, _, y0, _, _, _, _ = bg.place(np.zeros((H, W, 3)), shape)
        assert np.all(np.diff(x0) >= 0) and np.all(np.diff(y0) >= 0)
        assert x0.min() >= 0 and x0.max() <= shape[0] - 2 and y0.min() >= 0 and y0.max() <= shape[1] - 2
    x0, _, y0, _, _, _, _ = bg.place(np.zeros((11, 37, 3)), (16, 16, 8))
    assert len(set(y0)) < 15                      # 11 rows over 15 cell rows


def test_learning_rate_schedule():
    from gaussiansplattingmlx_amd.trainer import bilateralGridLearningRate as f
    T = 30000
    assert math.isclose(f(0, T), 2e-5, rel_tol=1e-12)
    assert math.isclose(f(1000, T), 2e-3 * 0.01 ** (1000 / T), rel_tol=1e-12)
    assert math.isclose(f(500, T), 2e-3 * (0.01 + 0.99 * 0.5) * 0.01 ** (500 / T), rel_tol=1e-12)
    assert math.isclose(f(T, T), 2e-5, rel_tol=1e-12)
    assert math.isclose(f(3 * T, T), 2e-5, rel_tol=1e-12)              # held at the final rate
    assert math.isclose(f(1000, T, 1e-2), 1e-2 * 0.01 ** (1000 / T), rel_tol=1e-12)
    up = [f(t, T) for t in range(0, 1001, 100)]
    down = [f(t, T) for t in range(1000, T + 1, 1000)]
    assert all(a < b for a, b in zip(up, up[1:])) and all(a > b for a, b in zip(down, down[1:]))


@pytest.mark.parametrize("kw", [dict(exposure_opt=True), dict(views_per_rank=2), dict(process_group=object()),
                                dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"), dict(n_views=None),
                                dict(n_views=0), dict(n_views=2.5), dict(n_views=-1), dict(bilateral_grid_shape=(1, 16, 8)),
                                dict(bilateral_grid_shape=(16, 65, 8)), dict(bilateral_grid_shape=(16, 16, 33)),
                                dict(bilateral_grid_shape=(16, 16)), dict(bilateral_grid_shape=(16.5, 16, 8)),
                                dict(bilateral_grid_shape="big"), dict(bilateral_grid_lr=0.0), dict(bilateral_grid_lr=-1e-3),
                                dict(bilateral_grid_lr=float("nan")), dict(bilateral_grid_lr="fast"),
                                dict(bilateral_grid_lr=None), dict(bilateral_grid_tv=-1.0),
                                dict(bilateral_grid_tv=float("inf")), dict(bilateral_grid_tv=None)])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(bilateral_grid=True, n_views=4)
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_header_declares_and_library_exports_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "int gs_set_bilateral_grid(gs_ctx* ctx, const float* grid" in src
    assert "int gs_apply_bilateral_grid(gs_ctx* ctx, int W, int H, const float* grid" in src
    assert "#define GSPLAT_ABI_VERSION 6" in src
    from gaussiansplattingmlx_amd import _lib
    assert {"gs_set_bilateral_grid", "gs_apply_bilateral_grid"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert hasattr(lib, "gs_set_bilateral_grid") and hasattr(lib, "gs_apply_bilateral_grid")


def test_hip_source_is_built_without_contraction():
    from gaussiansplattingmlx_amd import build
    assert build.SOURCES["bilateral_grid.hip"] == ["-ffp-contract=off"]
    assert build.SOURCES["exposure.hip"] == ["-ffp-contract=off"]
