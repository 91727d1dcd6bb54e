"""Held-out evaluation, host side: the numpy restatement of gs_image_metrics / gs_colour_moments
(tests/metrics_numpy.py) against its own brute force and against closed forms, and gaussiansplattingmlx_amd/evaluation.py --
the affine colour fit, the result container and the view split.  No GPU."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_mc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("metrics_numpy")


def test_separable_float64_agrees_with_the_121_tap_window():
    a, b = mn.ramp_pair(23, 17, 1)
    a, b = mn.clamp(a), mn.clamp(b)
    assert np.abs(mn.ssim_map(a, b) - mn.ssim_map_bruteforce(a, b)).max() <= 1e-12
    w = mn.weights(mn.make_mask("soft", 23, 17, 1), (23, 17))[..., None]
    assert np.abs(mn.ssim_map(w * a, w * b) - mn.ssim_map_bruteforce(w * a, w * b)).max() <= 1e-12


def test_the_window_is_centred_and_is_the_package_s():
    from gaussiansplattingmlx_amd.evaluation import centred_window
    g = mn.taps()
    np.testing.assert_allclose(g, g[::-1], rtol=0, atol=1e-17)
    assert abs(g.sum() - 1.0) < 1e-15 and g.argmax() == 5
    win = centred_window()
    assert win.dtype == np.float32 and win.shape == (11, 11)
    np.testing.assert_allclose(win, np.outer(g, g), rtol=0, atol=1e-8)
    np.testing.assert_array_equal(win, win.T[::-1, ::-1])


def test_constant_offset_of_a_tenth_is_20_db():
    a = np.full((9, 13, 3), 0.4, np.float32)
    res = mn.image_metrics(a, a + np.float32(0.1))
    assert abs(res["psnr"] - 20.0) < 1e-5          # (0.4f + 0.1f is 0.5f to a rounding: 1.5e-7 of the difference)


def test_identical_images_give_inf_and_one():
    from gaussiansplattingmlx_amd.evaluation import metrics_from_sums
    a, _ = mn.noise_pair(12, 15, 2)
    res = mn.image_metrics(a, a)
    assert res["psnr"] == np.inf and abs(res["ssim"] - 1.0) < 1e-12
    psnr, ssim, weight = metrics_from_sums(res["sums"])
    assert psnr == np.inf and abs(ssim - 1.0) < 1e-12 and weight == 12 * 15


def test_all_zero_mask_gives_nan_and_is_left_out_of_the_mean_and_counted():
    from gaussiansplattingmlx_amd.evaluation import EvalResult
    a, b = mn.noise_pair(12, 15, 3)
    blank = mn.image_metrics(a, b, mn.make_mask("zeros", 12, 15, 3))
    assert np.isnan(blank["psnr"]) and np.isnan(blank["ssim"]) and blank["sums"][2] == 0
    seen = mn.image_metrics(a, b)
    same = mn.image_metrics(a, a)
    res = EvalResult.from_sums(np.stack([seen["sums"], blank["sums"], same["sums"]]))
    assert np.isnan(res.psnr[1]) and res.psnr[2] == np.inf
    assert res.mean_psnr == seen["psnr"]                     # the nan view and the inf view are left out
    assert abs(res.mean_ssim - 0.5 * (seen["ssim"] + 1.0)) < 1e-15
    assert res.skipped == dict(psnr=2, ssim=1, cc_psnr=0, cc_ssim=0)
    assert res.cc_psnr is None and np.isnan(res.mean_cc_psnr)
    np.testing.assert_array_equal(res.weight, [180.0, 0.0, 180.0])


def test_a_mask_of_all_255_equals_no_mask():
    a, b = mn.ramp_pair(14, 19, 4)
    for dtype in (np.float64, np.float32):
        x, y = mn.image_metrics(a, b, None, dtype), mn.image_metrics(a, b, mn.make_mask("ones", 14, 19, 4), dtype)
        np.testing.assert_array_equal(x["sums"], y["sums"])


def test_float32_mirror_stays_close_to_float64():
    a, b = mn.noise_pair(33, 29, 5)
    x, y = mn.image_metrics(a, b, None, np.float32), mn.image_metrics(a, b)
    assert x["map"].dtype == np.float32
    assert np.abs(x["map"] - y["map"]).max() < 1e-5 and abs(x["ssim"] - y["ssim"]) < 1e-6
    assert abs(x["sums"][0] - y["sums"][0]) <= 1e-6 * y["sums"][0]


def test_fit_matches_lstsq_on_the_pixel_matrix():
    from gaussiansplattingmlx_amd.evaluation import fit_affine_colour
    a, b = mn.noise_pair(21, 16, 6)
    for kind in ("none", "soft"):
        mask = mn.make_mask(kind, 21, 16, 6)
        m = mn.colour_moments(a, b, mask)
        assert m.shape == (22,) and abs(m[9] - mn.weights(mask, (21, 16)).sum()) < 1e-9
        S = np.zeros((4, 4))
        for k, (i, j) in enumerate(mn.TRIU):
            S[i, j] = S[j, i] = m[k]
        want = np.linalg.lstsq(S, m[10:].reshape(4, 3), rcond=None)[0].T
        M = fit_affine_colour(m)
        assert M.dtype == np.float32 and M.shape == (3, 4)
        np.testing.assert_array_equal(M, want.astype(np.float32))
        assert np.abs(want - mn.pixel_matrix_fit(a, b, mask)).max() <= 1e-9


def test_fit_is_finite_for_a_constant_render():
    from gaussiansplattingmlx_amd.evaluation import fit_affine_colour
    _, b = mn.noise_pair(10, 10, 7)
    for value in (0.0, 0.37):
        M = fit_affine_colour(mn.colour_moments(np.full((10, 10, 3), value, np.float32), b))
        assert np.isfinite(M).all()
        # the minimum-norm answer still maps the constant onto the target's mean colour
        got = M[:, :3] @ np.full(3, np.float32(value), np.float64) + M[:, 3]
        np.testing.assert_allclose(got, b.reshape(-1, 3).mean(0, dtype=np.float64), atol=1e-6)


def test_colour_correction_recovers_an_affine_colour_change():
    from gaussiansplattingmlx_amd.evaluation import fit_affine_colour
    rng = np.random.default_rng(8)
    a = (0.2 + 0.6 * rng.random((24, 20, 3))).astype(np.float32)
    A = np.array([[0.8, 0.1, -0.05], [0.05, 0.7, 0.1], [-0.1, 0.05, 0.9]])
    bias = np.array([0.08, 0.12, 0.05])
    t = (a.astype(np.float64) @ A.T + bias).astype(np.float32)
    assert t.min() > 0.0 and t.max() < 1.0
    plain = mn.image_metrics(a, t)
    M = np.linalg.lstsq(*_normal(mn.colour_moments(a, t)), rcond=None)[0].T      # float64 M: the truth
    cc = mn.image_metrics(mn.apply_affine(M, a), t)
    assert plain["psnr"] < 30.0 and cc["psnr"] > 100.0
    M32 = fit_affine_colour(mn.colour_moments(a, t))
    assert np.abs(M32[:, :3] - A).max() < 1e-5 and np.abs(M32[:, 3] - bias).max() < 1e-5


def _normal(m):
    S = np.zeros((4, 4))
    for k, (i, j) in enumerate(mn.TRIU):
        S[i, j] = S[j, i] = m[k]
    return S, m[10:].reshape(4, 3)


def test_split_views():
    from gaussiansplattingmlx_amd.evaluation import split_views
    tr, te = split_views(10, 8)
    assert te.tolist() == [0, 8] and tr.tolist() == [1, 2, 3, 4, 5, 6, 7, 9]
    tr, te = split_views(10, 4, offset=3)
    assert te.tolist() == [3, 7] and len(tr) == 8
    for every in (0, -1):
        tr, te = split_views(5, every)
        assert tr.tolist() == [0, 1, 2, 3, 4] and te.size == 0
    tr, te = split_views(0)
    assert tr.size == 0 and te.size == 0


def test_split_train_data_slices_every_field_and_keeps_none():
    import dataclasses
    from gaussiansplattingmlx_amd.data import TrainData
    from gaussiansplattingmlx_amd.evaluation import split_train_data
    n, H, W = 10, 4, 5
    rng = np.random.default_rng(9)
    full = TrainData(Hs=np.full(n, H), Ws=np.full(n, W), intrinsicArray=rng.random((n, 3, 3)), c2wArray=rng.random((n, 4, 4)),
                     rgbArray=rng.random((n, H, W, 3)), alphaArray=rng.random((n, H, W)), depthArray=rng.random((n, H, W)),
                     maskArray=rng.integers(0, 256, (n, H, W), dtype=np.uint8), depthAlign=rng.random((n, 2)))
    train, test = split_train_data(full, 8)
    for f in dataclasses.fields(TrainData):
        whole = getattr(full, f.name)
        np.testing.assert_array_equal(getattr(test, f.name), whole[[0, 8]])
        np.testing.assert_array_equal(getattr(train, f.name), whole[[1, 2, 3, 4, 5, 6, 7, 9]])
    bare = dataclasses.replace(full, depthArray=None, maskArray=None, depthAlign=None)
    train, test = split_train_data(bare, 8)
    for part in (train, test):
        assert part.depthArray is None and part.maskArray is None and part.depthAlign is None
    assert len(test.rgbArray) == 2 and len(train.c2wArray) == 8


def test_the_binding_declares_both_entry_points_and_the_library_has_the_kernels():
    import ctypes as C
    from gaussiansplattingmlx_amd import _lib, build
    assert "metrics.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["metrics.hip"]
    build.build()
    lib = _lib.load()
    assert len(_lib._SIGS["gs_image_metrics"][1]) == 7 and len(_lib._SIGS["gs_colour_moments"][1]) == 6
    assert _lib.STATUS.get(lib.gs_image_metrics(None, 4, 4, None, None, None, None)) == "GS_ERR_INVALID_ARG"
    assert _lib.STATUS.get(lib.gs_colour_moments(None, C.c_longlong(16), None, None, None, None)) == "GS_ERR_INVALID_ARG"
    so = open(_lib.LIB_PATH, "rb").read()
    assert b"image_metrics_kernel" in so and b"colour_moments_kernel" in so
