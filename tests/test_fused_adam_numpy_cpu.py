"""tests/fused_adam_numpy.py on the CPU: the bars admit the IEEE float32 step and no more than rounding, the hand-laid arena
is what it says, and every scene of tests/test_gpu_fused_adam_elementwise.py gives the gradients and the invisible sets that
file relies on (float32 oracle)."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_fan_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fan = _load("fused_adam_numpy")
LRS = [0.00016, 0.0025, 0.0025 / 20, 0.005, 0.001, 0.025]          # trainer.getLearningRates(0, 1000)


def _within(p0, m0, v0, g, lr, scale, what):
    p, m, v = fan.restate32(p0, m0, v0, g, lr, scale=scale, **fan.ADAM)
    b = fan.bars(p0, m0, v0, g, p, m, v, lr, scale=scale, **fan.ADAM)
    for k in ("ratio_m", "ratio_v", "ratio_p"):
        assert b[k].shape == p0.shape and np.isfinite(b[k]).all(), (what, k)      # the pair leaves out no element
        i = int(np.argmax(b[k]))
        print(f"{what} scale {scale}: largest {k} {b[k][i]:.3f} at element {i} (p0 {p0[i]:.3e} m0 {m0[i]:.3e} v0 {v0[i]:.3e} g {g[i]:.3e})")
        assert b[k][i] <= 1.0, (what, k, i)
    return b


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_the_ieee_step_lies_within_every_bar_on_the_value_table(scale):
    from gaussiansplattingmlx_amd.trainer import getLearningRates
    assert np.array_equal(np.asarray(LRS, np.float32), np.asarray(getLearningRates(0, 1000), np.float32))
    t = fan.value_table(LRS)
    assert t["g"].dtype == np.float32 and t["g"].shape[0] >= 6 * 100
    g, m0, v0 = t["g"], t["m0"], t["v0"]
    # the table holds what it says
    assert ((g == 0) & (m0 == 0) & (v0 == 0)).any() and ((g == 0) & (m0 != 0)).any()
    tiny = np.abs(g) == np.float32(1e-25)
    assert tiny.any() and (tiny & (m0 != 0)).any() and ((g[tiny] * g[tiny]) == 0).all()
    sub = (np.abs(g) == np.float32(1e-20)) & (v0 == 0)
    assert sub.any()
    p, m, v = fan.restate32(t["p0"], m0, v0, g, t["lr"], scale=scale, **fan.ADAM)
    assert ((v[sub] > 0) & (v[sub] < fan.TINY)).all()                      # a subnormal v
    near = (g != 0) & (np.abs(m) < 1e-2 * np.abs(np.float32(0.9) * m0)) & (m0 != 0)
    assert near.sum() >= 20 or scale != 1.0                                # b1 m0 close to -(1 - b1) g: the sum cancels
    assert (np.sign(m0[near]) == -np.sign(g[near])).all()
    _within(t["p0"], m0, v0, g, t["lr"], scale, "value table")


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_the_ieee_step_lies_within_every_bar_on_random_elements(scale):
    rng = np.random.default_rng(21)
    n = 100_000
    size = 10.0 ** rng.uniform(-9, 0, n)
    g = (size * rng.normal(0, 1, n)).astype(np.float32)
    m0 = (size * rng.normal(0, 0.5, n)).astype(np.float32)
    v0 = (size * size * rng.uniform(0.01, 1, n)).astype(np.float32)
    p0 = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-5, 0, n)).astype(np.float32)
    lr = np.asarray(LRS, np.float32)[rng.integers(0, 6, n)]
    b = _within(p0, m0, v0, g, lr, scale, "random")
    # the bars are rounding and no more: a step one part in a million off is beyond them
    p, m, v = fan.restate32(p0, m0, v0, g, lr, scale=scale, **fan.ADAM)
    off = fan.bars(p0, m0, v0, g, p, (m * np.float32(1 + 1e-6)), (v * np.float32(1 + 1e-6)), lr, scale=scale, **fan.ADAM)
    assert (off["ratio_v"] > 1).mean() > 0.99 and (off["ratio_m"] > 1).mean() > 0.5
    # (where the step is no smaller than the parameter: elsewhere the subtraction's own rounding is the larger term)
    d = lr.astype(np.float64) * m / (np.sqrt(v.astype(np.float64)) + float(np.float32(1e-15)))
    moved = np.abs(d) > np.abs(p0)
    off = fan.bars(p0, m0, v0, g, (p0 - d * (1 + 3e-6)).astype(np.float32), m, v, lr, scale=scale, **fan.ADAM)
    assert moved.sum() > 1000 and (off["ratio_p"][moved] > 1).all()
    assert float(b["ratio_p"].max()) > 0.05                                # ... and the IEEE step is not far inside them


def test_a_flushed_square_root_lies_within_the_parameter_bar():
    """A stored v that is subnormal: the step taken with sqrt(v) and the step taken with 0 both pass, a step beyond does not."""
    f = np.float32
    p0, m0, v0, g = f([0.0, 1e-8]), f([0.0, 0.0]), f([0.0, 0.0]), f([1e-20, -1e-20])
    lr = f([0.005, 0.025])
    p, m, v = fan.restate32(p0, m0, v0, g, lr, scale=1.0, **fan.ADAM)
    assert ((v > 0) & (v < fan.TINY)).all()
    flushed = p0 - (lr * m) / f(1e-15)
    for step in (p, flushed):
        assert (fan.bars(p0, m0, v0, g, step, m, v, lr, scale=1.0, **fan.ADAM)["ratio_p"] <= 1).all()
    beyond = p0 - (lr * m) / f(1e-15) * f(1.001)
    assert (fan.bars(p0, m0, v0, g, beyond, m, v, lr, scale=1.0, **fan.ADAM)["ratio_p"] > 1).all()


@pytest.mark.parametrize("K", [16, 25])
@pytest.mark.parametrize("res", [1, 2, 3])
def test_hand_arena(K, res):
    N = 65
    p, _, _ = fan.scene(32, 16, N, K, 5)
    h = fan.hand_arena(p, N, K, res)
    per = fan.row_floats(K)
    assert h["starts"]["features_rest"] % 4 == res and h["numel"] % 4 == 0
    assert int(h["mask"].sum()) == N * sum(per.values()) and not h["mask"].all()
    for name in ("arena", "m", "v"):
        buf = h[name]
        assert buf.dtype == np.float32 and buf.shape == (h["numel"],)
        assert (buf[~h["mask"]] != 0).all()                                # the gaps hold values a stray store would change
        seen = np.zeros(h["numel"], np.int32)
        for k in fan.KEYS:
            view = h["views"][name][k]
            assert np.shares_memory(view, buf) and view.shape == (N,) + fan.row_shape(K)[k]
            assert view.ravel().ctypes.data == buf.ctypes.data + 4 * h["starts"][k]      # (ravel of a contiguous view: no copy)
            seen[h["starts"][k]:h["starts"][k] + N * per[k]] += 1
        assert np.array_equal(seen == 1, h["mask"]) and seen.max() == 1    # the tensors partition the masked elements
    for k in fan.KEYS:
        assert np.array_equal(h["views"]["arena"][k], p[k])
        assert not h["views"]["m"][k].any() and not h["views"]["v"][k].any()
    # a write through a view lands in the buffer
    h["views"]["m"]["features_rest"][3, 2, 1] = 7.0
    assert h["m"][h["starts"]["features_rest"] + 3 * per["features_rest"] + 2 * 3 + 1] == 7.0
    rows, cols = fan.element_rows(h["ids"], h["starts"], N, K), fan.rest_columns(h["ids"], h["starts"], N, K)
    assert np.array_equal(rows >= 0, h["mask"]) and np.array_equal(cols >= 0, h["ids"] == 2)
    assert np.bincount(rows[rows >= 0]).tolist() == [sum(per.values())] * N


def test_invisible_sets_have_the_structure_asked_for():
    inv = fan.invisible_set(321, "blocked")
    waves = inv[:320].reshape(5, 64).sum(axis=1)
    assert waves.tolist() == [64, 64, 0, 64, 45] and not inv[320]        # a workgroup, a visible and an invisible wave, a mixed wave
    inv = fan.invisible_set(321, "scattered", 4)
    waves = inv[:320].reshape(5, 64).sum(axis=1)
    assert ((waves > 8) & (waves < 56)).all() and 0.25 < inv.mean() < 0.45
    assert not fan.invisible_set(64, None).any()


SCENES = [(W, H, N, K, inv) for (W, H) in fan.SIZES for N, K, inv in
          [(321, 25, None), (321, 16, "scattered"), (321, 25, "blocked"), (129, 9, None), (65, 4, "scattered"), (63, 1, None)]]


@pytest.mark.parametrize("W,H,N,K,inv", SCENES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in SCENES])
def test_scene_reaches_what_the_device_test_needs(oracle32, W, H, N, K, inv):
    p, cams, invisible = fan.scene(W, H, N, K, 7, invisible=inv)
    assert np.array_equal(invisible, fan.invisible_set(N, inv, 7))
    cot = fan.cotangent(W, H)
    z = np.zeros(W * H, np.float32)
    for d in sorted({fan.DEGREE[K], min(1, fan.DEGREE[K])}):
        lact = fan.active_columns(d)
        for cam in cams:
            fw = oracle32.render_forward(p, cam.as_dict(), W, H, 16, 16, d)
            radii = np.asarray(fw["proj"]["radii"]).reshape(-1)
            assert np.array_equal(radii == 0, invisible)                   # behind the camera, and nothing else
            g = oracle32.render_backward(p, cam.as_dict(), W, H, 16, 16, d, fw, cot.reshape(-1, 3), z, z)
            for k in fan.KEYS:
                if np.asarray(g[k]).size:
                    assert np.abs(np.asarray(g[k])).max() > 0, k
                    assert not np.asarray(g[k]).reshape(N, -1)[invisible].any(), k
            if lact:
                rest = np.asarray(g["features_rest"]).reshape(N, -1)
                full = (rest[:, :lact] != 0).all(axis=1)
                print(f"{W}x{H} N {N} K {K} degree {d}: {int(full.sum())} of {N} rows ({int((~invisible).sum())} visible) "
                      f"with a non-zero gradient in every active column")
                # half of all rows; the blocked set leaves fewer than half visible, so there three quarters of those
                assert full.sum() >= (0.75 * (~invisible).sum() if inv == "blocked" else 0.5 * N)
                assert not rest[:, lact:].any()
