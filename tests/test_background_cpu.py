"""Background colour without a device (gaussiansplattingmlx_amd/background.py, include/gsplat.h gs_set_background, DESIGN.md
section 18): the two identities that make a reference for a colour out of the black oracle (tests/background_numpy.py), the
step's colour as a function of (seed, iteration), the settings' checks, the trainer's refusals and the entry points' declaration.

The white identity: with b = (1, 1, 1) the composed backward must be the oracle's own white backward, to the last bit in both
precisions (the shifted alpha cotangent cA - ((gx + gy) + gz) gives the white path's cT = -cA + (gx + gy + gz) exactly).
The finite-difference check: float64 central differences of the composed loss under a colour, h = 1e-4 and a 5 % bar as in
test_gpu_antialiasing (the oracle's 3-sigma cull and integer radii make its loss piecewise smooth).
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import background as bgm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("gs_set_background", "gs_get_background", "gs_composite_target")
FD_BAR, FD_H = 5e-2, 1e-4


def _load(name):
    spec = importlib.util.spec_from_file_location("_bgc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("background_numpy")
W, H, N = ref.W, ref.H, ref.N


def _cotangents(dt):
    rng = np.random.default_rng(17)
    return (rng.normal(size=(W * H, 3)).astype(dt), (0.1 * rng.normal(size=W * H)).astype(dt), rng.normal(size=W * H).astype(dt))


# --------------------------------------------------------------------------------------------------------- the identities
@pytest.mark.parametrize("prec", ["float32", "float64"])
def test_white_is_the_black_backward_under_the_shifted_alpha_cotangent(oracle32, oracle64, prec):
    o = oracle32 if prec == "float32" else oracle64
    p, cams = ref.scene()
    cam = cams[0].as_dict()
    cot, cd, ca = _cotangents(o.dtype)
    black, white = ref.forward(o), ref.forward(o, white=True)
    # forward: the white render is the black one plus 1 - alpha (to rounding: the oracle adds T, not 1 - alpha)
    assert np.abs(bgm.with_background(black["color"], black["alpha"], (1, 1, 1)) - white["color"]).max() <= (1e-6 if prec == "float32" else 1e-14)
    assert np.array_equal(black["alpha"], white["alpha"]) and np.array_equal(black["last"], white["last"])
    want = o.render_backward(p, cam, W, H, 16, 16, 4, white, cot, cd, ca, whiteBg=True)
    got = ref.backward_under(o, (1.0, 1.0, 1.0), cot, cd, ca)
    for k in ref.KEYS + ("gradPacked",):
        assert got[k].dtype == o.dtype
        assert np.array_equal(got[k], want[k]), k
    assert np.abs(want["gradPacked"]).max() > 0


def test_the_scene_shows_its_background_and_has_long_lists(oracle64):
    fw = ref.forward(oracle64)
    a = fw["alpha"].reshape(-1)
    assert abs(float((a < 0.5).mean()) - 0.585) < 0.001
    assert abs(float((a > 0.95).mean()) - 0.307) < 0.001
    assert int(ref.list_lengths(fw).max()) == 775              # against GS_SEG_LEN = 64: the backward's checkpointed segments
    assert int(ref.list_lengths(ref.forward(oracle64, (50, 38))).max()) == 2236


def test_a_colour_moves_the_gradients(oracle64):
    """b = (0.9, 0.2, 0.55) against black, per packed column, as shares of the column's maximum: a backward that ignores or
    mis-channels the colour cannot pass the 1e-3 gradient bar."""
    cot, cd, ca = _cotangents(np.float64)
    g0 = ref.backward_under(oracle64, (0.0, 0.0, 0.0), cot, cd, ca)["gradPacked"]
    g1 = ref.backward_under(oracle64, ref.B_IN, cot, cd, ca)["gradPacked"]
    for col, name in ((9, "opacity"), (0, "mean x"), (2, "conic00")):
        s = np.abs(g1[:, col] - g0[:, col]).max() / np.abs(g0[:, col]).max()
        print(f"{name}: colour against black {s:.3f} of the column's maximum")
        assert s > 5e-2, (name, s)          # fifty times the gradient bar (the share depends on the cotangents drawn)
    # ... and a colour with two channels swapped is as far away
    g2 = ref.backward_under(oracle64, (ref.B_IN[1], ref.B_IN[0], ref.B_IN[2]), cot, cd, ca)["gradPacked"]
    assert np.abs(g2[:, 9] - g1[:, 9]).max() / np.abs(g1[:, 9]).max() > 1e-2


def test_composed_gradient_against_central_differences(oracle64):
    """The black backward under the shifted cotangent against float64 central differences of the composed loss under b: opacity
    and mean elements of the visible splats with the largest opacity gradients."""
    aa = _load("test_antialiasing_cpu")
    from gaussiansplattingmlx_amd.scenes import make_gaussians
    p, cam, w, h = aa._fd_scene()
    c = cam.as_dict()
    b = ref.B_IN
    tgt = oracle64.render_forward(make_gaussians(60, "trained_like", 4), c, w, h, 16, 16, 4)["color"].reshape(h, w, 3)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    _, fw, cot = ref.loss_under(oracle64, p64, c, w, h, tgt, b)
    assert float((fw["alpha"] < 0.5).mean()) > 0.2             # (the background shows)
    g = ref.backward_under(oracle64, b, cot, None, None, fw=fw, p=p64, cam=c, w=w, h=h)
    gblack = ref.backward_under(oracle64, (0, 0, 0), cot, None, None, fw=fw, p=p64, cam=c, w=w, h=h)
    assert np.abs(g["opacity"] - gblack["opacity"]).max() > 1e-2 * np.abs(g["opacity"]).max()
    vis = np.nonzero(fw["proj"]["radii"].reshape(-1) > 0)[0]
    pick = vis[np.argsort(-np.abs(g["opacity"].reshape(-1)[vis]))[:3]]
    for k, cols in (("opacity", (None,)), ("xyz", (0, 1, 2))):
        scale = np.abs(g[k]).max()
        for i in pick:
            for j in cols:
                idx = (i,) if j is None else (i, j)

                def L(d):
                    q = dict(p64); q[k] = p64[k].copy(); q[k][idx] += d
                    return ref.loss_under(oracle64, q, c, w, h, tgt, b)[0]
                fd = (L(FD_H) - L(-FD_H)) / (2 * FD_H)
                gk = float(np.asarray(g[k]).reshape(p64[k].shape)[idx])
                assert abs(gk - fd) <= FD_BAR * max(abs(fd), 1e-2 * scale), (k, idx, gk, fd)


def test_numpy_statements():
    rng = np.random.default_rng(2)
    rgb, a, b = rng.random((5, 7, 3)), rng.random((5, 7)), np.array(ref.B_OUT)
    c = bgm.composite(rgb, a, b)
    assert c.dtype == np.float64 and c.shape == (5, 7, 3)
    assert np.allclose(c, a[..., None] * rgb + (1 - a[..., None]) * b, rtol=0, atol=1e-15)
    assert np.array_equal(bgm.composite(rgb, np.ones((5, 7)), b), rgb)
    assert np.array_equal(bgm.composite(rgb, np.zeros((5, 7)), b), np.broadcast_to(b, (5, 7, 3)))
    w = bgm.with_background(rgb, a, b)
    assert np.allclose(w, rgb + (1 - a)[..., None] * b, rtol=0, atol=1e-15)
    assert bgm.with_background(rgb.astype(np.float32), a.astype(np.float32), b).dtype == np.float32
    g, ca = rng.normal(size=(35, 3)), rng.normal(size=35)
    s = bgm.shifted_cot_alpha(g, ca, b)
    assert np.allclose(s, ca - g @ b, rtol=0, atol=1e-14)
    assert np.array_equal(bgm.shifted_cot_alpha(g, ca, (0, 0, 0)), ca)


# ----------------------------------------------------------------------------------------------------- the step's colour
def test_background_for_is_a_pure_function_of_seed_and_iteration():
    c = bgm.background_for(5, 7)
    assert c.dtype == np.float32 and c.shape == (3,)
    want = np.random.default_rng([5, 7]).random(3, dtype=np.float32)
    assert np.array_equal(c, want)
    table = {(s, t): bgm.background_for(s, t) for s in (0, 5) for t in range(200)}
    allc = np.stack(list(table.values()))
    assert (allc >= 0).all() and (allc < 1).all()
    assert allc.min() < 0.01 and allc.max() > 0.99 and abs(float(allc.mean()) - 0.5) < 0.03
    # the order of the calls does not enter
    for key in reversed(list(table)):
        assert np.array_equal(bgm.background_for(*key), table[key])
    # every (seed, iteration) has a colour of its own
    assert len({v.tobytes() for v in table.values()}) == len(table)
    assert not np.array_equal(bgm.background_for(0, 1), bgm.background_for(1, 0))
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            bgm.background_for(*bad)


def test_config_validate():
    C = bgm.BackgroundConfig
    assert C().validate().mode == "random" and C().seed == 0 and C().color is None
    assert np.array_equal(C(seed=5).color_at(9), bgm.background_for(5, 9))
    f = C(mode="fixed", color=ref.B_OUT).validate()
    assert np.array_equal(f.color_at(0), np.asarray(ref.B_OUT, np.float32)) and np.array_equal(f.color_at(0), f.color_at(31))
    for bad in (C(mode="fixed"), C(mode="random", color=(0, 0, 0)), C(mode="white"), C(mode=None), C(seed=-1), C(seed=1.5),
                C(seed=True), C(mode="fixed", color=(0.1, 0.2)), C(mode="fixed", color=(0.1, 0.2, float("nan"))),
                C(mode="fixed", color=(0.1, 0.2, float("inf"))), C(mode="fixed", color="red"), C(mode="fixed", color=0.5)):
        with pytest.raises(ValueError):
            bad.validate()


# ------------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(background="random"), dict(background=(0.5, 0.5, 0.5)),
                                dict(background=True), dict(background=bgm.BackgroundConfig(mode="fixed")),
                                dict(background=bgm.BackgroundConfig(color=(0, 0, 0)))])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(background=bgm.BackgroundConfig(seed=5))
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_train_step_wants_alpha_with_the_config_and_only_then():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)         # (the check comes before anything of the trainer is touched)
    tr.background = None
    with pytest.raises(ValueError, match="targetAlpha"):
        tr.trainStep(None, None, targetAlpha=np.zeros((2, 2), np.float32))
    tr.background = bgm.BackgroundConfig()
    with pytest.raises(ValueError, match="targetAlpha"):
        tr.trainStep(None, None)


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
        assert e in _lib._SIGS
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+6\b", src)


def test_null_context_and_bad_arguments_are_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    assert lib.gs_set_background(None, None) == invalid
    assert lib.gs_get_background(None, None) == invalid
    assert lib.gs_composite_target(None, 0, None, None, None, None) == invalid
