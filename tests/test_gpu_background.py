"""Background colour on the device (include/gsplat.h gs_set_background / gs_composite_target): every
blend kernel of the library under a colour against the black oracle through the two identities of tests/background_numpy.py,

    colour_b = colour_black + (1 - alpha) b            gradient_b(g, cD, cA) = gradient_black(g, cD, cA - g . b),

that off is off, the latch, the composite kernel and the trainer's step.

Scene: test_gpu_trajectory._scene(71, 3000, 160, 120, 0.03), camera 0 (58.5 % of the pixels have alpha < 0.5: the background
shows; the longest 16 x 16 list has 775 entries against GS_SEG_LEN = 64: the fused backward reconstructs the owed sums from the
stored image behind checkpoints).  Op-level cases: test_gpu_parity._blend_case.  Colours: (0.9, 0.2, 0.55) and, outside the unit
cube, (-0.5, 2.0, 0.0).

Bars, the project's own: images 1e-4 L-inf against the float64 reference (the float32 oracle for the op-level kernels, which
are fed its records), gradients max|a - b| / max|b| <= 1e-3 per tensor, the composite 1e-6 absolute (three float32 roundings of
values <= 1 of at most 6e-8 each).  Under b = (-0.5, 2, 0) the image spans [-0.5, 2] plus the colours: the 1e-4 bar is kept
as it is.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import background as bgm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IMG_BAR, GRAD_BAR, COMPOSITE_BAR = 1e-4, 1e-3, 1e-6


def _load(name):
    spec = importlib.util.spec_from_file_location("_bgg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("background_numpy")
W, H, N, KEYS = ref.W, ref.H, ref.N, ref.KEYS
COLOURS = [ref.B_IN, ref.B_OUT]


def _renderer(tile=(16, 16), white=False, aa=False, w=W, h=H):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, w, h, tile, white, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _perturbed(p):
    from gaussiansplattingmlx_amd.scenes import perturb
    return perturb(p, 5, 0.1)


def _step(r, params, cam, target):
    res = r.renderForward(params, cam)
    img, alpha, depth = res.render.clone(), res.alpha.clone(), res.depth.clone()
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    g = r.renderBackward(cot)
    return img, alpha, depth, float(loss[0]), {k: v.clone() for k, v in g.items()}


# ------------------------------------------------------------------------------------------------------------ the setter
def test_setter_refuses_non_finite_values_and_keeps_the_setting():
    from gaussiansplattingmlx_amd import _lib
    p, cams = ref.scene()
    params = _dev(p)
    r = _renderer()
    invalid = {v: k for k, v in _lib.STATUS.items()}["GS_ERR_INVALID_ARG"]
    assert np.array_equal(r.background, [0, 0, 0])
    assert np.array_equal(_renderer(white=True).background, [1, 1, 1])
    black = r.renderForward(params, cams[0]).render.clone()
    r.setBackground(ref.B_OUT)
    assert np.array_equal(r.background, np.asarray(ref.B_OUT, np.float32))
    on = r.renderForward(params, cams[0]).render.clone()
    assert float((on - black).abs().max()) > 0.5
    for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
        b = np.asarray(bad, np.float32)
        assert r.lib.gs_set_background(r.ctx, b.ctypes.data) == invalid
        assert "gs_set_background" in r.lib.gs_last_error(r.ctx).decode()
        assert np.array_equal(r.background, np.asarray(ref.B_OUT, np.float32))       # kept
    assert torch.equal(r.renderForward(params, cams[0]).render, on)
    with pytest.raises(ValueError):
        r.setBackground((0.1, 0.2))
    r.setBackground(ref.B_IN)
    assert np.array_equal(r.background, np.asarray(ref.B_IN, np.float32))
    r.setBackground(None)
    assert np.array_equal(r.background, [0, 0, 0])
    assert torch.equal(r.renderForward(params, cams[0]).render, black)
    # (0, 0, 0) as a colour is the black render, through the colour path
    r.setBackground((0.0, 0.0, 0.0))
    assert torch.equal(r.renderForward(params, cams[0]).render, black)
    assert r.lib.gs_composite_target(r.ctx, -1, black.data_ptr(), black.data_ptr(), np.zeros(3, np.float32).ctypes.data,
                                     black.data_ptr()) == invalid
    assert r.lib.gs_composite_target(r.ctx, 4, None, black.data_ptr(), np.zeros(3, np.float32).ctypes.data, black.data_ptr()) == invalid
    assert "gs_composite_target" in r.lib.gs_last_error(r.ctx).decode()


@pytest.mark.parametrize("white", [False, True])
def test_off_is_off(white):
    """A context that had a colour and then None renders and differentiates like a fresh one, bit for bit (where the fresh one
    is itself run-to-run identical: the blend backward's float atomics are not on every scene)."""
    p, cams = ref.scene()
    params = _dev(p)
    fresh = _renderer(white=white)
    target = fresh.renderForward(_dev(_perturbed(p)), cams[1]).render.clone()
    a = _step(fresh, params, cams[0], target)
    b = _step(fresh, params, cams[0], target)
    r = _renderer(white=white)
    r.setBackground(ref.B_IN)
    coloured = _step(r, params, cams[0], target)
    assert not torch.equal(coloured[0], a[0])
    r.setBackground(None)
    c = _step(r, params, cams[0], target)
    for i in range(3):
        assert torch.equal(a[i], c[i]), i
    assert a[3] == c[3]
    for k in KEYS:
        if torch.equal(a[4][k], b[4][k]):
            assert torch.equal(a[4][k], c[4][k]), k
        else:
            assert torch.allclose(a[4][k], c[4][k], rtol=1e-5, atol=1e-7 * float(a[4][k].abs().max())), k


def test_backward_uses_its_forwards_background():
    p, cams = ref.scene()
    params = _dev(p)
    r = _renderer()
    r.setBackground(ref.B_IN)
    target = torch.zeros(H, W, 3, device="cuda")
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    want = {k: v.clone() for k, v in r.renderBackward(cot).items()}
    res = r.renderForward(params, cams[0])
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.setBackground(ref.B_OUT)       # between the forward and its backward: changes nothing for that pair
    got = {k: v.clone() for k, v in r.renderBackward(cot).items()}
    for k in KEYS:
        assert _rel(_np(got[k]), _np(want[k])) <= 1e-5, k
    # ... where a backward under the other colour is somewhere else altogether
    res = r.renderForward(params, cams[0])
    other = r.renderBackward(cot)
    assert _rel(_np(other["opacity"]), _np(want["opacity"])) > 1e-2


# ------------------------------------------------------------------------------------------------------ forward parity
@pytest.mark.parametrize("b", COLOURS)
@pytest.mark.parametrize("variant", ["one_wave", "pair", "four_waves", "untrimmed", "block_lists"])
def test_forward_matches_the_identity(oracle64, variant, b):
    p, cams = ref.scene()
    tile = (50, 38) if variant == "block_lists" else (16, 16)
    fw = ref.forward(oracle64, tile)
    assert abs(float((fw["alpha"] < 0.5).mean()) - 0.585) < 0.001 and abs(float((fw["alpha"] > 0.95).mean()) - 0.307) < 0.001
    want, alpha, depth = ref.render_under(oracle64, b, tile)
    r = _renderer(tile)
    assert r.blockLists == (variant == "block_lists")
    knobs = dict(one_wave=dict(fwd_four_waves=0, fwd_pair=0), pair=dict(fwd_four_waves=0, fwd_pair=1),
                 four_waves=dict(fwd_four_waves=1), untrimmed=dict(trim_rects=0), block_lists={})[variant]
    r.setTuning(**knobs)
    r.setBackground(b)
    params = _dev(p)
    res = r.renderForward(params, cams[0])
    err = np.abs(_np(res.render).reshape(-1, 3) - want).max()
    print(f"{variant} {b}: image against the float64 identity {err:.3e} (bar {IMG_BAR:.0e})")
    assert err <= IMG_BAR
    assert np.abs(_np(res.alpha).reshape(-1) - alpha).max() <= IMG_BAR
    assert np.abs(_np(res.depth).reshape(-1) - depth).max() <= IMG_BAR * max(1.0, float(np.abs(depth).max()))
    nod = r.renderForward(params, cams[0], wantDepth=False)
    assert nod.depth is None
    assert np.abs(_np(nod.render).reshape(-1, 3) - want).max() <= IMG_BAR
    # the colour is what is seen where nothing is: an uncovered pixel holds b (alpha == 0 in float32 is 1 - T < 6e-8, so what
    # was blended there is below 6e-8 times the largest colour, and T b is b)
    empty = np.nonzero((fw["alpha"].reshape(-1) == 0) & (_np(nod.alpha).reshape(-1) == 0))[0]
    assert len(empty) > 100
    assert np.abs(_np(nod.render).reshape(-1, 3)[empty] - np.asarray(b, np.float32)).max() <= 1e-6


# ----------------------------------------------------------------------------------------------------- op-level parity
_cases = {}


def _blend_case(oracle32, w, h, tile):
    """test_gpu_parity._blend_case over black, computed once per shape."""
    if (w, h, tile) not in _cases:
        _cases[(w, h, tile)] = _load("test_gpu_parity")._blend_case(oracle32, w, h, tile, False)
    return _cases[(w, h, tile)]


def _target64(oracle64, tile):
    if ("target", tile) not in _cases:
        p, cams = ref.scene()
        _cases[("target", tile)] = oracle64.render_forward(_perturbed(p), cams[0].as_dict(), W, H, tile[0], tile[1], 4)["color"].reshape(H, W, 3)
    return _cases[("target", tile)]


@pytest.mark.parametrize("b", COLOURS)
@pytest.mark.parametrize("w,h,tile", [(200, 152, (16, 16)), (128, 96, (32, 32))])          # (32, 32): the cull kernels
@pytest.mark.parametrize("ppl", [1, 2, 4])
def test_blend_ops_match_the_identity(oracle32, w, h, tile, ppl, b):
    p, c, fw = _blend_case(oracle32, w, h, tile)
    pr, bn = fw["proj"], fw["bin"]
    r = _renderer(tile, w=w, h=h)
    r.setTuning(op_fwd_ppl=ppl, op_bwd_ppl=ppl)
    r.setBackground(b)
    r.buildGlobalTileSliceInfo((pr["rectMin"], pr["rectMax"]), pr["radii"], pr["depths"])
    color, depth, alpha = r.globalTileComposite(fw["packed"])
    want = bgm.with_background(fw["color"], fw["alpha"], b)
    assert want.dtype == np.float32
    assert np.abs(_np(color) - want).max() <= IMG_BAR
    assert np.abs(_np(alpha) - fw["alpha"]).max() <= IMG_BAR
    np.testing.assert_allclose(_np(depth), fw["depth"], rtol=1e-4, atol=1e-4)
    rng = np.random.default_rng(8)
    cC = rng.normal(size=(w * h, 3)).astype(np.float32)
    cD = (rng.normal(size=w * h) * 0.1).astype(np.float32)
    cA = rng.normal(size=w * h).astype(np.float32)
    # same saved forward state on both sides: the oracle's (the blend backward reads alpha and nContrib, not the colour)
    saved = dict(packed=r._t(fw["packed"]), color=r._t(want), depth=r._t(fw["depth"]), alpha=r._t(fw["alpha"]),
                 last=torch.as_tensor(fw["last"].astype(np.int32), device=r.device))
    got = _np(r.globalTileCompositeVJP(cC, cD, cA, saved=saved))

    def black(ca):
        return oracle32.blend_backward(fw["packed"], bn.sortedIdx, bn.tileRanges, w, h, tile[0], tile[1], False, cC, cD, ca,
                                       fw["color"], fw["depth"], fw["alpha"], fw["last"])
    wantg, plain = black(bgm.shifted_cot_alpha(cC, cA, b)), black(cA)
    assert _rel(wantg[:, 9], plain[:, 9]) > 1e-2               # (the colour matters, from the reference alone)
    for col in range(11):
        assert _rel(got[:, col], wantg[:, col]) <= GRAD_BAR, col


# ------------------------------------------------------------------------------------------------ fused gradient parity
@pytest.mark.parametrize("b", COLOURS)
@pytest.mark.parametrize("tile", [(16, 16), (50, 38)])
def test_gradients_match_the_composed_oracle(oracle64, tile, b):
    p, cams = ref.scene()
    cam = cams[0].as_dict()
    fw = ref.forward(oracle64, tile)
    assert int(ref.list_lengths(fw).max()) == (775 if tile == (16, 16) else 2236)
    target = _target64(oracle64, tile)
    want_loss, fwl, cot = ref.loss_under(oracle64, p, cam, W, H, target, b, tile)
    want = ref.backward_under(oracle64, b, cot, None, None, tile)
    black = ref.backward_under(oracle64, (0, 0, 0), cot, None, None, tile)
    assert np.abs(want["opacity"] - black["opacity"]).max() > 1e-2 * np.abs(want["opacity"]).max()
    r = _renderer(tile)
    r.setBackground(b)
    _, _, _, loss, g = _step(r, _dev(p), cams[0], torch.as_tensor(target, dtype=torch.float32, device="cuda"))
    assert abs(loss - want_loss) <= 1e-5
    for k in KEYS:
        err = _rel(_np(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1))
        print(f"{tile} {b} {k}: gradient against the float64 composed oracle {err:.3e} (bar {GRAD_BAR:.0e})")
        assert err <= GRAD_BAR, k


def test_fused_adam_matches_backward_then_adam():
    """gs_render_backward_adam == gs_render_backward + gs_adam_step under a colour (test_gpu_parity's check, through the
    trainer, the colour set on the renderer)."""
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = ref.scene()
    r = _renderer()
    r.setBackground(ref.B_IN)
    target = torch.rand(H, W, 3, device=r.device, generator=torch.Generator(device=r.device).manual_seed(3))
    out = {}
    for fuse in (False, True):
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, fuse_adam=fuse)
        for _ in range(3):
            tr.trainStep(cams[0], target)
        out[fuse] = (_np(model.arena).copy(), _np(model.m).copy(), _np(model.v).copy())
    assert np.array_equal(r.background, np.asarray(ref.B_IN, np.float32))
    start = _np(GaussModel(p, r.device).arena)
    a, b = out[True][0] - start, out[False][0] - start
    assert np.abs(b).max() > 0
    assert np.mean(np.abs(a - b) > 1e-3 * np.abs(b).max()) < 1e-3
    for k in (1, 2):
        want = out[False][k]
        assert np.mean(np.abs(out[True][k] - want) > 1e-3 * np.abs(want).max()) < 1e-3, k


# --------------------------------------------------------------------------------------------------------------- AbsGS
def test_absgrad_composes(oracle64):
    """absgrad() under a colour against the float64 rule on the BLACK forward under the shifted alpha cotangent."""
    from gaussiansplattingmlx_amd import absgrad as ag
    p, cams = ref.scene()
    b = ref.B_IN
    fw = ref.forward(oracle64)
    bn = fw["bin"]
    cot = np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)
    ca = np.random.default_rng(5).standard_normal((H, W)) / (W * H)
    A64, _ = ag.blend_absgrad(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, 16, 16, cot, fw["color"], fw["last"],
                              cotAlpha=bgm.shifted_cot_alpha(cot, ca, b), outAlpha=fw["alpha"])
    A0, _ = ag.blend_absgrad(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, 16, 16, cot, fw["color"], fw["last"],
                             cotAlpha=ca, outAlpha=fw["alpha"])
    assert _rel(A64, A0) > 1e-2
    r = _renderer()
    r.setAbsgrad(True)
    r.setBackground(b)
    r.renderChecked(_dev(p), cams[0], wantDepth=False)
    r.renderBackward(_t(cot), None, _t(ca))
    got = _np(r.absgrad())
    for col in range(2):
        err = _rel(got[:, col], A64[:, col])
        print(f"column {col}: device against float64 {err:.3e} (bar 1e-3)")
        assert err <= 1e-3


# ------------------------------------------------------------------------------------------------------- the composite
@pytest.mark.parametrize("n", [1, 63, 64, 65, W * H])
def test_composite_target(n):
    r = _renderer()
    rng = np.random.default_rng(n)
    rgb, a = rng.random((n, 3), dtype=np.float32), rng.random(n, dtype=np.float32)
    a[:: 7] = 0.0
    a[3:: 7] = 1.0
    for b in COLOURS + [tuple(bgm.background_for(5, 0))]:
        want = bgm.composite(rgb, a, np.asarray(b, np.float32))
        trgb, ta = _t(rgb), _t(a)
        got = r.compositeTarget(trgb, ta, b)
        assert got.shape == (n, 3) and torch.equal(trgb, _t(rgb))
        assert np.abs(_np(got) - want).max() <= COMPOSITE_BAR
        assert r.compositeTarget(trgb, ta, b, out=trgb) is trgb
        assert torch.equal(trgb, got)                                  # in place: the same bits
    img = r.compositeTarget(_t(rng.random((3, 5, 3), dtype=np.float32)), _t(np.zeros((3, 5), np.float32)), ref.B_IN)
    assert img.shape == (3, 5, 3) and torch.equal(img, _t(np.broadcast_to(np.asarray(ref.B_IN, np.float32), (3, 5, 3))))
    with pytest.raises(ValueError):
        r.compositeTarget(_t(rgb), _t(a[:-1]) if n > 1 else _t(np.zeros(2, np.float32)), ref.B_IN)


# ---------------------------------------------------------------------------------------------------------- the trainer
def _rgba_target(r, p, cam):
    """An RGBA view: the render of a perturbed model over black, un-premultiplied by its alpha."""
    res = r.renderForward(_dev(_perturbed(p)), cam)
    alpha = res.alpha.reshape(H, W).clone()
    rgb = (res.render.reshape(H, W, 3) / alpha.clamp_min(1e-3)[..., None]).clamp(0.0, 1.0).contiguous()
    return rgb, alpha


def _trainer(r, p, **kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    model = GaussModel(p, r.device)
    kw.setdefault("densify", False)
    return GaussianTrainer(model, r, iterationCount=1000, **kw), model


def test_one_step_is_the_manual_sequence():
    from gaussiansplattingmlx_amd.trainer import getLearningRates
    p, cams = ref.scene()
    r = _renderer()
    rgb, alpha = _rgba_target(r, p, cams[1])
    r.setBackground(ref.B_OUT)                       # the renderer's own setting: put back behind the step
    tr, model = _trainer(r, p, background=bgm.BackgroundConfig(seed=5))
    loss = tr.trainStep(cams[0], rgb, targetAlpha=alpha)
    b = bgm.background_for(5, 0)
    assert np.array_equal(tr.lastBackground, b)
    assert np.array_equal(r.background, np.asarray(ref.B_OUT, np.float32))
    got = [_np(x).copy() for x in (model.arena, model.m, model.v)]
    # by hand
    from gaussiansplattingmlx_amd.trainer import GaussModel
    m2 = GaussModel(p, r.device)
    r2 = _renderer()
    r2.setTuning(depth_gradient=0)
    r2.setBackground(b)
    target = r2.compositeTarget(rgb, alpha, b)
    assert np.abs(_np(target) - bgm.composite(_np(rgb), _np(alpha), b)).max() <= COMPOSITE_BAR
    res = r2.renderForward(m2.getParams(), cams[0], wantDepth=False)
    loss2, cot, _ = r2.lossForwardBackward(res.render, target, 0.2)
    r2.renderBackwardAdam(cot, m2.arena, m2.m, m2.v, getLearningRates(0, 1000))
    assert float(loss[0]) == float(loss2[0])
    start = _np(GaussModel(p, r.device).arena)
    for name, a, w in zip(("arena", "m", "v"), got, (m2.arena, m2.m, m2.v)):
        w = _np(w)
        assert np.abs(w).max() > 0
        if name == "arena":
            # Adam's step is lr m / sqrt(v): on the first step +-3.16 lr whatever the gradient's size, so an element whose
            # gradient is within the atomics' noise of zero may step the other way in two runs of the SAME sequence; no
            # element-wise bound holds there.  The parameters are held to the project's measure for two device runs of a step
            # (test_fused_adam_matches_backward_then_adam), the moments, which are linear in the gradient, to off-is-off's rtol.
            a, w = a - start, w - start
            share = float(np.mean(np.abs(a - w) > 1e-3 * np.abs(w).max()))
            print(f"parameters: share of elements further than 1e-3 max|step| from the manual sequence {share:.2e} (bar 1e-3)")
            assert share < 1e-3
        else:
            assert np.allclose(a, w, rtol=1e-5, atol=1e-7 * float(np.abs(w).max())), name
    # the next step takes the next colour, and a restart sees the same ones
    tr.trainStep(cams[0], rgb, targetAlpha=alpha)
    assert np.array_equal(tr.lastBackground, bgm.background_for(5, 1)) and not np.array_equal(tr.lastBackground, b)
    with pytest.raises(ValueError):
        tr.trainStep(cams[0], rgb)
    tr0, _ = _trainer(r, p)
    with pytest.raises(ValueError):
        tr0.trainStep(cams[0], rgb, targetAlpha=alpha)
    r.setBackground(None)
    trf, _ = _trainer(r, p, background=bgm.BackgroundConfig(mode="fixed", color=ref.B_IN))
    trf.trainStep(cams[0], rgb, targetAlpha=alpha, viewKey=0)
    assert np.array_equal(trf.lastBackground, np.asarray(ref.B_IN, np.float32)) and np.array_equal(r.background, [0, 0, 0])


def test_target_statistics_cache_under_a_background():
    """Random mode never hands the loss a target key (the trainer's one buffer keeps its address and its tensor version while
    its image changes every step: a cached statistic would be served for ever); fixed mode keeps one entry per (view, image,
    colour), and another image behind the same view key is a miss, not a stale hit."""
    p, cams = ref.scene()
    r = _renderer()
    rgb, alpha = _rgba_target(r, p, cams[1])
    tr, _ = _trainer(r, p, background=bgm.BackgroundConfig(seed=4))
    for _ in range(2):
        tr.trainStep(cams[0], rgb, targetAlpha=alpha, viewKey=0)
    assert len(r._target_cache) == 0
    cfg = bgm.BackgroundConfig(mode="fixed", color=ref.B_IN)
    rgb2 = (1.0 - rgb).contiguous()
    losses = {}
    for cached in (True, False):
        rr = _renderer()
        rr.targetStatsCache = cached
        trf, _ = _trainer(rr, p, background=cfg)
        trf.trainStep(cams[0], rgb, targetAlpha=alpha, viewKey=0)
        trf.trainStep(cams[0], rgb, targetAlpha=alpha, viewKey=0)
        assert len(rr._target_cache) == (1 if cached else 0)
        losses[cached] = float(trf.trainStep(cams[0], rgb2, targetAlpha=alpha, viewKey=0)[0])      # another image, the same key
        assert len(rr._target_cache) == (2 if cached else 0)
    # (the two runs differ by the blend backward's atomics in two Adam steps; statistics of the wrong image move the loss by tens of per cent)
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses


def test_fused_and_unfused_agree():
    p, cams = ref.scene()
    r = _renderer()
    rgb, alpha = _rgba_target(r, p, cams[1])
    out = {}
    for fuse in (False, True):
        tr, model = _trainer(r, p, background=bgm.BackgroundConfig(seed=2), fuse_adam=fuse)
        for _ in range(3):
            tr.trainStep(cams[0], rgb, targetAlpha=alpha)
        out[fuse] = (_np(model.arena).copy(), _np(model.m).copy(), _np(model.v).copy())
    from gaussiansplattingmlx_amd.trainer import GaussModel
    start = _np(GaussModel(p, r.device).arena)
    a, b = out[True][0] - start, out[False][0] - start
    assert np.abs(b).max() > 0
    assert np.mean(np.abs(a - b) > 1e-3 * np.abs(b).max()) < 1e-3
    for k in (1, 2):
        want = out[False][k]
        assert np.mean(np.abs(out[True][k] - want) > 1e-3 * np.abs(want).max()) < 1e-3, k


def test_training_on_rgba_views_reduces_the_loss():
    p, cams = ref.scene()
    r = _renderer()
    views = [_rgba_target(r, p, c) for c in cams]
    assert float((views[0][1] < 0.5).float().mean()) > 0.3           # (transparent pixels: the background shows in the target)
    tr, model = _trainer(r, p, background=bgm.BackgroundConfig(seed=1))
    losses = []
    for it in range(30):
        v = it % len(cams)
        losses.append(float(tr.trainStep(cams[v], views[v][0], targetAlpha=views[v][1], viewKey=v)[0]))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-6:]) < 0.8 * np.mean(losses[:6]), losses
    assert np.array_equal(r.background, [0, 0, 0]) and torch.isfinite(model.arena).all()


@pytest.mark.parametrize("variant", ["exposure_sparse", "mcmc"])
def test_composes_with_the_other_step_features(variant):
    p, cams = ref.scene()
    r = _renderer(aa=variant == "mcmc")
    views = [_rgba_target(r, p, c) for c in cams]
    if variant == "mcmc":
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=int(N * 1.2)))
    else:
        kw = dict(exposure_opt=True, sparse_adam=True, n_views=len(cams))
    tr, model = _trainer(r, p, background=bgm.BackgroundConfig(seed=3), **kw)
    for it in range(10):
        v = it % len(cams)
        loss = tr.trainStep(cams[v], views[v][0], targetAlpha=views[v][1], viewKey=v)
        assert np.isfinite(float(loss[0]))
        assert np.array_equal(tr.lastBackground, bgm.background_for(3, it))
    assert torch.isfinite(model.arena[: model.numel]).all() and np.array_equal(r.background, [0, 0, 0])
