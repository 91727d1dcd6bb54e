"""N-channel feature rendering on the device (include/gsplat.h gs_blend_features / gs_render_features and their _backward,
features.FeatureField) against gaussiansplattingmlx_amd/features.py in float64 on the oracle's lists.

Bars, fixed before the first run on the card.  Features and cotangents are drawn uniformly in [-1, 1], so |out| <= 1.
  forward   1e-4 absolute -- the project's image bar: the image is a sum of the same weights as the colour image, against
            payloads of magnitude <= 1; it also covers a pixel whose stop falls one entry later in float32 (the entry behind a
            stop weighs less than T_STOP = 1e-4).
  gradient  test_gpu_parity's gradient metric, max |a - b| / max |b| <= 1e-3: a per-Gaussian sum over pixels accumulated with
            float atomics.
  Occluded and off-screen Gaussians: gradient rows exactly 0.  Pixels whose list is empty: exactly 0, and no pixel of an
            image pre-filled with NaN is left unwritten.
  Device adjoint identity: |<cot, out> - <grad, f>| / sum |cot out| <= 1e-3, the sums in float64 on the host.
  Gradients of renderBackward after a feature pass: 1e-3 in the gradient metric, against the gradients taken without it.
  Training: the per-step loss within max(4 d32[k], 1e-6) relative of the float64 host loop, d32 the float32 host loop's
            distance from it (the factor 4: the device's different summation order on top of the format).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import features as ft

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
FWD_BAR, GRAD_BAR, ADJ_BAR = 1e-4, 1e-3, 1e-3
W, H = 160, 120
G = ft.CHANNEL_GROUP
CHANNELS = (1, 3, G - 1, G, G + 1, 2 * G + 3)


def _load(name):
    spec = importlib.util.spec_from_file_location("_ftg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gcp = _load("test_gpu_contrib_prune")
fcpu = _load("test_features_cpu")
cpu, traj, aacpu = gcp.cpu, gcp.traj, gcp.aacpu
_renderer, _dev, _np, _rel = gcp._renderer, gcp._dev, gcp._np, gcp._rel


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _draw(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def _check(tag, out, grad, want_out, want_grad):
    ef = np.abs(_np(out).astype(np.float64) - want_out).max()
    eg = _rel(_np(grad), want_grad)
    print(f"{tag}: forward err {ef:.3e} (bar {FWD_BAR:.0e}), gradient rel {eg:.3e} (bar {GRAD_BAR:.0e})")
    assert ef <= FWD_BAR
    assert eg <= GRAD_BAR


# --------------------------------------------------------------------------------------------------------- 1. op level
_op_cache = {}


def _op_case(name, oracle64):
    if name not in _op_cache:
        c, s, bn, _ = gcp._op_case(name, oracle64)
        lists = (s["packed"], bn.sortedIdx, bn.tileRanges, c["W"], c["H"], c["tile"][0], c["tile"][1])
        _op_cache[name] = (c, s, bn, lists, ft.tile_weights(*lists))
    return _op_cache[name]


def _bin(r, s, bn):
    info = r.buildGlobalTileSliceInfo((s["rectMin"], s["rectMax"]), s["radii"], s["depths"])
    if bn is not None:        # both sides sweep identical lists
        assert np.array_equal(_np(info["sortedGaussIdx"]).astype(np.uint32), bn.sortedIdx)
        assert np.array_equal(_np(info["tileRanges"]).astype(np.uint32), bn.tileRanges)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("name", list(gcp.OP_CASES))
def test_op_level_matches_float64(oracle64, name, C):
    c, s, bn, lists, weights = _op_case(name, oracle64)
    if name == "deep_lists":      # longer than one LDS chunk, and the pixels stop inside the list
        first_layer = int(np.where(s["packed"][:, 9] == np.float32(0.95))[0][0])
        pos = [int(np.where(bn.sortedIdx[a:b] == first_layer)[0][0]) for a, b in bn.tileRanges]
        assert min(pos) > 256 and bn.B > max(pos) + 256
    f, cot = _draw(11 * C, c["N"], C), _draw(11 * C + 1, c["H"], c["W"], C)
    want_out = ft.blend_features(*lists, f, weights=weights)
    want_grad = ft.blend_features_vjp(*lists, cot, weights=weights)
    r = _renderer(c["W"], c["H"], c["tile"])
    _bin(r, s, bn)
    out = torch.full((c["H"], c["W"], C), float("nan"), device="cuda")
    assert r.blendFeatures(s["packed"], _cuda(f), out) is out
    assert not bool(out.isnan().any())                                # every pixel is written
    grad = r.blendFeaturesVJP(s["packed"], _cuda(cot))
    assert tuple(grad.shape) == (c["N"], C)
    _check(f"{name} C={C}", out, grad, want_out, want_grad)
    for what in ("occluded", "offscreen"):
        assert not want_grad[s[what]].any()
        assert not bool(grad[torch.as_tensor(s[what], device="cuda")].any()), what
    assert float(grad[s["spanning"]].abs().max()) > 0


def test_pixels_outside_every_list_are_written_as_zeros(oracle64):
    """Only two splats keep a radius, both in the top left tile: every other tile of the 48 x 40 image (partial blocks at both
    edges) has an empty list."""
    Wc, Hc, N, C = 48, 40, 300, G + 1
    s = dict(cpu.op_scene(Wc, Hc, N, seed=17))
    radii = np.zeros_like(s["radii"])
    radii[[1, 4]] = s["radii"][[1, 4]]
    s["radii"] = radii
    s["rectMin"] = (s["packed"][:, 0:2] - radii[:, None]).astype(np.float32)
    s["rectMax"] = (s["packed"][:, 0:2] + radii[:, None]).astype(np.float32)
    bn = oracle64.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], Wc, Hc, 16, 16)
    lists = (s["packed"], bn.sortedIdx, bn.tileRanges, Wc, Hc, 16, 16)
    empty = np.zeros((Hc, Wc), bool)
    for t, (a, b) in enumerate(bn.tileRanges):
        if b <= a:
            ty, tx = divmod(t, 3)
            empty[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    assert 0 < empty.sum() < Wc * Hc and empty[Hc - 1].all() and empty[:, Wc - 1].all()
    f = _draw(5, N, C)
    r = _renderer(Wc, Hc)
    _bin(r, s, bn)
    out = torch.full((Hc, Wc, C), float("nan"), device="cuda")
    r.blendFeatures(s["packed"], _cuda(f), out)
    got = _np(out)
    assert not np.isnan(got).any()
    assert not got[empty].any()
    assert np.abs(got - ft.blend_features(*lists, f)).max() <= FWD_BAR and np.abs(got).max() > 0.01


def test_offsets_beyond_2_31_elements(oracle64):
    """2944 x 2944 x 256 floats: the image has more than 2^31 elements, and every splat sits in its last 64 x 48 pixels, whose
    offsets into out and cot lie beyond that.  The float64 model is evaluated on the tiles that have lists."""
    Wb = Hb = 2944
    C, N = ft.MAX_CHANNELS, 60
    s = dict(cpu.op_scene(64, 48, N, seed=3))
    shift = np.array([Wb - 64, Hb - 48], np.float32)
    packed = s["packed"].copy()
    packed[:, 0:2] += shift
    s.update(packed=packed, rectMin=s["rectMin"] + shift, rectMax=s["rectMax"] + shift)
    bn = oracle64.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], Wb, Hb, 16, 16)
    weights = ft.tile_weights(packed, bn.sortedIdx, bn.tileRanges, Wb, Hb, 16, 16)
    y0, x0 = min(t[0][0] for t in weights), min(t[1][0] for t in weights)
    assert ((Hb - 48) * Wb + Wb - 64) * C > 2 ** 31                               # the splats' own pixels lie beyond
    f = _draw(21, N, C)
    r = _renderer(Wb, Hb)
    _bin(r, s, bn)
    out = torch.full((Hb, Wb, C), float("nan"), device="cuda")
    r.blendFeatures(packed, _cuda(f), out)
    assert not bool(out.isnan().any())
    assert not bool(out[:y0].any()) and not bool(out[:, :x0].any())
    cot = torch.rand(Hb, Wb, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)) * 2 - 1
    grad = r.blendFeaturesVJP(packed, cot)
    got, ct = _np(out[y0:, x0:]).astype(np.float64), _np(cot[y0:, x0:]).astype(np.float64)
    want_grad, err = np.zeros((N, C)), 0.0
    for ys, xs, g, w in weights:
        rows, cols = slice(ys[0] - y0, ys[-1] + 1 - y0), slice(xs[0] - x0, xs[-1] + 1 - x0)
        err = max(err, np.abs(got[rows, cols] - np.einsum("jyx,jc->yxc", w, f[g].astype(np.float64))).max())
        np.add.at(want_grad, g, np.einsum("jyx,yxc->jc", w, ct[rows, cols]))
    eg = _rel(_np(grad), want_grad)
    print(f"2944 x 2944 x 256: forward err {err:.3e} (bar {FWD_BAR:.0e}), gradient rel {eg:.3e} (bar {GRAD_BAR:.0e})")
    assert err <= FWD_BAR and eg <= GRAD_BAR and np.abs(want_grad).max() > 1.0


# ------------------------------------------------------------------------------------- 2. cross-checks that need no model
def test_three_channels_are_the_colour_image_and_ones_are_alpha(oracle64):
    c, s, bn, lists, _ = _op_case("partial_blocks", oracle64)
    r = _renderer(c["W"], c["H"], c["tile"])
    _bin(r, s, bn)
    color = r.globalTileComposite(s["packed"])[0].clone()             # (a black background)
    out = r.blendFeatures(s["packed"], _cuda(s["packed"][:, 6:9]))
    err = float((out.reshape(-1, 3) - color).abs().max())
    print(f"C = 3 against globalTileComposite: {err:.3e}")
    assert err <= FWD_BAR and float(color.max()) > 0.1
    p, cams = gcp._scene()
    r = _renderer(W, H)
    res = r.renderChecked(_dev(p), cams[0])
    ones = r.renderFeatures(torch.ones(3000, 1, device="cuda"))
    err = float((ones - res.alpha).abs().max())
    print(f"C = 1 ones against the fused alpha: {err:.3e}")
    assert err <= FWD_BAR and float(res.alpha.max()) > 0.5


# -------------------------------------------------------------------------------------------------------- 3. fused path
_fused_cache = {}


def _want_fused(oracle64, variant, tile=(16, 16)):
    key = (variant, tile)
    if key not in _fused_cache:
        p, cams = gcp._scene()
        o = aacpu.AAOracle(oracle64) if variant == "aa" else oracle64
        fw = o.render_forward(p, cams[0].as_dict(), W, H, tile[0], tile[1], 4)
        lists = (fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, tile[0], tile[1])
        C = G + 1
        f, cot = _draw(41, 3000, C), _draw(42, H, W, C)
        weights = ft.tile_weights(*lists)
        _fused_cache[key] = (fw, f, cot, ft.blend_features(*lists, f, weights=weights),
                             ft.blend_features_vjp(*lists, cot, weights=weights))
    return _fused_cache[key]


@pytest.mark.parametrize("variant", ["plain", "aa"])
def test_fused_matches_float64(oracle64, variant):
    p, cams = gcp._scene()
    fw, f, cot, want_out, want_grad = _want_fused(oracle64, variant)
    r = _renderer(W, H, aa=variant == "aa")
    r.renderChecked(_dev(p), cams[0])
    out = r.renderFeatures(_cuda(f), torch.full((H, W, G + 1), float("nan"), device="cuda"))
    grad = r.renderFeaturesVJP(_cuda(cot))
    _check("fused " + variant, out, grad, want_out, want_grad)
    unseen = ~want_grad.any(axis=1)
    assert unseen.sum() > 0 and not bool(grad[torch.as_tensor(unseen, device="cuda")].any())
    if variant != "plain":        # (the mode matters on this scene)
        assert np.abs(_want_fused(oracle64, "plain")[3] - want_out).max() > 10 * FWD_BAR


def test_fused_on_block_lists(oracle64):
    """A tile size that is not a multiple of 16: the fused path's block lists, and the op-level form at that tile size."""
    p, cams = gcp._scene()
    fw, f, cot, want_out, want_grad = _want_fused(oracle64, "plain", (50, 38))
    r = _renderer(W, H, (50, 38))
    assert r.blockLists
    r.renderChecked(_dev(p), cams[0])
    out = r.renderFeatures(_cuda(f), torch.full((H, W, G + 1), float("nan"), device="cuda"))
    grad = r.renderFeaturesVJP(_cuda(cot))
    _check("fused block lists", out, grad, want_out, want_grad)
    pr = fw["proj"]
    r.buildGlobalTileSliceInfo((pr["rectMin"], pr["rectMax"]), pr["radii"], pr["depths"])
    out2 = r.blendFeatures(fw["packed"], _cuda(f), torch.full((H, W, G + 1), float("nan"), device="cuda"))
    grad2 = r.blendFeaturesVJP(fw["packed"], _cuda(cot))
    _check("op level 50x38", out2, grad2, want_out, want_grad)


# ------------------------------------------------------------------------------------- 4. determinism and accumulation
def test_forward_is_bit_identical_and_backward_accumulates(oracle64):
    c, s, bn, lists, _ = _op_case("deep_lists", oracle64)
    C = G + 1
    f, cot = _cuda(_draw(7, c["N"], C)), _cuda(_draw(8, c["H"], c["W"], C))
    r = _renderer(c["W"], c["H"], c["tile"])
    _bin(r, s, bn)
    a = r.blendFeatures(s["packed"], f)
    _bin(r, s, None)
    b = r.blendFeatures(s["packed"], f)
    assert torch.equal(a, b)                                          # two runs: the same bits
    grad = r.blendFeaturesVJP(s["packed"], cot)
    first = grad.clone()
    assert r.blendFeaturesVJP(s["packed"], cot, grad) is grad         # once more into the same buffer
    assert _rel(_np(grad), 2.0 * _np(first).astype(np.float64)) <= GRAD_BAR
    kept = torch.full((c["N"], C), 2.0, device="cuda")
    r.blendFeaturesVJP(s["packed"], cot, kept)
    untouched = torch.as_tensor(s["occluded"] | s["offscreen"], device="cuda")
    assert bool((kept[untouched] == 2.0).all())
    assert _rel(_np(kept - 2.0), _np(first)) <= GRAD_BAR


# ---------------------------------------------------------------------------------------------- 5. device adjoint identity
@pytest.mark.parametrize("C", [1, G + 1])
def test_device_adjoint_identity(C):
    p, cams = gcp._scene()
    r = _renderer(W, H)
    r.renderChecked(_dev(p), cams[0])
    f, cot = _draw(61 + C, 3000, C), _draw(62 + C, H, W, C)
    out = _np(r.renderFeatures(_cuda(f))).astype(np.float64)
    grad = _np(r.renderFeaturesVJP(_cuda(cot))).astype(np.float64)
    lhs, rhs, scale = (cot * out).sum(), (grad * f).sum(), np.abs(cot * out).sum()
    print(f"C = {C}: <cot, out> = {lhs:.6f}, <grad, f> = {rhs:.6f}, relative {abs(lhs - rhs) / scale:.3e} (bar {ADJ_BAR:.0e})")
    assert scale > 1.0 and abs(lhs - rhs) / scale <= ADJ_BAR


# ------------------------------------------------------------------------------------------- 6. leaves the forward usable
def test_feature_passes_leave_the_forward_usable():
    p, cams = gcp._scene()
    r = _renderer(W, H)
    params = _dev(p)
    target = torch.rand(H, W, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    f, fcot = _cuda(_draw(1, 3000, G + 1)), _cuda(_draw(2, H, W, G + 1))

    def step(features):
        res = r.renderChecked(params, cams[0])
        img, alpha, stats = res.render.clone(), res.alpha.clone(), r.stats()
        _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
        cot = cot.clone()
        if features:
            first = r.renderFeatures(f)
            r.renderFeaturesVJP(fcot)
            assert torch.equal(r.renderFeatures(f), first)            # further feature calls on the same forward
            assert torch.equal(res.render, img) and torch.equal(res.alpha, alpha) and r.stats() == stats
        return img, {k: v.clone() for k, v in r.renderBackward(cot).items()}
    img0, g0 = step(False)
    img1, g1 = step(True)
    assert torch.equal(img0, img1)
    for k in KEYS:
        assert _rel(_np(g1[k]), _np(g0[k])) <= GRAD_BAR, k


# ---------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(oracle64):
    from gaussiansplattingmlx_amd._lib import GsplatError
    p, cams = gcp._scene()
    r = _renderer(W, H)
    f, out = torch.zeros(3000, 4, device="cuda"), torch.zeros(H, W, 4, device="cuda")
    grad = torch.zeros(3000, 4, device="cuda")
    assert r.lib.gs_render_features(r.ctx, 4, f.data_ptr(), out.data_ptr()) == 5              # GS_ERR_NO_FORWARD
    assert r.lib.gs_render_features_backward(r.ctx, 4, out.data_ptr(), grad.data_ptr()) == 5
    with pytest.raises(GsplatError) as e:
        r.renderFeatures(f)
    assert e.value.code == 5
    with pytest.raises(GsplatError):
        r.renderFeaturesVJP(out)
    r.renderChecked(_dev(p), cams[0])
    for C in (0, 257):
        assert r.lib.gs_render_features(r.ctx, C, f.data_ptr(), out.data_ptr()) == 1          # GS_ERR_INVALID_ARG
        assert r.lib.gs_render_features_backward(r.ctx, C, out.data_ptr(), grad.data_ptr()) == 1
    assert r.lib.gs_render_features(r.ctx, 4, None, out.data_ptr()) == 1
    assert r.lib.gs_render_features(r.ctx, 4, f.data_ptr(), None) == 1
    assert r.lib.gs_render_features_backward(r.ctx, 4, None, grad.data_ptr()) == 1
    assert r.lib.gs_render_features_backward(r.ctx, 4, out.data_ptr(), None) == 1
    for bad in (torch.zeros(2999, 4, device="cuda"), torch.zeros(3000, 4), torch.zeros(3000, 4, device="cuda", dtype=torch.float64),
                torch.zeros(3000, 8, device="cuda")[:, ::2], torch.zeros(3000, 257, device="cuda")):
        with pytest.raises(ValueError):
            r.renderFeatures(bad)
    with pytest.raises(ValueError):
        r.renderFeatures(f, torch.zeros(H, W, 5, device="cuda"))
    with pytest.raises(ValueError):
        r.renderFeaturesVJP(out, torch.zeros(3000, 5, device="cuda"))
    with pytest.raises(ValueError):
        r.renderFeaturesVJP(torch.zeros(H, W - 1, 4, device="cuda"))
    # the op-level pair: a binning first, the binned N, C in range, no null buffer
    c, s, bn, lists, _ = _op_case("partial_blocks", oracle64)
    r2 = _renderer(c["W"], c["H"], c["tile"])
    packed = r2._t(s["packed"])
    f2, out2 = torch.zeros(c["N"], 4, device="cuda"), torch.zeros(c["H"], c["W"], 4, device="cuda")
    assert r2.lib.gs_blend_features(r2.ctx, c["N"], 4, packed.data_ptr(), f2.data_ptr(), out2.data_ptr()) == 5
    _bin(r2, s, bn)
    assert r2.lib.gs_blend_features(r2.ctx, c["N"] - 1, 4, packed.data_ptr(), f2.data_ptr(), out2.data_ptr()) == 2
    for C in (0, 257):
        assert r2.lib.gs_blend_features(r2.ctx, c["N"], C, packed.data_ptr(), f2.data_ptr(), out2.data_ptr()) == 1
        assert r2.lib.gs_blend_features_backward(r2.ctx, c["N"], C, packed.data_ptr(), out2.data_ptr(), f2.data_ptr()) == 1
    assert r2.lib.gs_blend_features(r2.ctx, c["N"], 4, packed.data_ptr(), None, out2.data_ptr()) == 1
    assert r2.lib.gs_blend_features_backward(r2.ctx, c["N"], 4, packed.data_ptr(), out2.data_ptr(), None) == 1
    with pytest.raises(ValueError):
        r2.blendFeatures(s["packed"], torch.zeros(c["N"] + 1, 4, device="cuda"))
    # a field of another N
    field = ft.FeatureField(r, 2999, 4)
    with pytest.raises(ValueError):
        field.trainStep(_dev(p), cams[0], torch.zeros(H, W, 4, device="cuda"))
    with pytest.raises(ValueError):
        field.render(_dev(p), cams[0])
    with pytest.raises(ValueError):
        ft.FeatureField(r, 3000, 257)


# ---------------------------------------------------------------------------------------------------------- 8. training
def test_training_follows_the_float64_host_loop(oracle64):
    """The case of the CPU test (C = 8, "l2", five steps from zeros, lr 1e-3) on the 3000-Gaussian scene, which a fused forward
    needs: the host loops run on that forward's oracle records and lists, the weights computed once per format."""
    t = fcpu.TRAIN
    p, cams = gcp._scene()
    fw = _want_fused(oracle64, "plain")[0]
    lists = (fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, 16, 16)
    fstar = np.random.default_rng(t["fseed"]).uniform(-1, 1, (3000, t["C"]))
    target = ft.blend_features(*lists, fstar)
    l64 = fcpu.host_loop(lists, target, 3000, t["C"], np.float64)
    l32 = fcpu.host_loop(lists, target, 3000, t["C"], np.float32)
    d32 = fcpu.relative_distance(l32, l64)
    r = _renderer(W, H)
    field = ft.FeatureField(r, 3000, t["C"], lr=t["lr"])
    params, tgt = _dev(p), _cuda(target)
    got = np.array([float(field.trainStep(params, cams[0], tgt, loss=t["loss"])) for _ in range(t["steps"])])
    dist = fcpu.relative_distance(got, l64)
    bars = np.maximum(4 * d32, 1e-6)
    print(f"float64 losses {l64}\ndevice losses {got}\nd32 {d32}\ndevice distance {dist}\nbars {bars}")
    assert (np.diff(l64) < 0).all()
    assert got[-1] < got[0]
    assert (dist <= bars).all()
    # a masked "l1" step is the host statement's too
    mask = (np.random.default_rng(4).integers(0, 256, (H, W))).astype(np.uint8)
    img = _np(field.render(params, cams[0])).astype(np.float64)
    want = ft.loss_and_cotangent(img, target, mask, "l1")[0]
    value = float(field.trainStep(params, cams[0], tgt, mask=torch.as_tensor(mask, device="cuda"), loss="l1"))
    assert abs(value - want) <= 1e-5 * abs(want)
