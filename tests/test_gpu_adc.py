"""Adaptive density control on the device (include/gsplat.h gs_set_adc_stats, csrc/adc.hip) against the
numpy restatement of tests/adc_numpy.py, which tests/test_adc_cpu.py qualifies without a device.

Sizes.  Images of 64 x 48 (4 x 3 tiles of 16 x 16) and N = 2500 Gaussians: two boundaries of the 1024-item scan tile and a
partial 256-thread block.  The scene is scenes.make_gaussians(2500, "trained_like", seed, sh_degree=3) with its scales raised to
~0.06 (at 64 x 48 the generator's 0.012 is a fifth of a pixel) and every fifth position moved out past the cameras' ring (so
that every view has Gaussians it does not see), under three of scenes.lego_cameras.

Bars.
  float results (the statistic, the gather's xyz / scales / revised opacity): no element further from the float64 restatement
      than 4 x the float32-to-float64 distance of the restatements, floor one float32 ulp.  The unit is an ulp of the element's
      magnitude -- the value for the statistic, what was added up for the gather (adc_numpy.gather_magnitudes: a child's
      |position| + |offset| terms, max(|o'|, |o|, 1) for a revised opacity), since a rounding error is an ulp of an operand, not
      of a sum that came out small.  The distance is ONE number per tensor, the largest over the elements (adc_numpy.yardstick):
      the device's exp, log and hypot round differently from numpy's, so which element is a last place off differs between them.
      Measured on MI355X (device / float32 numpy / bar, ulps): gradSum 1.27 / 1.27 / 5.1 and, after the adding call, 1.70 / 1.51 /
      6.1; gather scales 0.44 / 0.44 / 1.75; gather xyz 2.6 - 3.6 / 2.9 - 4.1 / 11.5 - 16.5; revised opacity 2.1 - 2.5 / 1.7 - 2.1 /
      6.8 - 8.3; the table is in DESIGN.md section 26.
  the statistic in a step against hypot(W/2 S_x, H/2 S_y) of the float64 oracle's blend backward: 1e-3 of the largest value.
  decisions, copies, moments, counts, radii: exact.
  a step with the statistic set against the same step without it: the render bit for bit (no atomics on that path); gradients,
      parameters and moments bit for bit where two runs WITHOUT the statistic are bit-identical themselves -- the blend backward
      adds a Gaussian's per-block sums with float atomics whose order varies from launch to launch (tests/test_gpu_contrib_prune.py
      test_off_is_off, tests/test_gpu_parity.py) --, and where they are not, within the project's bars for two runs of those
      atomics (_spread_ok; measured here: two runs of one step part by 1e-7 to 4e-6 of a tensor's largest, with or without the
      statistic).  The kernel reads the rows and the radii and writes three buffers of the caller's.
  classify: all four actions must occur at both settings of sizePrune with allowDensify on; with it off no rule produces a
      split or a clone, so there the test requires keep and prune, and that no growth occurs.
  the trainer's first event against the float32 restatement: exact on every row not within 1e-6 (relative, float64) of a
      threshold, where the device's exp may round to the other side; at most two such rows (measured: none).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import adc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
W, H, N, DEGREE = 64, 48, 2500, 3
GRAD_BAR = 1e-3


def _load(name):
    spec = importlib.util.spec_from_file_location("_adcg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


az = _load("adc_numpy")
_cache = {}


def _renderer():
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(DEGREE, W, H, (16, 16), False)


def _scene():
    if "scene" not in _cache:
        from gaussiansplattingmlx_amd.scenes import lego_cameras, make_gaussians
        p = make_gaussians(N, "trained_like", 20260626, sh_degree=DEGREE)
        p["scales"] = (p["scales"] + np.float32(np.log(5.0))).astype(np.float32)
        p["xyz"][::5] *= np.float32(4.0)          # every fifth out to +-5.2, past the cameras' ring: no view sees all of them
        _cache["scene"] = (p, lego_cameras(3, W, H, 20260627))
    return _cache["scene"]


def _cot():
    return torch.as_tensor((np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)).astype(np.float32), device="cuda")


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_distance(what, got, want32, want64, magnitude=None):
    worst, yard, bar, bad = az.distance_check(got, want32, want64, magnitude)
    print(f"{what}: device against float64 {worst:.3f} ulp, float32 restatement against float64 {yard:.3f} ulp (bar {bar:.3f} ulp)")
    assert len(bad) == 0, (what, worst, bar, bad[:5])


# ------------------------------------------------------------------------------------------------ 1. accumulate, op level
def test_accumulate_matches_the_restatement():
    r = _renderer()
    rows, radii, acc0 = az.accumulate_inputs()
    acc0[0, 5] = 0.0                                   # the 1e-25 row starts from nothing: what it adds must show
    acc = _t(acc0)
    want32, want64 = tuple(acc0), tuple(acc0)
    for call, use_abs in enumerate((False, True)):     # the second call adds, and reads columns 12, 13
        r.adcAccumulate(rows, radii, use_abs, acc[0], acc[1], acc[2])
        want32 = az.accumulate(rows, radii, use_abs, W, H, *want32, dtype=np.float32)
        want64 = az.accumulate(rows, radii, use_abs, W, H, *want64, dtype=np.float64)
        got = _np(acc)
        _check_distance(f"gradSum after call {call + 1} (use_abs={use_abs})", got[0], want32[0], want64[0])
        assert np.array_equal(got[1], want64[1]) and np.array_equal(got[2], want64[2])
        zero = radii == 0
        assert zero.sum() > 500 and zero[7] and not zero[6] and not zero[8]
        assert np.array_equal(_bits(got[:, zero]), _bits(acc0[:, zero]))           # radius 0: all three words keep their bits
        assert got[0, 5] > 0 and np.isfinite(got[0, 6])
    assert got[0, 5] == pytest.approx(2 * np.hypot(32e-25, 24e-25), rel=1e-5)      # 1e-25 in both columns, both calls
    # the mode matters: the signed and the absolute columns hold different numbers
    one = _t(acc0)
    r.adcAccumulate(rows, radii, False, one[0], one[1], one[2])
    two = _t(acc0)
    r.adcAccumulate(rows, radii, True, two[0], two[1], two[2])
    assert not torch.equal(one[0], two[0]) and torch.equal(one[1:], two[1:])
    # arguments
    a = acc
    assert r.lib.gs_adc_accumulate(r.ctx, -1, _t(rows).data_ptr(), _t(radii).data_ptr(), 0, *[x.data_ptr() for x in a]) == 1
    assert r.lib.gs_adc_accumulate(r.ctx, N, None, _t(radii).data_ptr(), 0, *[x.data_ptr() for x in a]) == 1
    assert r.lib.gs_adc_accumulate(r.ctx, N, _t(rows).data_ptr(), _t(radii).data_ptr(), 2, *[x.data_ptr() for x in a]) == 1
    assert r.lib.gs_adc_accumulate(r.ctx, 0, None, None, 0, None, None, None) == 0
    r.close()


# ---------------------------------------------------------------------------------------------- 2. accumulate, in a step
def _spread_ok(what, a, b, c, loop=False):
    """c (the run with the statistic) against a, where a and b are two runs without it: bit for bit where a and b are, else the
    project's bars for two runs of the blend backward's float atomics -- one step: 1e-4 of the tensor's largest
    (tests/test_gpu_dp_kernels.py); a loop of steps: the share of elements beyond 1e-3 of the largest below 1e-3
    (tests/test_gpu_trajectory.py, tests/test_gpu_contrib_prune.py test_off_is_off), which a and b are held to as well."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    if np.array_equal(_bits(a), _bits(b)):
        print(f"{what}: two runs without the statistic are bit-identical; with it: {np.array_equal(_bits(a), _bits(c))}")
        assert np.array_equal(_bits(a), _bits(c)), what
        return
    big = np.abs(a).max()
    print(f"{what}: two runs without the statistic differ by {np.abs(a - b).max() / big:.3e} of the largest (float atomics); "
          f"with it {np.abs(a - c).max() / big:.3e}")
    if loop:
        assert np.mean(np.abs(a - b) > 1e-3 * big) < 1e-3 and np.mean(np.abs(a - c) > 1e-3 * big) < 1e-3, what
    else:
        assert np.abs(a - b).max() <= 1e-4 * big and np.abs(a - c).max() <= 1e-4 * big, what


def test_a_step_accumulates_and_moves_nothing_else(oracle64):
    p, cams = _scene()
    r = _renderer()
    params, cot = _dev(p), _cot()

    def step(stats):
        r.setADCStats(*(stats if stats is not None else (None, None, None)))
        res = r.renderChecked(params, cams[0], wantDepth=False)
        img = res.render.clone()
        g = {k: v.clone() for k, v in r.renderBackward(cot).items()}
        r.setADCStats(None)
        return img, g

    radii = _np(r.renderChecked(params, cams[0], want_radii=True, wantDepth=False).radii)
    img_a, g_a = step(None)
    img_b, g_b = step(None)
    acc = torch.zeros(3, N, device="cuda")
    img_c, g_c = step((acc[0], acc[1], acc[2]))            # (no radii buffer of the caller's: the context keeps them)
    assert torch.equal(img_a, img_b) and torch.equal(img_a, img_c)
    for k in KEYS:
        _spread_ok(f"gradient {k}", _np(g_a[k]), _np(g_b[k]), _np(g_c[k]))
    got = _np(acc)
    vis = radii > 0
    assert 1000 < vis.sum() < N                              # some of each
    assert np.array_equal(got[1], vis.astype(np.float32))
    assert np.array_equal(got[2], np.where(vis, radii, 0.0).astype(np.float32))
    assert not got[0][~vis].any()
    # the float64 oracle's signed 2-D mean gradient
    fw = oracle64.render_forward(p, cams[0].as_dict(), W, H, 16, 16, DEGREE)
    bn = fw["bin"]
    z = np.zeros(W * H)
    gp = oracle64.blend_backward(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, 16, 16, False,
                                 _np(cot).astype(np.float64).reshape(-1, 3), z, z, fw["color"], fw["depth"], fw["alpha"], fw["last"])
    want = np.hypot(0.5 * W * gp[:, 0], 0.5 * H * gp[:, 1])
    assert np.array_equal(np.asarray(fw["proj"]["radii"]).reshape(-1) > 0, vis)
    err = np.abs(got[0] - want).max() / want.max()
    print(f"gradSum of one step against hypot(W/2 S_x, H/2 S_y) of the float64 oracle: {err:.3e} of the largest (bar {GRAD_BAR:.0e}); "
          f"{int((want > 0).sum())} non-zero, largest {want.max():.3e}")
    assert err <= GRAD_BAR and (want > 0).sum() > 1000
    # a second step adds; a caller's radii buffer serves as well as the context's
    # (the result is dropped on purpose: the renderer keeps the buffer the backward will read until its next forward)
    r.setADCStats(acc[0], acc[1], acc[2])
    ptr = r.renderChecked(params, cams[0], want_radii=True, wantDepth=False).radii.data_ptr()
    assert r._fused["radii"] is not None and r._fused["radii"].data_ptr() == ptr
    filler = [torch.full((N,), -7.0, device="cuda") for _ in range(8)]      # would take a freed block of that size
    assert all(f.data_ptr() != ptr for f in filler)
    r.renderBackward(cot)
    got2 = _np(acc)
    assert np.array_equal(got2[1], 2 * vis.astype(np.float32)) and np.array_equal(got2[2], got[2])
    assert np.abs(got2[0] - 2 * want).max() / want.max() <= 2 * GRAD_BAR
    r.setADCStats(None)
    r.close()


def test_the_fused_adam_step_is_the_one_without_the_statistic():
    from gaussiansplattingmlx_amd.trainer import GaussModel
    p, cams = _scene()
    r = _renderer()
    target = torch.rand(H, W, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = []
    for stats in (False, False, True):
        model = GaussModel(p, r.device)
        model.m.fill_(1e-4)
        model.v.fill_(1e-8)
        acc = torch.zeros(3, N, device="cuda")
        if stats:
            r.setADCStats(acc[0], acc[1], acc[2])
        res = r.renderChecked(model.getParams(), cams[1], wantDepth=False)
        img = res.render.clone()
        _, gc, _ = r.lossForwardBackward(res.render, target, 0.2)
        r.renderBackwardAdam(gc, model.arena, model.m, model.v, [1e-3] * 6)
        r.setADCStats(None)
        out.append((img, model.arena.clone(), model.m.clone(), model.v.clone(), acc))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][0], out[2][0])
    for i, name in ((1, "parameters"), (2, "first moments"), (3, "second moments")):
        _spread_ok(name, _np(out[0][i]), _np(out[1][i]), _np(out[2][i]))
    assert bool(out[2][4][1].sum() > 1000) and bool(out[2][4][0].sum() > 0) and not bool(out[0][4].any())
    r.close()


def test_an_overflowed_step_adds_nothing():
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel
    p, cams = _scene()
    r0 = _renderer()
    r0.renderForward(_dev(p), cams[0])
    r0.sync()
    M = r0.stats()["M"]
    r0.close()
    r = _renderer()
    r.reserve(N, M // 3)                                     # too small on purpose: a reported overflow
    acc = torch.full((3, N), 0.5, device="cuda")
    r.setADCStats(acc[0], acc[1], acc[2])
    model = GaussModel(p, r.device)
    before = model.arena.clone()
    res = r.renderForward(model.getParams(), cams[0], wantDepth=False)
    try:                                                     # may or may not have seen the flag yet: both are in contract
        _, gc, _ = r.lossForwardBackward(res.render, torch.rand(H, W, 3, device="cuda"), 0.2)
        r.renderBackwardAdam(gc, model.arena, model.m, model.v, [1e-2] * 6)
    except GsplatError as e:
        assert e.code == 3
    with pytest.raises(GsplatError) as ei:
        r.sync()
    assert ei.value.code == 3 and r.stats()["overflow"] == 1
    assert torch.equal(acc, torch.full((3, N), 0.5, device="cuda"))
    assert torch.equal(model.arena, before)
    r.setADCStats(None)
    r.close()


def test_refusals(monkeypatch):
    p, cams = _scene()
    monkeypatch.setenv("GSPLAT_BLOCK_LISTS", "0")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    rg = GaussianRenderer(DEGREE, W, H, (50, 38), False)    # a context whose fused path is the generic kernels
    assert not rg.blockLists
    a = torch.zeros(3, N, device="cuda")
    assert rg.lib.gs_set_adc_stats(rg.ctx, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr()) == 1
    assert rg.lib.gs_set_adc_stats(rg.ctx, None, None, None) == 0
    rg.close()
    monkeypatch.delenv("GSPLAT_BLOCK_LISTS")
    r = _renderer()
    assert r.lib.gs_set_adc_stats(r.ctx, a[0].data_ptr(), None, a[2].data_ptr()) == 1          # all three or none
    assert r.lib.gs_set_adc_stats(r.ctx, None, None, a[2].data_ptr()) == 1
    params, cot = _dev(p), _cot()
    # a forward made before the statistic was set kept no radii for a backward, a caller's buffer or not
    r.renderChecked(params, cams[0], want_radii=True, wantDepth=False)
    r.setADCStats(a[0], a[1], a[2])
    g = [torch.zeros(N, k, device="cuda") for k in (3, 3, 4, 1)]
    g6 = [torch.zeros(N, 3, device="cuda"), torch.zeros(N, 1, 3, device="cuda"), torch.zeros(N, 15, 3, device="cuda"),
          torch.zeros(N, 3, device="cuda"), torch.zeros(N, 4, device="cuda"), torch.zeros(N, device="cuda")]
    assert r.lib.gs_render_backward(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g6]) == 5      # GS_ERR_NO_FORWARD
    r.renderChecked(params, cams[0], wantDepth=False)
    cc = torch.zeros(3 * N + 16, device="cuda")
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 1
    assert not any(bool(t.any()) for t in g) and not bool(a.any())
    r.renderBackward(cot)                                   # the forward is still usable
    assert bool(a[1].sum() > 1000)
    r.setADCStats(None)
    r.renderChecked(params, cams[0], wantDepth=False)
    assert r.lib.gs_render_backward_dp(r.ctx, cot.data_ptr(), None, None, *[t.data_ptr() for t in g], cc.data_ptr()) == 0
    r.close()


# ------------------------------------------------------------------------------------------------------------ 3. classify
@pytest.mark.parametrize("screen", [20.0, 0.0])
def test_classify_equals_the_float32_restatement(screen):
    r = _renderer()
    prm = dict(az.DEFAULTS, max_screen_size=screen)
    inp = az.classify_inputs(prm)
    assert not az.near_threshold(*inp, prm).any()             # none within 1e-3 relative of a threshold in float64
    scales4 = np.concatenate([inp[3], np.full((N, 1), 80.0, np.float32)], axis=1)      # junk in a fourth column: the stride is honoured
    for allow in (True, False):
        for size in (True, False):
            want_a, want_c = az.classify(*inp, prm, allow, size, np.float32)
            for sc in (inp[3], scales4):
                a, c = r.adcClassify(inp[0], inp[1], inp[2], sc, inp[4], gradThreshold=prm["grad_threshold"],
                                     percentDense=prm["percent_dense"], minOpacity=prm["min_opacity"], maxScreenSize=screen,
                                     pruneWorld=prm["prune_world"], sceneExtent=prm["scene_extent"], allowDensify=allow,
                                     sizePrune=size)
                assert a.dtype == torch.int32 and np.array_equal(_np(a), want_a) and np.array_equal(_np(c), want_c)
            hist = np.bincount(want_a, minlength=4)
            print(f"screen {screen} allowDensify {allow} sizePrune {size}: keep / split / clone / prune = {hist}")
            if allow:
                assert (hist > 0).all()
            else:
                assert hist[0] > 0 and hist[3] > 0 and hist[1] == hist[2] == 0
    # arguments
    bad = az.DEFAULTS["scene_extent"]
    from gaussiansplattingmlx_amd._lib import GsplatError
    for kw in (dict(sceneExtent=0.0), dict(gradThreshold=-1.0), dict(maxScreenSize=float("nan"))):
        with pytest.raises(GsplatError) as e:
            r.adcClassify(inp[0], inp[1], inp[2], inp[3], inp[4], **dict(dict(sceneExtent=bad), **kw))
        assert e.value.code == 1
    r.close()


# -------------------------------------------------------------------------------------------------- 4. gather and moments
def _event_maps(r, actions):
    counts = np.array([1, 2, 2, 0], np.int32)[actions]
    a, c = _t(actions, torch.int32), _t(counts, torch.int32)
    off, st = r.densifyOffsets(a, c)
    g, m = r.buildDensifyOutputMap(a, off, st["total"])
    return a, g, m, st


@pytest.mark.parametrize("K", [16, 4, 25])
@pytest.mark.parametrize("revised", [False, True])
def test_gather_matches_the_restatement(K, revised):
    """K = 16 and 4: f_rest rows of 45 and 9 floats (the one-float row gather); K = 25: 72 floats (the float4 one)."""
    r = _renderer()
    p = az.gather_params(N, K)
    act = az.gather_actions(N)
    a, g, m, st = _event_maps(r, act)
    total = st["total"]
    noise = r.densifyNoise(20260313 + K, total)
    out = {k: _np(v) for k, v in r.adcGather(_dev(p), g, m, noise, revisedOpacity=revised).items()}
    gi, mo, nz = _np(g), _np(m), _np(noise)
    want32 = az.gather(p, gi, mo, nz, revised, np.float32)
    want64 = az.gather(p, gi, mo, nz, revised, np.float64)
    assert total == int((act == 0).sum() + 2 * (act == 1).sum() + 2 * (act == 2).sum()) and total > N
    for k in KEYS:
        assert out[k].shape == want64[k].shape and out[k].dtype == np.float32, k
    mags = az.gather_magnitudes(p, gi, mo, nz, revised)
    for k in ("xyz", "scales", "opacity"):
        _check_distance(f"K={K} revised={revised} {k}", out[k], want32[k], want64[k], mags[k].reshape(want64[k].shape))
    for k in ("features_dc", "features_rest", "rotation"):
        assert np.array_equal(_bits(out[k]), _bits(p[k][gi])), k
    split = (mo == 1) | (mo == 2)
    copies = ~split
    assert (mo == 1).sum() == (mo == 2).sum() == (act == 1).sum() and (mo == 3).sum() == (act == 2).sum()
    for k in KEYS if not revised else ("xyz", "features_dc", "features_rest", "scales", "rotation"):
        assert np.array_equal(_bits(out[k][copies]), _bits(p[k][gi][copies])), k        # kept and cloned rows: exact copies
    if revised:
        rev = np.isin(act[gi], (1, 2))
        assert np.array_equal(_bits(out["opacity"][~rev]), _bits(p["opacity"][gi][~rev]))
        assert (out["opacity"][rev] < p["opacity"][gi][rev]).all()
    # both children of a split moved, each by its own noise; the unnormalised quaternions' rows among them
    first, second = np.flatnonzero(mo == 1), np.flatnonzero(mo == 2)
    assert np.array_equal(second, first + 1) and np.array_equal(gi[first], gi[second])
    assert (np.abs(out["xyz"][first] - p["xyz"][gi[first]]).max(axis=1) > 0).all()
    assert (np.abs(out["xyz"][second] - p["xyz"][gi[second]]).max(axis=1) > 0).all()
    assert (np.abs(out["xyz"][first] - out["xyz"][second]).max(axis=1) > 0).all()
    assert {3, 4} <= set(gi[first])
    r.close()


@pytest.mark.parametrize("K", [16, 4, 25])
def test_moments_survive_where_the_gaussian_does(K):
    r = _renderer()
    rng = np.random.default_rng([43, K])
    act = az.gather_actions(N)
    a, g, m, st = _event_maps(r, act)
    gi, mo = _np(g), _np(m)
    kept = (mo == 0) & (act[gi] != 1)
    for what in ("m", "v"):
        src = {k: rng.normal(0, 1e-3, v.shape).astype(np.float32) for k, v in az.gather_params(N, K).items()}
        if what == "v":
            src = {k: np.abs(v) for k, v in src.items()}
        out = {k: _np(v) for k, v in r.adcGatherMoments(_dev(src), g, m, a).items()}
        want = az.gather_moments(src, gi, mo, act)
        for k in KEYS:                                       # all six segments
            assert out[k].shape[0] == st["total"]
            assert np.array_equal(_bits(out[k]), _bits(want[k])), (what, k)
            assert np.array_equal(_bits(out[k][kept]), _bits(src[k][gi][kept])), (what, k)      # kept rows, clone originals
            assert not _bits(out[k][~kept]).any(), (what, k)                                     # children and copies: +0.0
    assert kept[(mo == 0) & (act[gi] == 2)].all() and not kept[mo == 3].any() and not kept[(mo == 1) | (mo == 2)].any()
    r.close()


# --------------------------------------------------------------------------------------------------------------- 5. reset
def test_reset_caps_the_opacities_and_zeroes_their_moments():
    from gaussiansplattingmlx_amd.trainer import GaussModel
    r = _renderer()
    p = {k: v.copy() for k, v in az.gather_params(N, 16).items()}
    cap = az.reset_raw(0.01)
    p["opacity"][:6] = [cap, np.nextafter(cap, np.float32(np.inf)), np.nextafter(cap, np.float32(-np.inf)), 9.0, -9.0, 0.0]
    model = GaussModel(p, r.device)
    model.m.fill_(1.0)
    model.v.fill_(2.0)
    arena0, m0, v0 = model.arena.clone(), model.m.clone(), model.v.clone()
    mo, vo = model.getMoments()
    r.adcResetOpacity(model.getParams()["opacity"], mo["opacity"], vo["opacity"], 0.01)
    want, _, _ = az.reset_opacity(p["opacity"], 0, 0, 0.01)
    got = _np(model.getParams()["opacity"]).reshape(-1)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got <= p["opacity"]).all() and (got[[0, 1, 3, 5]] == cap).all() and got[2] < cap and got[4] == -9.0
    assert (p["opacity"] > cap).sum() > 500 and (p["opacity"] < cap).sum() > 100
    assert not bool(mo["opacity"].any()) and not bool(vo["opacity"].any())
    s, e = int(model.seg_start[3]), int(model.seg_start[3]) + N            # the opacity segment of the arenas (ARENA_ORDER)
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    assert ARENA_ORDER[3] == "opacity"
    for now, was in ((model.arena, arena0), (model.m, m0), (model.v, v0)):
        assert torch.equal(now[:s], was[:s]) and torch.equal(now[e:], was[e:])      # every other segment, pads included
    r.adcResetOpacity(model.getParams()["opacity"], mo["opacity"], vo["opacity"], 0.01)
    assert np.array_equal(_bits(_np(model.getParams()["opacity"]).reshape(-1)), _bits(want))      # idempotent
    assert r.lib.gs_adc_reset_opacity(r.ctx, N, model.getParams()["opacity"].data_ptr(), None, vo["opacity"].data_ptr(), 0.01) == 1
    assert r.lib.gs_adc_reset_opacity(r.ctx, N, model.getParams()["opacity"].data_ptr(), mo["opacity"].data_ptr(),
                                      vo["opacity"].data_ptr(), 1.0) == 1
    r.close()


# ------------------------------------------------------------------------------------------------------------- 6. trainer
def _targets(r, p, cams):
    tp = _dev(p)
    return [r.renderChecked(tp, c).render.clone() for c in cams]


def _adc_config(cams, **kw):
    return adc.ADCConfig(scene_extent=adc.scene_extent(cams), densify_from=20, densify_interval=20, opacity_reset_interval=60,
                         densify_until=160, **kw)


def test_trainer_runs_the_strategy(monkeypatch):
    """strategy="adc" with absgrad (the combination the trainer allows here and only here: the absolute sums can be read back
    after every step, so the accumulators can be held to the device's own per-step statistic), 180 steps."""
    from gaussiansplattingmlx_amd.absgrad import AbsGradConfig
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = _scene()
    r = _renderer()
    targets = _targets(r, p, cams)
    model = GaussModel(perturb(p, 5, 0.3), r.device)
    cfg = _adc_config(cams)
    tr = GaussianTrainer(model, r, iterationCount=1000, strategy="adc", adc=cfg, absgrad=AbsGradConfig(), densify=False)
    tr.maxGaussians = 6000          # (the first event cannot pass it from 2500; later ones may, and then only prune)
    assert tr.gradientThreshold == 0.0008 and not tr.densify and tr.adc is cfg
    seen, gathered = [], []
    real, real_moments = r.adcClassify, r.adcGatherMoments

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append(([_np(x).copy() for x in a[:5]], dict(kw), _np(out[0]).copy(), _np(out[1]).copy()))
        return out

    def spy_moments(moments, gather, mode, actions, out=None):
        if len(gathered) < 2:       # the first event's two arenas: what went in, and the event's map
            gathered.append(({k: _np(v).copy() for k, v in moments.items()}, _np(gather).copy(), _np(mode).copy(), _np(actions).copy()))
        return real_moments(moments, gather, mode, actions, out=out)

    monkeypatch.setattr(r, "adcClassify", spy)
    monkeypatch.setattr(r, "adcGatherMoments", spy_moments)
    running, visits, biggest = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    losses = []
    for it in range(19):
        radii = _np(r.renderChecked(model.getParams(), cams[it % 3], want_radii=True, wantDepth=False).radii)
        losses.append(float(tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)[0]))
        A = _np(r.absgrad())
        hw, hh = np.float32(0.5 * W), np.float32(0.5 * H)
        running = running + np.where(radii > 0, np.hypot(hw * A[:, 0], hh * A[:, 1], dtype=np.float32), np.float32(0))
        visits += radii > 0
        biggest = np.maximum(biggest, radii)
        assert getattr(r, "_adc_stats", None) is None        # the statistic is set around the trainer's own steps only
    got = _np(tr._adcAcc)
    nz = running > 1e-30
    err = np.abs(got[0].astype(np.float64) - running)[nz] / running[nz]
    print(f"gradSum against the running float32 sum of 19 steps: {err.max():.3e} per element (bar 1e-5); {int(nz.sum())} non-zero")
    assert nz.sum() > 1500 and err.max() <= 1e-5 and np.abs(got[0] - running)[~nz].max() <= 1e-35
    assert np.array_equal(got[1], visits) and np.array_equal(got[2], biggest) and 7 <= visits.max() <= 19
    losses.append(float(tr.trainStep(cams[19 % 3], targets[19 % 3], viewKey=19 % 3)[0]))
    assert model.N == N and not seen
    # step 20 and the first event behind it
    losses.append(float(tr.trainStep(cams[20 % 3], targets[20 % 3], viewKey=20 % 3)[0]))
    assert len(seen) == 1 and len(gathered) == 2
    (gs, cn, mr, sc, op), kw, dev_a, dev_c = seen[0]
    prm = dict(grad_threshold=kw["gradThreshold"], percent_dense=kw["percentDense"], min_opacity=kw["minOpacity"],
               max_screen_size=kw["maxScreenSize"], prune_world=kw["pruneWorld"], scene_extent=kw["sceneExtent"])
    assert kw["gradThreshold"] == 0.0008 and kw["sizePrune"] is False and kw["allowDensify"] is True and 7 <= cn.max() <= 21
    want_a, want_c = az.classify(gs, cn, mr, sc, op, prm, True, False, np.float32)
    near = az.near_threshold(gs, cn, mr, sc, op, prm, rel=1e-6)      # (where the device's exp may round the other way)
    print(f"the first event: actions {np.bincount(dev_a, minlength=4)}, {int(near.sum())} rows within 1e-6 of a threshold")
    assert near.sum() <= 2 and np.array_equal(dev_a[~near], want_a[~near]) and np.array_equal(dev_c[~near], want_c[~near])
    st = tr.lastDensifyStats
    assert st["split"] + st["clone"] > 0 and st["keep"] > 0
    assert tr.lastADCStats["reset"] is False and tr.lastADCStats["size_prune"] is False
    final = seen[-1]
    assert model.N == st["total"] == int(final[3].sum()) and model.N <= tr.maxGaussians
    assert not bool(tr._adcAcc.any()) and tr._adcAcc.shape == (3, model.N)      # the accumulators start anew
    # a kept Gaussian's and a clone original's moments are those they had behind the step's own Adam update (what the event
    # was handed); split children and clone copies start at zero
    for (src, gi, mo_, act_), now in zip(gathered, model.getMoments()):
        assert np.array_equal(act_, dev_a) and len(gi) == model.N
        want = az.gather_moments(src, gi, mo_, act_)
        kept = (mo_ == 0) & (act_[gi] != 1)
        for k in KEYS:
            assert np.array_equal(_bits(_np(now[k])), _bits(want[k])), k
            assert np.array_equal(_bits(_np(now[k])[kept]), _bits(src[k][gi][kept])) and not _np(now[k])[~kept].any(), k
        assert src["xyz"][gi][kept].any() and kept.sum() == st["keep"] + st["clone"]
    n_max = model.N
    for it in range(21, 61):
        losses.append(float(tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)[0]))
        n_max = max(n_max, model.N)
        if it == 59:
            assert not tr.adcSizePrune
    # behind step 60: the event, then the reset
    op60 = torch.sigmoid(model.getParams()["opacity"])
    assert float(op60.max()) <= 0.01 + 1e-6 and tr.adcSizePrune and tr.lastADCStats["reset"] is True
    mo, vo = model.getMoments()
    assert not bool(mo["opacity"].any()) and not bool(vo["opacity"].any()) and bool(mo["xyz"].any())
    for it in range(61, 180):
        losses.append(float(tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)[0]))
        n_max = max(n_max, model.N)
    assert seen[-1][1]["sizePrune"] is True
    assert not bool(tr._adcAcc.any())         # behind densify_until = 160 nothing reads the statistic: steps 161 .. 179 add none
    print(f"N: {N} -> {model.N} (largest {n_max}, maxGaussians {tr.maxGaussians}); loss {losses[0]:.4f} -> {losses[-1]:.4f}; "
          f"last event {tr.lastADCStats}")
    assert n_max <= tr.maxGaussians
    assert bool(torch.isfinite(model.arena).all()) and bool(torch.isfinite(model.m).all()) and bool(torch.isfinite(model.v).all())
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert tr.iteration == 180 and len([s for s in seen]) >= 8
    r.close()


@pytest.mark.parametrize("fuse", [True, False])
def test_trainer_without_absgrad_counts_visits(fuse):
    """The signed statistic (no absgrad), fused and unfused Adam, with revised opacity, through two events."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = _scene()
    r = _renderer()
    targets = _targets(r, p, cams)
    model = GaussModel(perturb(p, 5, 0.3), r.device)
    tr = GaussianTrainer(model, r, iterationCount=1000, strategy="adc", adc=_adc_config(cams, revised_opacity=True), fuse_adam=fuse)
    assert tr.gradientThreshold == 0.0002 and not getattr(r, "_absgrad", False)
    visits, biggest = np.zeros(N, np.float32), np.zeros(N, np.float32)
    for it in range(20):
        radii = _np(r.renderChecked(model.getParams(), cams[it % 3], want_radii=True, wantDepth=False).radii)
        tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
        visits += radii > 0
        biggest = np.maximum(biggest, radii)
    got = _np(tr._adcAcc)
    assert np.array_equal(got[1], visits) and np.array_equal(got[2], biggest)
    assert (got[0][visits > 0] > 0).mean() > 0.9 and not got[0][visits == 0].any()
    for it in range(20, 45):
        tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
    print(f"fuse={fuse}: N {N} -> {model.N}; last event {tr.lastADCStats}")
    assert tr.lastADCStats is not None and tr.lastADCStats["N"] > 0 and tr._adcAcc.shape == (3, model.N)
    assert 2.0 <= float(tr._adcAcc[1].max()) <= 4.0                        # steps 41 .. 44 since the event behind step 40
    assert bool(torch.isfinite(model.arena).all()) and getattr(r, "_grad_norm_accum", None) is None
    r.close()


# ------------------------------------------------------------------------------------------------------ 7. non-interference
def test_the_reference_strategy_is_untouched_by_an_adc_trainer_before_it():
    """Twelve steps and one event of a strategy="reference" trainer on a context that an ADC trainer has used before, against
    the same on a fresh context: the same bits where two fresh runs are bit-identical themselves, else within their spread
    (the blend backward's float atomics: the module docstring)."""
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = _scene()
    start = perturb(p, 5, 0.3)

    def reference_run(r, targets):
        model = GaussModel(start, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000)
        tr.plannedDensify = False
        tr.noiseSource = "library"
        for it in range(12):
            tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
        acc = tr.xyzGradAccumulation.clone()
        tr.densifyFromIter = 1
        st = tr.split_and_prune(12)
        return st, acc, model.arena.clone()

    out = []
    for before in (False, False, True):
        r = _renderer()
        targets = _targets(r, p, cams)
        if before:
            m2 = GaussModel(start, r.device)
            t2 = GaussianTrainer(m2, r, iterationCount=1000, strategy="adc", adc=_adc_config(cams))
            for it in range(22):
                t2.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
            print(f"the ADC trainer before it: N {N} -> {m2.N}, {t2.lastADCStats}")
            assert t2.lastADCStats is not None and getattr(r, "_adc_stats", None) is None
            r._work_hints.clear()                           # (the views' scheduling hints and cuts are the renderer's, not the strategy's)
            r._cut_policy.clear()
        out.append(reference_run(r, targets))
        assert r.lib.gs_set_adc_stats(r.ctx, None, None, None) == 0
        r.close()
    (st_a, acc_a, ar_a), (st_b, acc_b, ar_b), (st_c, acc_c, ar_c) = out
    _spread_ok("the reference statistic after 12 steps", _np(acc_a), _np(acc_b), _np(acc_c), loop=True)
    if st_a == st_b and ar_a.shape == ar_b.shape:
        assert st_c == st_a, (st_a, st_c)
        _spread_ok("the reference model after its event", _np(ar_a), _np(ar_b), _np(ar_c), loop=True)
    else:       # two fresh runs already decide differently at a threshold (the atomics' noise): hold the counts to their spread
        for k in st_a:
            assert abs(st_c[k] - st_a[k]) <= max(4 * abs(st_a[k] - st_b[k]), 2), (k, st_a, st_b, st_c)
