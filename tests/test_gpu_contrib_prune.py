"""Contribution-based pruning on the device (include/gsplat.h gs_blend_contrib / gs_render_contrib / gs_contrib_actions,
GaussianTrainer(contrib_prune=...)) against gaussiansplattingmlx_amd/contrib_prune.py in float64 on the oracle's lists.

Bars, fixed before the first run on the card.
  max_w   1e-4 absolute -- the project's image bar: with unit colours the image IS the sum of these weights, so the bar that
          holds for the sum holds for a term; it also covers a pixel whose stop falls one entry later in float32 (the entry behind
          a stop weighs less than T_STOP = 1e-4).
  sum_w   test_gpu_parity's gradient metric, max |a - b| / max |b| <= 1e-3: like the gradients a per-Gaussian sum over pixels
          accumulated with float atomics.
  Occluded and off-screen Gaussians: exactly 0.0 in both.
  Gradients after a scoring pass: GRAD_BAR = 1e-3 in the same metric, against the gradients taken without it.
  Prune decisions: the threshold is the midpoint of the widest gap between consecutive float64 scores inside [0.005, 0.2], and
          the gap is asserted to be at least 4e-4 (twice the max_w bar on each side): no float32 score within the bar can sit on
          the other side.  Nothing is excluded.
  Renders after the prune: threshold x (the largest number of pruned entries in any pixel's list) x max |colour|, computed in
          float64 from the oracle's lists -- every pruned entry moved a pixel by at most w |colour| <= threshold |colour|, and
          the weights of the entries behind it grow by no more than what it took (plus the image bar for the two renders' own
          float32 arithmetic).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import contrib_prune as cp
from gaussiansplattingmlx_amd import filter3d as f3

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
MAX_BAR, SUM_BAR, GRAD_BAR, IMG_BAR = 1e-4, 1e-3, 1e-3, 1e-4
W, H = 160, 120


def _load(name):
    spec = importlib.util.spec_from_file_location("_cbp_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_contrib_prune_cpu")
traj = _load("test_gpu_trajectory")
f3cpu = _load("test_filter3d_cpu")
aacpu = _load("test_antialiasing_cpu")


def _renderer(w, h, tile=(16, 16), aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, w, h, tile, False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _zeros(n):
    return torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")


def _check_scores(tag, got_max, got_sum, want_max, want_sum):
    em, es = np.abs(_np(got_max).astype(np.float64) - want_max).max(), _rel(_np(got_sum), want_sum)
    print(f"{tag}: max_w err {em:.3e} (bar {MAX_BAR:.0e}), sum_w rel {es:.3e} (bar {SUM_BAR:.0e})")
    assert em <= MAX_BAR
    assert es <= SUM_BAR


# --------------------------------------------------------------------------------------------------------- 1. op level
OP_CASES = {"partial_blocks": dict(W=48, H=40, tile=(16, 16), N=300, kw={}),
            "deep_lists": dict(W=64, H=48, tile=(16, 16), N=4000, kw=dict(layer_depth=5.5, radius=(8.0, 20.0))),
            "tile_32": dict(W=64, H=64, tile=(32, 32), N=500, kw={})}
_op_cache = {}


def _op_case(name, oracle64):
    if name not in _op_cache:
        c = OP_CASES[name]
        s = cpu.op_scene(c["W"], c["H"], c["N"], seed=17, **c["kw"])
        bn = oracle64.tile_bin(s["rectMin"], s["rectMax"], s["radii"], s["depths"], c["W"], c["H"], c["tile"][0], c["tile"][1])
        want = cp.blend_weights(s["packed"], bn.sortedIdx, bn.tileRanges, c["W"], c["H"], c["tile"][0], c["tile"][1])
        _op_cache[name] = (c, s, bn, want)
    return _op_cache[name]


def _op_run(r, s, bn, maxW, sumW):
    info = r.buildGlobalTileSliceInfo((s["rectMin"], s["rectMax"]), s["radii"], s["depths"])
    if bn is not None:        # both sides sweep identical lists
        assert np.array_equal(_np(info["sortedGaussIdx"]).astype(np.uint32), bn.sortedIdx)
        assert np.array_equal(_np(info["tileRanges"]).astype(np.uint32), bn.tileRanges)
    return r.blendContrib(s["packed"], maxW, sumW)


@pytest.mark.parametrize("name", list(OP_CASES))
def test_op_level_scores_match_float64(oracle64, name):
    c, s, bn, (want_max, want_sum) = _op_case(name, oracle64)
    if name == "deep_lists":      # longer than one LDS chunk and than GS_SEG_LEN, and the pixels stop inside the list
        first_layer = int(np.where(s["packed"][:, 9] == np.float32(0.95))[0][0])
        pos = [int(np.where(bn.sortedIdx[a:b] == first_layer)[0][0]) for a, b in bn.tileRanges]
        assert min(pos) > 256 and bn.B > max(pos) + 256
        assert (want_max[s["depths"] > 6.0] == 0).all()
    r = _renderer(c["W"], c["H"], c["tile"])
    maxW, sumW = _zeros(c["N"])
    _op_run(r, s, bn, maxW, sumW)
    _check_scores(name, maxW, sumW, want_max, want_sum)
    for what in ("occluded", "offscreen"):
        assert not want_max[s[what]].any()
        assert not bool(maxW[torch.as_tensor(s[what], device="cuda")].any()), what
        assert not bool(sumW[torch.as_tensor(s[what], device="cuda")].any()), what
    assert float(sumW[s["spanning"]]) > 0.05 * c["W"] * c["H"]


# ------------------------------------------------------------------------------------- 2. determinism and accumulation
def test_max_is_bit_identical_and_both_accumulate(oracle64):
    c, s, bn, _ = _op_case("deep_lists", oracle64)
    r = _renderer(c["W"], c["H"], c["tile"])
    a_max, a_sum = _zeros(c["N"])
    _op_run(r, s, bn, a_max, a_sum)
    b_max, b_sum = _zeros(c["N"])
    _op_run(r, s, None, b_max, b_sum)
    assert torch.equal(a_max, b_max)                                  # two runs: the same bits
    assert _rel(_np(b_sum), _np(a_sum)) <= SUM_BAR
    first_max, first_sum = a_max.clone(), a_sum.clone()
    _op_run(r, s, None, a_max, a_sum)                                 # once more into the same buffers
    assert torch.equal(a_max, first_max)
    assert _rel(_np(a_sum), 2.0 * _np(first_sum).astype(np.float64)) <= SUM_BAR
    # one output only: the other buffer is not touched
    only_sum = torch.zeros(c["N"], device="cuda")
    assert r.blendContrib(s["packed"], None, only_sum)[0] is None
    assert _rel(_np(only_sum), _np(first_sum)) <= SUM_BAR
    only_max = torch.zeros(c["N"], device="cuda")
    r.blendContrib(s["packed"], only_max, None)
    assert torch.equal(only_max, first_max)
    with pytest.raises(ValueError):
        r.blendContrib(s["packed"], None, None)
    assert r.lib.gs_blend_contrib(r.ctx, c["N"], r._t(s["packed"]).data_ptr(), None, None) == 1      # GS_ERR_INVALID_ARG
    # accumulation keeps what is larger already
    big = torch.full((c["N"],), 2.0, device="cuda")
    r.blendContrib(s["packed"], big, None)
    assert bool((big == 2.0).all())


# -------------------------------------------------------------------------------------------------------- 3. fused path
_scene_cache = {}


def _scene():
    if "scene" not in _scene_cache:
        _scene_cache["scene"] = traj._scene(71, 3000, W, H, 0.06)
    return _scene_cache["scene"]


def _want_fused(oracle64, variant, n_cams):
    """Per camera (max_w, sum_w, forward dict) of the float64 rule on the matching composed oracle's records and lists."""
    key = ("want", variant)
    have = _scene_cache.setdefault(key, [])
    p, cams = _scene()
    if variant == "plain":
        o = oracle64
    elif variant == "aa":
        o = aacpu.AAOracle(oracle64)
    else:
        o = f3cpu.Filter3DOracle(oracle64, _filter(), False)
    while len(have) < n_cams:
        fw = o.render_forward(p, cams[len(have)].as_dict(), W, H, 16, 16, 4)
        m, s = cp.blend_weights(fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, 16, 16)
        have.append((m, s, fw))
    return have[:n_cams]


def _filter():
    p, cams = _scene()
    return f3.filter_width(p["xyz"], cams).astype(np.float32)


@pytest.mark.parametrize("variant", ["plain", "aa", "filter3d"])
def test_fused_scores_match_float64(oracle64, variant):
    p, cams = _scene()
    want_max, want_sum, _ = _want_fused(oracle64, variant, 1)[0]
    r = _renderer(W, H, aa=variant == "aa")
    if variant == "filter3d":
        r.setFilter3D(torch.as_tensor(_filter(), device="cuda"))
    r.renderChecked(_dev(p), cams[0])
    maxW, sumW = _zeros(3000)
    r.renderContrib(maxW, sumW)
    _check_scores("fused " + variant, maxW, sumW, want_max, want_sum)
    assert (want_max == 0).sum() > 0 and not bool(maxW[torch.as_tensor(want_max == 0, device="cuda")].any())
    if variant != "plain":        # (the mode matters on this scene)
        plain = _want_fused(oracle64, "plain", 1)[0][0]
        assert np.abs(plain - want_max).max() > 10 * MAX_BAR


def test_fused_scores_on_block_lists(oracle64):
    """A tile size that is not a multiple of 16: the fused path's block lists against the reference's semantics at that
    tile size (every Gaussian of a pixel's tile blended)."""
    p, cams = _scene()
    fw = oracle64.render_forward(p, cams[0].as_dict(), W, H, 50, 38, 4)
    want_max, want_sum = cp.blend_weights(fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, 50, 38)
    r = _renderer(W, H, (50, 38))
    assert r.blockLists
    r.renderChecked(_dev(p), cams[0])
    maxW, sumW = _zeros(3000)
    r.renderContrib(maxW, sumW)
    _check_scores("fused block lists", maxW, sumW, want_max, want_sum)
    # ... and the op-level form at that tile size (the caller's tile grid, a tile's list swept per block)
    pr, bn = fw["proj"], fw["bin"]
    r.buildGlobalTileSliceInfo((pr["rectMin"], pr["rectMax"]), pr["radii"], pr["depths"])
    m2, s2 = _zeros(3000)
    r.blendContrib(fw["packed"], m2, s2)
    _check_scores("op level 50x38", m2, s2, want_max, want_sum)


def test_scoring_leaves_the_forward_usable():
    p, cams = _scene()
    r = _renderer(W, H)
    params = _dev(p)
    target = torch.rand(H, W, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))

    def step(score):
        res = r.renderChecked(params, cams[0])
        img, alpha, stats = res.render.clone(), res.alpha.clone(), r.stats()
        _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
        cot = cot.clone()
        if score:
            r.renderContrib(*_zeros(3000))
            assert torch.equal(res.render, img) and torch.equal(res.alpha, alpha) and r.stats() == stats
        return img, {k: v.clone() for k, v in r.renderBackward(cot).items()}
    img0, g0 = step(False)
    img1, g1 = step(True)
    assert torch.equal(img0, img1)
    for k in KEYS:
        assert _rel(_np(g1[k]), _np(g0[k])) <= GRAD_BAR, k


def test_scoring_refuses_what_a_backward_refuses():
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cams = _scene()
    r = _renderer(W, H)
    maxW, sumW = _zeros(3000)
    assert r.lib.gs_render_contrib(r.ctx, maxW.data_ptr(), sumW.data_ptr()) == 5          # GS_ERR_NO_FORWARD
    with pytest.raises(GsplatError):
        r.renderContrib(maxW, sumW)
    model = GaussModel(p, r.device)
    res = r.renderChecked(model.getParams(), cams[0])
    with pytest.raises(ValueError):
        r.renderContrib(None, None)
    assert r.lib.gs_render_contrib(r.ctx, None, None) == 1                                  # GS_ERR_INVALID_ARG
    _, cot, _ = r.lossForwardBackward(res.render, torch.zeros(H, W, 3, device="cuda"), 0.2)
    r.renderContrib(maxW, sumW)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, getLearningRates(0, 1000))     # consumes the parameters
    with pytest.raises(GsplatError) as eb:
        r.renderBackward(cot)
    with pytest.raises(GsplatError) as ec:
        r.renderContrib(maxW, sumW)
    assert eb.value.code == ec.value.code == 5
    assert not bool(maxW.isnan().any()) and float(maxW.max()) > 0.5


def test_contribution_scores_over_the_cameras(oracle64):
    p, cams = _scene()
    r = _renderer(W, H)
    params = _dev(p)
    single = []
    for c in cams:
        r.renderChecked(params, c)
        single.append(r.renderContrib(*_zeros(3000)))
    maxW, sumW = r.contributionScores(params, cams)
    assert torch.equal(maxW, torch.maximum(torch.maximum(single[0][0], single[1][0]), single[2][0]))
    assert _rel(_np(sumW), sum(_np(s[1]).astype(np.float64) for s in single)) <= SUM_BAR
    want = _want_fused(oracle64, "plain", 3)
    _check_scores("three cameras", maxW, sumW, np.maximum.reduce([w[0] for w in want]), sum(w[1] for w in want))
    with pytest.raises(ValueError):
        r.contributionScores(params, cams, viewKeys=[0, 1])


# --------------------------------------------------------------------------------------------------- 4. prune decisions
def _gap_threshold(score64):
    """The midpoint of the widest gap between consecutive sorted scores inside [0.005, 0.2], and that gap."""
    v = np.sort(np.asarray(score64, np.float64))
    v = v[(v >= 0.005) & (v <= 0.2)]
    assert v.size >= 2
    g = np.diff(v)
    k = int(np.argmax(g))
    return 0.5 * (v[k] + v[k + 1]), float(g[k])


def _pruned_entries_bound(fwds, pruned, tau):
    """tau x the largest number of pruned entries in any pixel's (= its tile's) list x max |colour| of a pruned record."""
    most, colour = 0, 0.0
    for fw in fwds:
        bn = fw["bin"]
        for a, b in bn.tileRanges:
            most = max(most, int(pruned[bn.sortedIdx[a:b].astype(np.int64)].sum()))
        colour = max(colour, float(np.abs(np.asarray(fw["packed"], np.float64)[pruned, 6:9]).max()))
    return tau * most * colour


def test_prune_decisions_and_the_pruned_model(oracle64):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    p, cams = _scene()
    want = _want_fused(oracle64, "plain", 3)
    want_max = np.maximum.reduce([w[0] for w in want])
    tau, gap = _gap_threshold(want_max)
    print(f"threshold {tau:.6f}, gap {gap:.3e}")
    assert gap >= 4e-4
    want_actions, want_counts = cp.contrib_actions(want_max, tau)
    r = _renderer(W, H)
    params = _dev(p)
    maxW, _ = r.contributionScores(params, cams)
    actions, counts = r.contribActions(maxW, tau)
    assert np.array_equal(_np(actions), want_actions) and np.array_equal(_np(counts), want_counts)
    keep = want_actions == 0
    assert 100 < keep.sum() < 2900
    before = [r.renderChecked(params, c).render.clone() for c in cams]
    for planned in (True, False):
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, densify=False)
        tr.plannedDensify = planned
        st = tr.pruneByContribution(cams, tau)
        assert st == tr.lastContribPruneStats == dict(N=3000, kept=int(keep.sum()), pruned=int((~keep).sum()), threshold=float(tau))
        assert model.N == int(keep.sum())
        for k in KEYS:
            assert np.array_equal(_np(model.getParams()[k]), p[k][keep]), (planned, k)      # the kept rows, in order, bit for bit
        assert not bool(model.m.any()) and not bool(model.v.any())
    bound = _pruned_entries_bound([w[2] for w in want], ~keep, tau)
    worst = max(float((r.renderChecked(model.getParams(), c).render - b).abs().max()) for c, b in zip(cams, before))
    print(f"render change after the prune: {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound + 2 * IMG_BAR
    assert worst > 0
    # a threshold below every score, and one above every score, change nothing
    for t in (1e-30, 1.0):
        n = model.N
        st = tr.pruneByContribution(cams, t)
        assert model.N == n and st["pruned"] == 0 and st["kept"] == n
    with pytest.raises(ValueError):
        tr.pruneByContribution([], tau)


# ----------------------------------------------------------------------------------------------------- 5. trainer event
def _targets(r, p, cams):
    from gaussiansplattingmlx_amd.scenes import perturb
    tp = _dev(perturb(p, 5, 0.1))
    return [r.renderChecked(tp, c).render.clone() for c in cams]


def _trainer(r, p, cams, densify, filter_3d, **kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    model = GaussModel(p, r.device)
    if filter_3d:
        kw.update(filter_3d=True, filter_cameras=cams)
    tr = GaussianTrainer(model, r, iterationCount=1000, densify=densify, **kw)
    tr.densifyFromIter, tr.split_and_prune_per_iteration = 1, 3          # densify events behind iterations 3, 6, 9
    return tr, model


@pytest.mark.parametrize("densify,filter_3d", [(False, True), (True, False)])
def test_trainer_event(oracle64, densify, filter_3d):
    p, cams = _scene()
    r = _renderer(W, H)
    targets = _targets(r, p, cams)
    # the state the event will see: a feature-off trainer driven identically through iteration 3 (its densify event included)
    off, m_off = _trainer(r, p, cams, densify, filter_3d)
    for it in range(4):
        off.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
    state = {k: _np(m_off.getParams()[k]).copy() for k in KEYS}
    N0 = m_off.N
    if densify:
        assert off.lastDensifyStats is not None and N0 != 3000            # (both kinds of event occur)
    filt = _np(off.filter3D()).astype(np.float64) if filter_3d else None
    o = f3cpu.Filter3DOracle(oracle64, filt, False) if filter_3d else oracle64
    score = np.zeros(N0)
    for c in cams:
        fw = o.render_forward(state, c.as_dict(), W, H, 16, 16, 4)
        score = np.maximum(score, cp.blend_weights(fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, 16, 16)[0])
    tau, gap = _gap_threshold(score)
    assert gap >= 4e-4
    kept = int((score >= tau).sum())
    print(f"densify={densify} filter_3d={filter_3d}: N {N0} at iteration 3, threshold {tau:.6f} (gap {gap:.3e}), predicted kept {kept}")
    r = _renderer(W, H)           # (a renderer without the first trainer's view hints)
    tr, model = _trainer(r, p, cams, densify, filter_3d, contrib_prune=cp.ContribPruneConfig(threshold=tau, at=(3,), cameras=cams))
    losses = []
    for it in range(12):
        losses.append(float(tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)[0]))
        if it < 3:
            assert tr.lastContribPruneStats is None
        if it == 3:
            assert tr.lastContribPruneStats == dict(N=N0, kept=kept, pruned=N0 - kept, threshold=float(tau))
            assert model.N == kept
            assert not bool(model.m.any()) and not bool(model.v.any())      # the optimizer state right after the event
            assert tr.xyzGradAccumulation.shape[0] == kept and tr.denomGradAccumulation == 0
            if filter_3d:
                want = f3.filter_width(_np(model.getParams()["xyz"]), cams)
                assert np.abs(_np(tr.filter3D()) - want).max() <= f3.width_bar(_np(model.getParams()["xyz"]), cams).max()
                assert np.array_equal(_np(tr.filter3D()), _np(r.computeFilter3D(model.getParams()["xyz"])))
    assert np.isfinite(losses).all(), losses
    assert tr.lastContribPruneStats["N"] == N0                             # one event only
    if not densify:
        assert model.N == kept
    assert r.filter3D is None


def test_off_is_off():
    """contrib_prune=None: the parameters of a 12-step run are those of a trainer built without the argument, bit for bit
    where that run is itself run-to-run identical (the blend backward's float atomics are not on every scene); where it is
    not, within the spread of two such runs as test_gpu_trajectory's harness measures a loop."""
    p, cams = _scene()
    r = _renderer(W, H)
    targets = _targets(r, p, cams)
    out = []
    for kw in ({}, {}, dict(contrib_prune=None)):
        tr, model = _trainer(r, p, cams, False, False, **kw)
        for it in range(12):
            tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
        assert tr.lastContribPruneStats is None
        out.append(model.arena.clone())
    a, b, c = (_np(t).astype(np.float64) for t in out)
    print(f"two runs without the argument: bit-identical = {np.array_equal(a, b)}, max diff {np.abs(a - b).max():.3e}; "
          f"contrib_prune=None against the first: max diff {np.abs(a - c).max():.3e}")
    if np.array_equal(a, b):
        assert np.array_equal(a, c)
    else:
        # two runs of the SAME trainer differ here (the atomics' order, carried through twelve Adam steps): the run with the
        # argument is held to test_gpu_trajectory's bar for such a loop (the share of elements beyond 1e-3 of the largest
        # stays below 1e-3), as the two runs without it are
        assert np.mean(np.abs(a - b) > 1e-3 * np.abs(a).max()) < 1e-3
        assert np.mean(np.abs(a - c) > 1e-3 * np.abs(a).max()) < 1e-3
