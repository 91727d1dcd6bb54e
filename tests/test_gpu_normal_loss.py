"""Normal regularisation on the device (include/gsplat.h gs_normal_loss / gs_depth_normals, GaussianRenderer.normalLoss /
depthNormals, GaussianTrainer(normal=NormalConfig(...))) against the float64 restatement
(tests/normal_loss_numpy.py) and -- a train step -- against the oracle's loop and the manual call sequence.

Bars, fixed before the first run on the card; the float32 restatement's distance from float64 on the same inputs in brackets
(the worst of the three shapes and six settings, measured with this file's own comparison):
  - normals within 2e-4 absolute (2.5e-5, at 300 x 450), with the same pixels having one; each of the three terms and loss[0]
    within 2e-6 (1.1e-7);
  - every compared cotangent element within 1e-4 of its image's largest magnitude in the five settings with a prior term in the
    sum (2.4e-5: the issue's bar, met with its margin of four), and within 4e-4 for the smoothness term alone: its cotangents
    are differences of neighbouring normals, so the image's largest magnitude is small beside the rounding of what cancels, and
    the restatement itself is 3.7e-5 from float64 at 152 x 200 and 9.9e-5 at 300 x 450.  It does not meet 1e-4 with a margin
    there, so that one setting's bar is re-derived by the issue's rule, four times the restatement.  Compared are the pixels whose stencil (the pixel and
    its four neighbours) holds no prior component |n_c - Nt_c| < 2e-4 in float64: there float32 may take the other sign of the
    L1 term.  That leaves out at most 3 % of the pixels that have a normal (0.65 to 1.1 %); pixels that are not depth-valid are
    exactly 0.0f; the outputs are pre-filled with NaN and must come back finite;
  - max_jump is tested where no rounding changes a verdict (normal_loss_numpy.pick_max_jump: the gap is at least 150 x what
    float32 leaves of z);
  - two calls torch.equal; accumulate = 1 over an image torch.equal to that image plus the accumulate = 0 result;
  - (2, 64), (64, 2), (1, 1), an alpha of zeros and an island smaller than the stencil: terms 0, cotangents exactly 0, nothing
    NaN or Inf;
  - three train steps, fuse_adam on and off, against the oracle loop (render_forward, loss_forward_backward, the numpy normal term,
    render_backward with cotDepth / cotAlpha, Adam): test_gpu_trajectory's own bars, as test_gpu_depth_loss applies them;
  - a step is the manual sequence renderForward, lossForwardBackward, (depthLoss,) normalLoss, renderBackwardAdam with both
    cotangents, to the bit, on test_gpu_loss_mask's one-block-per-splat scene; normal=None and a step before normal.start are
    today's step to the bit; the renderer's depth_gradient knob is what it was before the step, also when the step raises;
  - what it is for: two runs of 60 steps are compared, no absolute number is fixed.

Measured on an MI355X: the kernels' distances from float64 are the restatement's to the printed digits in all eighteen cases
(normals 2.5e-5, terms 6.6e-8, loss[0] 1.1e-7, cotangents 9.9e-5 for the smoothness term alone at 300 x 450 and at most 2.4e-5
with a prior term); three steps: per-step loss 6.7e-8 from the float32 oracle loop (float64 loop: 1.8e-7), parameters 3.0e-5 of
the tensor's largest magnitude (5.7e-5), first moments 1.2e-5 (4.0e-5), second moments 5.7e-6 (3.4e-5), no element beyond 1e-3;
the layer: mean 1 - n_p . n_q 4.80e-3 at the start, 4.9e-5 after 60 steps with the term, 8.1e-5 without.

Shapes, chosen for the reductions (256 threads a block, at most 512 blocks): (37, 53) fewer pixels than one grid, (152, 200)
several blocks with rows that are no multiple of 64, (300, 450) more pixels than 512 x 256 threads -- the grid-stride loops wrap."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NORMAL_BAR, LOSS_BAR, COT_BAR, COT_BAR_SMOOTH_ALONE, TIE, TIE_SHARE = 2e-4, 2e-6, 1e-4, 4e-4, 2e-4, 0.03
SHAPES = [(37, 53), (152, 200), (300, 450)]
AMIN, GAMMA = 0.05, 2.0
# name: (weights, mask?, max_jump?, accumulate)
SETTINGS = {"l1": ((0.7, 0.0, 0.0), False, False, 0), "cos": ((0.0, 0.6, 0.0), False, False, 0),
            "smooth": ((0.0, 0.0, 0.9), False, False, 0), "all_masked": ((0.7, 0.6, 0.9), True, False, 0),
            "all_jump": ((0.7, 0.6, 0.9), True, True, 0), "all_jump_accumulate": ((0.7, 0.6, 0.9), True, True, 1)}
BASE = (0.25, 0.0, 0.0, 0.5)


def _load(name):
    spec = importlib.util.spec_from_file_location("_nlg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


nln = _load("normal_loss_numpy")
dlg = _load("test_gpu_depth_loss")
traj, lmg, ge, en = dlg.traj, dlg.lmg, dlg.ge, dlg.en


def _renderer(W, H):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, (16, 16), False)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


_cases = {}
_renderers = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_contexts():
    """The renderers and device images the tests of this file share live as long as the file's tests do, no longer."""
    yield
    for r in _renderers.values():
        r.close()
    _renderers.clear()
    _cases.clear()


def _r(H, W):
    if (H, W) not in _renderers:
        _renderers[(H, W)] = _renderer(W, H)
    return _renderers[(H, W)]


def _scene(H, W):
    """The scene of one shape with its max_jump and the images a call accumulates into: computed once, never written."""
    if (H, W) not in _cases:
        s = nln.scene(H, W)
        s["max_jump"], s["gap"], s["dropped"] = nln.pick_max_jump(s, AMIN)
        rng = np.random.default_rng([7, H, W])
        s["held"] = tuple(rng.uniform(-1e-4, 1e-4, (H, W)).astype(np.float32) for _ in range(2))
        _cases[(H, W)] = s
    return _cases[(H, W)]


def _kw(s, setting):
    lam, masked, jump, acc = SETTINGS[setting]
    return dict(target=s["target"], mask=s["mask"] if masked else None, edge=s["edge"], lam=lam, alpha_min=AMIN,
                max_jump=s["max_jump"] if jump else 0.0, gamma=GAMMA)


def _want(H, W, setting):
    """The float64 result of one shape and setting: computed once, never written."""
    if (H, W, setting) not in _cases:
        s = _scene(H, W)
        _cases[(H, W, setting)] = nln.normal_loss(s["K"], s["D"], s["a"], **_kw(s, setting))
    return _cases[(H, W, setting)]


def compare_with_float64(s, setting, want, normals, terms, loss0, cd, ca, tag):
    """What test_against_float64 asserts of one result (host arrays); used on the float32 restatement too, to measure the bars.
    Returns the figures."""
    lam, masked, jump, acc = SETTINGS[setting]
    has = want["has"]
    assert np.isfinite(normals).all() and np.isfinite(terms).all() and np.isfinite(cd).all() and np.isfinite(ca).all()
    assert np.array_equal((normals != 0).any(-1), has), "the pixels that have a normal differ"
    dn = float(np.abs(normals.astype(np.float64) - want["n"]).max())
    dt = float(np.abs(np.asarray(terms, np.float64) - np.asarray(want["terms"])).max())
    l64 = [float(np.float32(x)) for x in lam]
    d0 = abs(float(loss0) - (BASE[0] + sum(w * t for w, t in zip(l64, want["terms"]))))
    # the stencils a near tie of the L1 term reaches
    near = want["prior"] & (np.abs(want["n"] - want["Nt"]) < TIE).any(-1) if lam[0] > 0 else np.zeros_like(has)
    out = near.copy()
    out[:, 1:] |= near[:, :-1]
    out[:, :-1] |= near[:, 1:]
    out[1:] |= near[:-1]
    out[:-1] |= near[1:]
    share = float((out & has).sum()) / max(int(has.sum()), 1)
    figures = dict(normals=dn, terms=dt, loss0=d0, excluded=share)
    held = s["held"] if acc else (np.zeros_like(cd), np.zeros_like(ca))
    for name, got, w64, h in (("cot_depth", cd, want["cot_depth"], held[0]), ("cot_alpha", ca, want["cot_alpha"], held[1])):
        err = np.abs(got.astype(np.float64) - (w64 + h.astype(np.float64)))
        figures[name] = float(err[~out].max()) / float(np.abs(w64).max())
        assert not (got - h)[~want["valid"]].any(), name + ": a pixel that is not depth-valid is not exactly 0"
    print(f"{tag} {setting}: normals {dn:.3g}, terms {dt:.3g}, loss[0] {d0:.3g}, cot_depth {figures['cot_depth']:.3g} and cot_alpha "
          f"{figures['cot_alpha']:.3g} of the image's largest; excluded {share:.4f} of the pixels with a normal; "
          f"#normals {int(has.sum())}, counts {want['counts']}")
    assert dn <= NORMAL_BAR and dt <= LOSS_BAR and d0 <= LOSS_BAR
    assert share <= TIE_SHARE
    bar = COT_BAR if lam[0] > 0 or lam[1] > 0 else COT_BAR_SMOOTH_ALONE
    assert figures["cot_depth"] <= bar and figures["cot_alpha"] <= bar
    return figures


def _call(r, s, setting, held=None):
    """normalLoss under one setting into NaN-filled cotangents (or `held`, with accumulate) and a loss that holds BASE."""
    lam, masked, jump, acc = SETTINGS[setting]
    if "dev" not in s:
        s["dev"] = {k: _dev(s[k]) for k in ("D", "a", "target", "mask", "edge")}
    dev = s["dev"]
    out = dict(loss=torch.tensor(BASE, dtype=torch.float32, device="cuda"), terms=torch.full((3,), float("nan"), device="cuda"))
    if acc:
        held = s["held"] if held is None else held
        out.update(cotDepth=_dev(held[0]).clone(), cotAlpha=_dev(held[1]).clone())
    else:
        out.update(cotDepth=torch.full((r.H, r.W), float("nan"), device="cuda"), cotAlpha=torch.full((r.H, r.W), float("nan"), device="cuda"))
    p = r.normalLossParams(s["K"], *lam, alpha_min=AMIN, max_jump=s["max_jump"] if jump else 0.0, edge_gamma=GAMMA, accumulate=bool(acc))
    return r.normalLoss(dev["D"], dev["a"], s["K"], dev["target"], dev["mask"] if masked else None, dev["edge"], p, out=out)


# ------------------------------------------------------------------------------------------------------------ float64
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_against_float64(H, W, setting):
    s, want, r = _scene(H, W), _want(H, W, setting), _r(H, W)
    jump = SETTINGS[setting][2]
    if jump:
        print(f"{H}x{W}: max_jump {s['max_jump']:.6g} in a gap of {s['gap']:.3g}, drops {s['dropped']} pixels")
        assert s["gap"] >= 150 * 1.2e-7 and s["dropped"] >= 10
        assert int(_want(H, W, "all_masked")["has"].sum()) - int(want["has"].sum()) == s["dropped"]
    loss, terms, cd, ca = _call(r, s, setting)
    normals = r.depthNormals((s["dev"]["D"], s["dev"]["a"]), s["K"], AMIN, s["max_jump"] if jump else 0.0)
    assert tuple(normals.shape) == (H, W, 3)
    assert _np(loss)[1:].tolist() == list(BASE[1:])                              # loss[1..3] are left alone
    assert want["has"].any() and want["prior"].any() and not want["valid"].all()
    compare_with_float64(s, setting, want, _np(normals), _np(terms), float(loss[0]), _np(cd), _np(ca), f"{H}x{W}")
    assert _np(cd)[0, 1:-1].any() and _np(cd)[1:-1, 0].any()                    # border pixels do receive cotangents


# ------------------------------------------------------------------------------------------------------------ edges
def _raw(r, H, W, D, a, target, edge, lam=(0.7, 0.6, 0.9), K=None):
    """gs_normal_loss through the binding on images of a size of their own (H and W are the params'), NaN-filled outputs."""
    from gaussiansplattingmlx_amd import _lib
    K = K or (0.9 * W, 0.9 * W, W / 2 + 0.2, H / 2 - 0.3)
    p = _lib.gs_normal_loss_params(*K, H, W, *lam, AMIN, 0.0, GAMMA, 0)
    loss = torch.tensor(BASE, dtype=torch.float32, device="cuda")
    terms, cd, ca = (torch.full(shape, float("nan"), device="cuda") for shape in ((3,), (H, W), (H, W)))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    r._check(r.lib.gs_normal_loss(r.ctx, C.byref(p), ptr(D), ptr(a), ptr(target), None, ptr(edge), ptr(loss), ptr(terms), ptr(cd), ptr(ca)))
    return loss, terms, cd, ca


def _is_nothing(loss, terms, cd, ca):
    return (_np(loss).tolist() == list(BASE) and _np(terms).tolist() == [0.0, 0.0, 0.0]
            and bool((cd == 0).all()) and bool((ca == 0).all()))


def test_edges():
    r = _r(37, 53)
    for H, W in ((2, 64), (64, 2), (1, 1)):
        t = nln.scene(H, W)
        D, a, tg, ed = (_dev(t[k]) for k in ("D", "a", "target", "edge"))
        assert _is_nothing(*_raw(r, H, W, D, a, tg, ed)), (H, W)
        n = torch.full((H, W, 3), float("nan"), device="cuda")
        K4 = (C.c_float * 4)(0.9 * W, 0.9 * W, W / 2, H / 2)
        r._check(r.lib.gs_depth_normals(r.ctx, K4, H, W, C.c_void_p(D.data_ptr()), C.c_void_p(a.data_ptr()), C.c_float(AMIN),
                                        C.c_float(0.0), C.c_void_p(n.data_ptr())))
        assert bool((n == 0).all())
    s = _scene(37, 53)
    _call(r, s, "smooth")
    d = s["dev"]
    assert _is_nothing(*_raw(r, 37, 53, d["D"], torch.zeros_like(d["a"]), d["target"], d["edge"]))          # nothing blended anywhere
    assert _is_nothing(*_raw(r, 37, 53, torch.zeros_like(d["D"]), d["a"], d["target"], d["edge"]))
    island = torch.zeros_like(d["a"])
    island[10:12, 20:23] = 0.9                                               # 2 x 3 depth-valid pixels: no pixel has all four neighbours
    assert _is_nothing(*_raw(r, 37, 53, d["D"], island, d["target"], d["edge"]))
    assert not bool(r.depthNormals((d["D"], island), s["K"], AMIN).any())
    # a NULL target skips the prior terms whatever their weights: the smoothness term's result, to the bit
    loss, terms, cd, ca = _raw(r, 37, 53, d["D"], d["a"], None, d["edge"], K=s["K"])
    only = _raw(r, 37, 53, d["D"], d["a"], None, d["edge"], lam=(0.0, 0.0, 0.9), K=s["K"])
    assert _np(terms)[:2].tolist() == [0.0, 0.0] and float(terms[2]) > 0
    assert all(torch.equal(x, y) for x, y in zip((loss, terms, cd, ca), only))
    # no edge image: every pair weighs exactly 1, as with gamma = 0
    flat = r.normalLoss(d["D"], d["a"], s["K"], None, None, None, dict(smooth_weight=0.9, alpha_min=AMIN, edge_gamma=GAMMA))
    zero = r.normalLoss(d["D"], d["a"], s["K"], None, None, d["edge"], dict(smooth_weight=0.9, alpha_min=AMIN, edge_gamma=0.0))
    assert all(torch.equal(x, y) for x, y in zip(flat, zero)) and float(flat[1][2]) > float(terms[2])


def test_argument_errors():
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd._lib import GsplatError
    H, W = 37, 53
    r, s = _r(H, W), _scene(H, W)
    _call(r, s, "smooth")
    d = s["dev"]
    good = dict(l1_weight=0.1, cos_weight=0.1, smooth_weight=0.1, alpha_min=AMIN, max_jump=0.0, edge_gamma=1.0)
    r.normalLoss(d["D"], d["a"], s["K"], d["target"], d["mask"], d["edge"], good)
    nan, inf = float("nan"), float("inf")
    for bad, text in ((dict(l1_weight=-0.1), "lambda"), (dict(cos_weight=nan), "lambda"), (dict(smooth_weight=inf), "lambda"),
                      (dict(alpha_min=-0.01), "alpha_min"), (dict(alpha_min=nan), "alpha_min"), (dict(max_jump=-1.0), "max_jump"),
                      (dict(max_jump=inf), "max_jump"), (dict(edge_gamma=-1.0), "edge_gamma"), (dict(edge_gamma=nan), "edge_gamma")):
        with pytest.raises(GsplatError, match="GS_ERR_INVALID_ARG") as ei:
            r.normalLoss(d["D"], d["a"], s["K"], d["target"], d["mask"], d["edge"], dict(good, **bad))
        assert text in str(ei.value)
    for K in ((0.0, 40.0, 20.0, 20.0), (40.0, -1.0, 20.0, 20.0), (nan, 40.0, 20.0, 20.0), (40.0, 40.0, inf, 20.0)):
        with pytest.raises(GsplatError, match="GS_ERR_INVALID_ARG"):
            r.normalLoss(d["D"], d["a"], K, None, None, None, good)
        with pytest.raises(GsplatError, match="GS_ERR_INVALID_ARG"):
            r.depthNormals((d["D"], d["a"]), K)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    p = r.normalLossParams(s["K"], **good)
    z4, z3, img, img2 = torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda"), torch.empty(H, W, device="cuda"), torch.empty(H, W, device="cuda")
    args = [ptr(d["D"]), ptr(d["a"]), ptr(d["target"]), ptr(d["mask"]), ptr(d["edge"]), ptr(z4), ptr(z3), ptr(img), ptr(img2)]
    for i in (0, 1, 5, 6, 7, 8):                                            # depth, alpha, loss, normal_out, both cotangents
        broken = list(args)
        broken[i] = None
        assert _lib.STATUS.get(r.lib.gs_normal_loss(r.ctx, C.byref(p), *broken)) == "GS_ERR_INVALID_ARG"
        assert b"gs_normal_loss" in r.lib.gs_last_error(r.ctx)
    assert _lib.STATUS.get(r.lib.gs_normal_loss(r.ctx, None, *args)) == "GS_ERR_INVALID_ARG"
    for Hb, Wb in ((0, W), (H, -1)):
        q = _lib.gs_normal_loss_params(*s["K"], Hb, Wb, 0.1, 0.1, 0.1, AMIN, 0.0, 0.0, 0)
        assert _lib.STATUS.get(r.lib.gs_normal_loss(r.ctx, C.byref(q), *args)) == "GS_ERR_INVALID_ARG"
    with pytest.raises(ValueError):
        r.normalLoss(d["D"], d["a"], s["K"], d["target"], torch.zeros(H, W, device="cuda"), None, good)      # a float mask
    with pytest.raises(ValueError):
        r.normalLoss(d["D"], d["a"], s["K"], d["target"][:-1], None, None, good)
    with pytest.raises(ValueError, match="accumulate"):
        r.normalLoss(d["D"], d["a"], s["K"], None, None, None, dict(good, accumulate=True))               # nothing to add to


# ------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("H,W", SHAPES)
def test_determinism_and_accumulation(H, W):
    r, s = _r(H, W), _scene(H, W)
    first = _call(r, s, "all_masked")
    assert all(torch.equal(x, y) for x, y in zip(first, _call(r, s, "all_masked")))
    assert not torch.equal(first[2], _call(r, s, "smooth")[2])
    loss0, terms0, cd0, ca0 = _call(r, s, "all_jump")
    for held in (s["held"], (_np(cd0), -3.0 * _np(ca0))):
        loss1, terms1, cd1, ca1 = _call(r, s, "all_jump_accumulate", held=held)
        assert torch.equal(loss1, loss0) and torch.equal(terms1, terms0)
        assert torch.equal(cd1, _dev(held[0]) + cd0) and torch.equal(ca1, _dev(held[1]) + ca0)
    again = _call(r, s, "all_jump_accumulate")
    assert all(torch.equal(x, y) for x, y in zip(again, _call(r, s, "all_jump_accumulate")))


# ------------------------------------------------------------------------------------------------------------ depthNormals
@pytest.mark.parametrize("H,W", SHAPES)
def test_depth_normals(H, W):
    from gaussiansplattingmlx_amd.renderer import RenderResult
    r, s = _r(H, W), _scene(H, W)
    _call(r, s, "smooth")
    d = s["dev"]
    n = r.depthNormals((d["D"], d["a"]), s["K"], AMIN)
    want, has = nln.depth_normals(s["K"], s["D"], s["a"], AMIN)
    got = _np(n)
    assert np.array_equal((got != 0).any(-1), has) and float(np.abs(got - want).max()) <= NORMAL_BAR
    assert not got[0].any() and not got[-1].any() and not got[:, 0].any() and not got[:, -1].any()      # the border
    hole = ~nln.depth_valid(s["D"], s["a"], AMIN)
    assert hole.any()
    reach = hole.copy()
    reach[:, 1:] |= hole[:, :-1]
    reach[:, :-1] |= hole[:, 1:]
    reach[1:] |= hole[:-1]
    reach[:-1] |= hole[1:]
    assert not got[reach].any() and has[1:-1, 1:-1][~reach[1:-1, 1:-1]].all()                            # a hole, or a neighbour of one
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    fx, fy, cx, cy = s["K"]
    rays = np.stack([((i + 0.5) - cx) / fx, ((j + 0.5) - cy) / fy, np.ones((H, W))], -1)
    assert ((got * rays).sum(-1)[has] < 0).all()                                                          # facing the camera
    assert float(np.abs(np.linalg.norm(got[has], axis=-1) - 1.0).max()) <= 1e-6
    res = RenderResult(None, d["D"].view(H, W, 1), d["a"].view(H, W, 1), None, None)
    assert torch.equal(r.depthNormals(res, s["K"], AMIN), n)
    with pytest.raises(ValueError):
        r.depthNormals(RenderResult(None, None, d["a"], None, None), s["K"])
    # another image size than the renderer's: H and W are the call's own
    sub = r.depthNormals((d["D"][: H - 5, : W - 3].contiguous(), d["a"][: H - 5, : W - 3].contiguous()), s["K"], AMIN)
    wsub, _ = nln.depth_normals(s["K"], s["D"][: H - 5, : W - 3], s["a"][: H - 5, : W - 3], AMIN)
    assert float(np.abs(_np(sub) - wsub).max()) <= NORMAL_BAR


# ------------------------------------------------------------------------------------------------------------ the oracle
SW, SH, SN, STEPS = dlg.SW, dlg.SH, dlg.SN, dlg.STEPS
CFG = dict(l1_weight=0.3, cos_weight=0.2, smooth_weight=0.5, alpha_min=AMIN, edge_gamma=GAMMA)


def _K(cam):
    return (float(cam.focalX), float(cam.focalY), float(cam.principalX), float(cam.principalY))


def _normal_targets(o, p0, cams, seed=13):
    """Per view: the normals of the oracle's own depth image at p0, each component moved by 0.1 to 0.3 either way (the kernel
    normalises), and the mask of the pixels where every component of the normalised target stays at least 0.03 from the
    normal's: no sign of the L1 term is in doubt within three steps, in either loop."""
    rng = np.random.default_rng(seed)
    tns, masks = [], []
    for c in cams:
        fw = o.render_forward(p0, c.as_dict(), SW, SH, 16, 16, 4)
        n, has = nln.depth_normals(_K(c), fw["depth"].reshape(SH, SW), fw["alpha"].reshape(SH, SW), AMIN)
        t = n + rng.uniform(0.1, 0.3, n.shape) * rng.choice([-1.0, 1.0], n.shape)
        t[~has] = (0.0, 0.0, -1.0)
        unit = t / np.linalg.norm(t, axis=-1, keepdims=True)
        masks.append((has & (np.abs(unit - n).min(-1) > 0.03)).astype(np.uint8))
        tns.append(t.astype(np.float32))
        assert int(masks[-1].sum()) > 100
    return tns, masks


def _oracle_normal_loop(o, p0, cams, targets, tns, masks, steps=STEPS):
    """test_gpu_trajectory._oracle_loop with the normal term: render_forward, loss_forward_backward, the numpy normal term on the
    forward's depth and alpha, render_backward with its two cotangents, Adam."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    dt = o.dtype
    p = {k: v.astype(dt).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    b1, b2, eps, one = dt.type(0.9), dt.type(0.999), dt.type(1e-15), dt.type(1)
    losses = []
    for it in range(steps):
        vi = it % len(cams)
        cam = cams[vi].as_dict()
        fw = o.render_forward(p, cam, SW, SH, 16, 16, 4)
        loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(SH, SW, 3), targets[vi].astype(dt), 0.2)
        r = nln.normal_loss(_K(cams[vi]), fw["depth"].reshape(SH, SW), fw["alpha"].reshape(SH, SW), tns[vi], masks[vi], targets[vi],
                            (CFG["l1_weight"], CFG["cos_weight"], CFG["smooth_weight"]), AMIN, 0.0, GAMMA, dtype=dt.type)
        g = o.render_backward(p, cam, SW, SH, 16, 16, 4, fw, cot.reshape(-1, 3), r["cot_depth"].reshape(-1).astype(dt),
                              r["cot_alpha"].reshape(-1).astype(dt))
        losses.append(float(loss) + r["total"])
        lr = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
        for k in traj.KEYS:
            gk = np.asarray(g[k], dt).reshape(p[k].shape)
            m[k] = b1 * m[k] + (one - b1) * gk
            v[k] = b2 * v[k] + (one - b2) * gk * gk
            p[k] = (p[k] - dt.type(lr[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
    return losses, p, m, v


def _oracle_runs(oracle32, oracle64):
    """The scene, its targets and both oracle loops: computed once for fuse_adam on and off, never written."""
    if "oracle" not in _cases:
        from gaussiansplattingmlx_amd.scenes import perturb
        p0, cams = traj._scene(71, SN, SW, SH, 0.06)
        tp = perturb(p0, 5, 0.1)
        targets = [oracle32.render_forward(tp, c.as_dict(), SW, SH, 16, 16, 4)["color"].reshape(SH, SW, 3).copy() for c in cams]
        tns, masks = _normal_targets(oracle32, p0, cams)
        _cases["oracle"] = (p0, cams, targets, tns, masks, _oracle_normal_loop(oracle32, p0, cams, targets, tns, masks),
                            _oracle_normal_loop(oracle64, p0, cams, targets, tns, masks))
    return _cases["oracle"]


@pytest.mark.parametrize("fuse", [True, False])
def test_three_steps_against_the_oracle_loop(oracle32, oracle64, fuse):
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, GaussianTrainer, GaussModel, getLearningRates
    p0, cams, targets, tns, masks, (want_l, want_p, want_m, want_v), (ref_l, ref_p, ref_m, ref_v) = _oracle_runs(oracle32, oracle64)
    r = _renderer(SW, SH)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, fuse_adam=fuse, normal=NormalConfig(**CFG))
    got_l = []
    for it in range(STEPS):
        vi = it % len(cams)
        loss = tr.trainStep(cams[vi], _dev(targets[vi]), viewKey=vi, targetNormal=_dev(tns[vi]), normalMask=_dev(masks[vi]))
        got_l.append(float(loss[0]))
        assert all(float(x) > 0 for x in tr.lastNormalTerms) and float(loss[3]) == 0.0
    assert r.stats()["overflow"] == 0
    N = model.N
    got_p = {k: _np(model.getParams()[k]).copy() for k in traj.KEYS}
    got_m = {k: _np(model._carve(model.m, N)[k]).copy() for k in traj.KEYS}
    got_v = {k: _np(model._carve(model.v, N)[k]).copy() for k in traj.KEYS}
    rep = {}
    for tag, got, want, ref in (("param", got_p, want_p, ref_p), ("m", got_m, want_m, ref_m), ("v", got_v, want_v, ref_v)):
        traj._compare(tag, got, want, p0, rep)
        traj._compare("oracle32_vs_64." + tag, {k: ref[k] for k in traj.KEYS}, want, p0, rep)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    dref = np.abs(np.asarray(ref_l) - np.asarray(want_l))
    print(f"fuse {fuse}: loss {got_l}; |hip - oracle32| {dl.max():.3g}, |oracle64 - oracle32| {dref.max():.3g}")
    for tag in ("param", "m", "v"):
        for k in traj.KEYS:
            e, ref = rep[f"{tag}.{k}"], rep[f"oracle32_vs_64.{tag}.{k}"]
            print(f"  {tag}.{k}: max_rel {e['max_rel']:.3g} share_beyond {e['share_beyond']:.3g} | oracle64: max_rel "
                  f"{ref['max_rel']:.3g} share_beyond {ref['share_beyond']:.3g}")
    assert dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in traj.KEYS:
        for tag in ("m", "v"):
            e = rep[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = rep[f"param.{k}"], rep[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * STEPS * 1.01 + 1e-6, (k, e)


# ------------------------------------------------------------------------------------------------------------ composition
def _block_inputs():
    """test_gpu_depth_loss's inputs on the one-block-per-splat scene, and a normal prior: the scene's own depth normals (the
    device's) tilted, (0, 0, -1) where there is none."""
    if "block" not in _cases:
        p, cam, target, alpha, tds = dlg._block_inputs()
        r = _renderer(SW, SH)
        res = r.renderForward(lmg._params(p), cam, wantDepth=True)
        n = r.depthNormals(res, cam, AMIN)
        assert int((n != 0).any(-1).sum()) > 100
        tn = n + torch.tensor([0.2, -0.1, -0.3], device="cuda")
        tn[(n == 0).all(-1)] = torch.tensor([0.0, 0.0, -1.0], device="cuda")
        r.close()
        _cases["block"] = (p, cam, target, alpha, tds, tn.contiguous())
    return _cases["block"]


def _manual_normal_step(with_depth, fuse=True, prior=True):
    """renderForward, lossForwardBackward, (depthLoss,) normalLoss, the backward with both cotangents and Adam, on a renderer
    and a model of its own."""
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cam, target, alpha, tds, tn = _block_inputs()
    r = _renderer(SW, SH)
    m = GaussModel(p, r.device)
    r.setTuning(depth_gradient=1)
    res = r.renderForward(m.getParams(), cam, wantDepth=True)
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    out = dict(loss=loss)
    if with_depth:
        td = tds[with_depth]
        loss, cd, ca = r.depthLoss(res.depth, res.alpha, td, (td > 0).to(torch.uint8),
                                   r.depthLossParams(with_depth, 0.5, AMIN), out=dict(loss=loss, cotAlpha=r._empty(SH, SW)))
        out.update(cotDepth=cd, cotAlpha=ca)
    params = r.normalLossParams(cam, CFG["l1_weight"], CFG["cos_weight"], CFG["smooth_weight"], AMIN, 0.0, GAMMA,
                                accumulate=bool(with_depth))
    loss, terms, cd, ca = r.normalLoss(res.depth, res.alpha, cam, tn if prior else None, None, target, params, out=out)
    if fuse:
        r.renderBackwardAdam(cot, m.arena, m.m, m.v, getLearningRates(0, 1000), cotDepth=cd, cotAlpha=ca)
    else:
        r.renderBackward(cot, cd, ca, out=m.getGrads())
        dlg._adam(r, m)
    r.sync()
    return loss.clone(), terms.clone(), m


@pytest.mark.parametrize("with_depth,fuse,prior", [(0, True, True), (0, False, True), (0, True, False), (1, True, True),
                                                   ("accumulated", True, True), (2, False, True)])
def test_one_normal_step_is_the_manual_sequence(with_depth, fuse, prior):
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    p, cam, target, alpha, tds, tn = _block_inputs()
    mode = 0 if with_depth == "accumulated" else with_depth
    kw, step_kw = {}, {}
    if with_depth:
        kw = dict(depth=DepthConfig(mode=dlg.dln.MODES[mode], weight=0.5, alpha_min=AMIN))
        step_kw = dict(targetDepth=tds[mode])
    if prior:
        step_kw["targetNormal"] = tn
    r = _renderer(SW, SH)
    r.setTuning(depth_gradient=0)
    tr, model = lmg._trainer(r, p, fuse_adam=fuse, normal=NormalConfig(**CFG), **kw)
    loss = tr.trainStep(cam, target, viewKey=0, **step_kw).clone()
    assert r.getTuning("depth_gradient") == 0
    if with_depth == "accumulated":
        loss2, terms2, m2 = _manual_accumulated_step(fuse)
    else:
        loss2, terms2, m2 = _manual_normal_step(with_depth, fuse, prior)
    print(f"depth {with_depth} fuse {fuse} prior {prior}: loss {_np(loss)} manual {_np(loss2)}; terms {_np(tr.lastNormalTerms)}; "
          f"max diff arena {float((model.arena - m2.arena).abs().max()):.3g} m {float((model.m - m2.m).abs().max()):.3g}")
    assert torch.equal(loss, loss2) and torch.equal(tr.lastNormalTerms, terms2)
    assert float(terms2[2]) > 0 and (float(terms2[0]) > 0) == prior and (float(loss[3]) > 0) == bool(with_depth)
    assert bool(m2.m.any())
    assert torch.equal(model.arena, m2.arena) and torch.equal(model.m, m2.m) and torch.equal(model.v, m2.v)
    # the normal term did its work: without it the step is another one
    tr0, model0 = lmg._trainer(_renderer(SW, SH), p, fuse_adam=fuse, **kw)
    loss0 = tr0.trainStep(cam, target, viewKey=0, **{k: v for k, v in step_kw.items() if k != "targetNormal"})
    assert not torch.equal(loss0, loss) and not torch.equal(model0.m, model.m)


def _manual_accumulated_step(fuse):
    """The manual sequence with the depth term in its accumulated mode: that term then writes an alpha cotangent too, zeros, for
    the normal term to add to."""
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cam, target, alpha, tds, tn = _block_inputs()
    r = _renderer(SW, SH)
    m = GaussModel(p, r.device)
    r.setTuning(depth_gradient=1)
    res = r.renderForward(m.getParams(), cam, wantDepth=True)
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    td = tds[0]
    ca = torch.full((SH, SW), float("nan"), device="cuda")
    loss, cd, ca = r.depthLoss(res.depth, res.alpha, td, (td > 0).to(torch.uint8), r.depthLossParams(0, 0.5, AMIN),
                               out=dict(loss=loss, cotAlpha=ca))
    assert not bool(ca.any())
    params = r.normalLossParams(cam, CFG["l1_weight"], CFG["cos_weight"], CFG["smooth_weight"], AMIN, 0.0, GAMMA, accumulate=True)
    loss, terms, cd, ca = r.normalLoss(res.depth, res.alpha, cam, tn, None, target, params, out=dict(loss=loss, cotDepth=cd, cotAlpha=ca))
    assert bool(ca.any())
    r.renderBackwardAdam(cot, m.arena, m.m, m.v, getLearningRates(0, 1000), cotDepth=cd, cotAlpha=ca)
    r.sync()
    return loss.clone(), terms.clone(), m


@pytest.mark.parametrize("fuse", [True, False])
def test_before_start_and_without_a_config_the_step_is_todays(fuse):
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    p, cam, target, alpha, tds, tn = _block_inputs()
    loss2, m2 = lmg._manual_step(p, cam, target, None, fuse)          # wantDepth=False, depth_gradient=0: the step as it was
    for kw in ({}, dict(normal=NormalConfig(start=1, **CFG))):
        r = _renderer(SW, SH)
        tr, model = lmg._trainer(r, p, fuse_adam=fuse, **kw)
        assert tr._cotDepth is None and tr._cotAlpha is None and tr.lastNormalTerms is None
        loss = tr.trainStep(cam, target, **(dict(targetNormal=tn) if kw else {})).clone()
        assert torch.equal(loss, loss2)
        assert torch.equal(model.arena, m2.arena) and torch.equal(model.m, m2.m) and torch.equal(model.v, m2.v)
        assert r._fused["depth"] is None and tr._cotDepth is None and tr.lastNormalTerms is None      # no depth image, no buffer
        if kw:
            tr.trainStep(cam, target, targetNormal=tn)                # iteration 1 = start: the term runs
            assert float(tr.lastNormalTerms[2]) > 0 and r._fused["depth"] is not None
        else:
            with pytest.raises(ValueError, match="targetNormal"):
                tr.trainStep(cam, target, targetNormal=tn)


@pytest.mark.parametrize("knob", [0, 1])
def test_the_depth_gradient_knob_is_put_back(knob):
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    p, cam, target, alpha, tds, tn = _block_inputs()
    r = _renderer(SW, SH)
    r.setTuning(depth_gradient=knob)
    tr, model = lmg._trainer(r, p, normal=NormalConfig(**CFG))
    tr.trainStep(cam, target, targetNormal=tn)
    assert r.getTuning("depth_gradient") == knob
    before = model.arena.clone()
    # raised inside the step, behind the knob's change: the term's own inputs are looked at behind it, a loss mask is bound behind it
    for bad in (dict(targetNormal=tn[:-1]), dict(targetNormal=tn, normalMask=torch.zeros(SH, SW, device="cuda")),
                dict(normalMask=np.zeros((SH, SW + 1), np.uint8)), dict(targetNormal=tn, lossMask=torch.zeros(SH, SW, device="cuda"))):
        with pytest.raises(ValueError):
            tr.trainStep(cam, target, **bad)
        assert r.getTuning("depth_gradient") == knob and tr._normalStep is None
    assert torch.equal(model.arena, before)
    tr.trainStep(cam, target)                                       # without a prior: the smoothness term alone
    assert _np(tr.lastNormalTerms)[:2].tolist() == [0.0, 0.0] and float(tr.lastNormalTerms[2]) > 0
    assert r.getTuning("depth_gradient") == knob


@pytest.mark.parametrize("variant", ["exposure", "loss_mask", "mcmc"])
def test_a_normal_step_composes(variant):
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    p, cams = lmg._step_scene()
    r = _renderer(SW, SH)
    res = r.renderForward(lmg._params(lmg.traj_perturbed(p)), cams[0], wantDepth=True)
    target = res.render.reshape(SH, SW, 3).clone()
    tn = r.depthNormals(res, cams[0], AMIN).clone()                  # (holes where the perturbed scene has no normal)
    kw, step_kw = {}, {}
    if variant == "mcmc":
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=int(lmg.SN * 1.2)))
    elif variant == "exposure":
        kw = dict(exposure_opt=True, n_views=1)
    else:
        step_kw = dict(lossMask=lmg._half_mask())
    tr, model = lmg._trainer(r, p, normal=NormalConfig(l1_weight=(1.0, 0.01), cos_weight=0.2, smooth_weight=0.5, max_jump=0.5,
                                                       edge_gamma=GAMMA), **kw)
    before = model.arena.clone()
    loss = tr.trainStep(cams[0], target, viewKey=0, targetNormal=tn, **step_kw)
    assert np.isfinite(float(loss[0])) and all(float(x) > 0 for x in tr.lastNormalTerms)
    assert bool(torch.isfinite(model.arena[: model.numel]).all()) and not torch.equal(model.arena, before)


# ------------------------------------------------------------------------------------------------------------ what it is for
LAYER_SPREAD, LAYER_WEIGHT = 0.5, 10.0


def _layer_runs(spread, weight, steps=60):
    """{with the term?: (roughness at the start, after `steps` steps)} of the jittered layer below."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.normal_loss import NormalConfig
    rng = np.random.default_rng(5)
    cam = Camera(SW, SH, 0.9 * SW, 0.9 * SW * 1.02, look_at_c2w([2.2, -2.6, 1.7]))
    jitter = rng.uniform(-0.5, 0.5, (2, 256))
    truth = dlg._layer(cam, 4.0, jitter)
    start = dlg._layer(cam, rng.uniform(4.0 - spread, 4.0 + spread, 256), jitter)
    r = _renderer(SW, SH)
    target = r.renderForward(lmg._params(truth), cam).render.reshape(SH, SW, 3).clone()
    r.close()

    def roughness(rr, params):
        n = rr.depthNormals(rr.renderForward(params, cam, wantDepth=True), cam, AMIN)
        has = (n != 0).any(-1)
        pr, pd = has[:, :-1] & has[:, 1:], has[:-1] & has[1:]
        total = (1 - (n[:, :-1] * n[:, 1:]).sum(-1))[pr].sum() + (1 - (n[:-1] * n[1:]).sum(-1))[pd].sum()
        pairs = int(pr.sum()) + int(pd.sum())
        assert pairs > 4000
        return float(total) / pairs

    out = {}
    for with_term in (True, False):
        rr = _renderer(SW, SH)
        tr, model = lmg._trainer(rr, start, **(dict(normal=NormalConfig(smooth_weight=weight)) if with_term else {}))
        e0 = roughness(rr, model.getParams())
        for _ in range(steps):
            loss = tr.trainStep(cam, target, viewKey=0)
        assert np.isfinite(float(loss[0])) and bool(torch.isfinite(model.arena[: model.numel]).all())
        out[with_term] = (e0, roughness(rr, model.getParams()))
        rr.close()
    return out


def test_the_smoothness_term_flattens_a_jittered_layer():
    """A layer of blobs of one colour in front of one camera, every blob moved along its view ray to a depth within LAYER_SPREAD
    of 4 (its size scaled with it): the training view is a uniform colour, which any depth renders alike, and the normals of its
    depth image point every way the jitter tilts them.  Sixty steps with NormalConfig(smooth_weight=LAYER_WEIGHT) against sixty
    without: the mean 1 - n_p . n_q of depthNormals over the pairs of neighbouring pixels that both have a normal."""
    out = _layer_runs(LAYER_SPREAD, LAYER_WEIGHT)
    print(f"mean 1 - n_p . n_q over the layer's pairs: start {out[True][0]:.4g}; after 60 steps with the smoothness term "
          f"{out[True][1]:.4g}, without {out[False][1]:.4g}")
    assert abs(out[True][0] - out[False][0]) < 1e-6 and out[True][0] > 1e-3
    assert out[True][1] < out[True][0] and out[True][1] < out[False][1], out
