"""Per-pixel loss masks on the device (include/gsplat.h gs_set_loss_mask, GaussianRenderer.setLossMask,
GaussianTrainer.trainStep(lossMask=...)) against the unmasked kernel on images weighted beforehand, and against the oracle's
loss composed with the numpy restatement (tests/loss_mask_numpy.py).

Bars, fixed before the first run on the card:
  - a mask of all 255, and no mask after another one: loss[4] and cotangent torch.equal to the unmasked call's;
  - the identity, exact: with w = v / 255 (loss_mask.weights: numpy's correctly rounded float32 quotient, uploaded -- torch's
    division by a host scalar multiplies by the reciprocal and is not that), the masked loss of (R, G) is torch.equal to the
    unmasked loss of (w R, w G) and its cotangent torch.equal to w times that call's; exactly zero where v = 0, finite
    everywhere.  This is the specification: it holds only if the kernel's weight is the correctly rounded quotient and its
    final multiply by w is not contracted into what comes before;
  - the three target-cache modes give the same bits under a mask, and a key filled under one mask is refilled under another,
    after an in-place write to the mask, and without one;
  - oracle: loss within 2e-6 of the float32 mirror, cotangent within 1e-3 of its largest component (the project's bars from
    test_gpu_parity.test_loss_forward_backward; on these inputs the float32 oracle itself is <= 6e-8 / <= 7e-7 from the float64
    one, far inside both);
  - corrections: identity exposure / identity grid under a mask give the masked plain loss's bits; a random exposure gives
    loss[4] torch.equal to the masked plain loss of applyExposure(render, M), and dL/dM within 1e-3 of the largest component of
    sum_p cotE_p (x) [r_p, 1] summed in float64 from that call's own cotangent cotE;
  - a step: trainStep(lossMask=m) leaves the model, the moments and the loss torch.equal to the manual sequence.  The blend
    backward adds a Gaussian's per-block contributions with float atomics, in an order that varies from run to run: on a
    random scene two runs of the SAME manual sequence differ (measured at 64 x 64, 300 Gaussians: 1e-10 in the parameters and
    moments), so bits say nothing there.  The step test's scene therefore keeps every splat inside one 16 x 16 block (one
    contribution per Gaussian: nothing to reorder), where the identity under test is exact; the other trainer tests use
    the random scene;
  - what it is for: two runs of 30 steps are compared, no absolute number is fixed.

Shapes: the loss tile is 32 x 32 with a 10-pixel halo on each side -- (37, 53) has one partial tile column and row with the
halo outside the image, (120, 160) and (152, 200) several tiles with partial last ones."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_BAR, GRAD_BAR = 2e-6, 1e-3
SHAPES = [(37, 53), (120, 160), (152, 200)]
MASKS = ["binary", "soft", "tile_edge", "rect", "zeros", "all255"]


def _load(name):
    spec = importlib.util.spec_from_file_location("_lmg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ge = _load("test_gpu_exposure")
en = _load("exposure_numpy")
bgn = _load("bilateral_grid_numpy")
lmn = _load("loss_mask_numpy")
traj = _load("test_gpu_trajectory")


def _renderer(W, H):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, (16, 16), False)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _masks(H, W):
    rng = np.random.default_rng(7)
    full = np.full((H, W), 255, np.uint8)
    edge, rect = full.copy(), full.copy()
    edge[:, 32:] = 0                     # an edge on a tile boundary
    rect[10:30, 20:45] = 0               # an edge inside tiles
    return dict(binary=(rng.uniform(size=(H, W)) > 0.5).astype(np.uint8) * np.uint8(255),
                soft=rng.integers(0, 256, (H, W)).astype(np.uint8), tile_edge=edge, rect=rect,
                zeros=np.zeros((H, W), np.uint8), all255=full)


def _weights(mask):
    from gaussiansplattingmlx_amd.loss_mask import weights
    return _dev(weights(mask))[..., None]


def _loss(r, ren, tgt, key=None):
    """(loss[4], cotangent) as device tensors of their own."""
    lo, cot, _ = r.lossForwardBackward(ren, tgt, 0.2, targetKey=key)
    return lo.clone(), cot.clone()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


_scenes = {}


def _scene(H, W):
    """The images of one shape, on the device, with the unmasked result: computed once, never written."""
    if (H, W) not in _scenes:
        ren, tgt, _ = ge._images(H, W)
        r = _renderer(W, H)
        ren_d, tgt_d = _dev(ren), _dev(tgt)
        _scenes[(H, W)] = dict(r=r, ren=ren, tgt=tgt, ren_d=ren_d, tgt_d=tgt_d, plain=_loss(r, ren_d, tgt_d), masks=_masks(H, W))
    return _scenes[(H, W)]


# ------------------------------------------------------------------------------------------------------------ off is off
@pytest.mark.parametrize("H,W", SHAPES)
def test_all_255_is_off_and_nothing_sticks(H, W):
    s = _scene(H, W)
    r = s["r"]
    try:
        r.setLossMask(s["masks"]["all255"])
        assert r.lossMask.dtype == torch.uint8 and tuple(r.lossMask.shape) == (H, W)
        assert _same(_loss(r, s["ren_d"], s["tgt_d"]), s["plain"])
        r.setLossMask(np.ones((H, W), bool))                   # bool: 0 / 255
        assert bool((r.lossMask == 255).all())
        assert _same(_loss(r, s["ren_d"], s["tgt_d"]), s["plain"])
        r.setLossMask(s["masks"]["binary"])
        other = _loss(r, s["ren_d"], s["tgt_d"])
        assert not torch.equal(other[0], s["plain"][0]) and not torch.equal(other[1], s["plain"][1])
        r.setLossMask(None)
        assert r.lossMask is None
        assert _same(_loss(r, s["ren_d"], s["tgt_d"]), s["plain"])
        for bad in (np.zeros((H, W), np.float32), np.zeros((W, H) if H != W else (H, W + 1), np.uint8),
                    torch.zeros(H, W, device="cuda"), torch.zeros(H, W, 1, dtype=torch.uint8, device="cuda")):
            with pytest.raises(ValueError):
                r.setLossMask(bad)
        assert r.lossMask is None and _same(_loss(r, s["ren_d"], s["tgt_d"]), s["plain"])      # the refused calls bound nothing
    finally:
        r.setLossMask(None)
    from gaussiansplattingmlx_amd import _lib
    assert _lib.STATUS.get(r.lib.gs_set_loss_mask(None, None)) == "GS_ERR_INVALID_ARG"


# ------------------------------------------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("mask", MASKS)
def test_masked_loss_is_the_plain_loss_of_the_weighted_images(H, W, mask):
    s = _scene(H, W)
    r, m = s["r"], s["masks"][mask]
    w = _weights(m)
    rw, gw = s["ren_d"] * w, s["tgt_d"] * w
    want = _loss(r, rw, gw)
    try:
        r.setLossMask(_dev(m))
        got = _loss(r, s["ren_d"], s["tgt_d"])
    finally:
        r.setLossMask(None)
    print(f"{H}x{W} {mask}: loss {_np(got[0])} weighted-plain {_np(want[0])}; cotangent max diff "
          f"{float((got[1] - w * want[1]).abs().max()):.3g} of {float(want[1].abs().max()):.3g}")
    assert torch.equal(got[0], want[0]), (_np(got[0]), _np(want[0]))
    assert torch.equal(got[1], w * want[1])
    assert bool(torch.isfinite(got[1]).all())
    assert bool((got[1][_dev(m) == 0] == 0).all())
    if mask == "zeros":
        assert _np(got[0]).tolist() == [0.0, 0.0, 1.0, 0.0]     # L1 exactly 0, ssim exactly 1: costs nothing, pushes nothing
    if mask == "all255":
        assert _same(got, s["plain"])


# ------------------------------------------------------------------------------------------------------------ the cache
@pytest.mark.parametrize("H,W", [(37, 53), (120, 160)])
def test_target_cache_under_a_mask(H, W):
    s = _scene(H, W)
    r = s["r"]
    ren, tgt = s["ren_d"], s["tgt_d"]
    m1, m2 = _dev(s["masks"]["binary"]), _dev(s["masks"]["soft"])
    key = ("mask-cache", H, W)
    try:
        r.setLossMask(m1)
        base = _loss(r, ren, tgt)
        assert not _same(base, s["plain"])
        assert _same(_loss(r, ren, tgt, key), base)             # filling
        ident = r._target_cache[key][1]
        assert _same(_loss(r, ren, tgt, key), base)             # reading
        assert r._target_cache[key][1] == ident and r._target_cache[key][2] == 1
        r.setLossMask(m2)                                       # another mask under the same key: refilled, not served
        want = _loss(r, ren, tgt)
        assert not _same(want, base)
        assert _same(_loss(r, ren, tgt, key), want) and r._target_cache[key][1] != ident
        assert _same(_loss(r, ren, tgt, key), want)
        ident = r._target_cache[key][1]
        m2[: H // 2] = 0                                        # the bound mask written in place
        want2 = _loss(r, ren, tgt)
        assert not _same(want2, want)
        assert _same(_loss(r, ren, tgt, key), want2) and r._target_cache[key][1] != ident
        assert _same(_loss(r, ren, tgt, key), want2)
        r.setLossMask(None)                                     # unbound
        assert _same(_loss(r, ren, tgt, key), s["plain"])
        assert _same(_loss(r, ren, tgt, key), s["plain"])
    finally:
        r.setLossMask(None)
        r.invalidateTarget(key)


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("mask", ["binary", "soft", "rect"])
def test_masked_loss_matches_the_mirror(oracle32, mask):
    H, W = 152, 200
    s = _scene(H, W)
    r, m = s["r"], s["masks"][mask]
    try:
        r.setLossMask(m)                                        # a host array: uploaded here
        lo, cot = _loss(r, s["ren_d"], s["tgt_d"])
    finally:
        r.setLossMask(None)
    l32, c32, l1, ss = lmn.masked_loss(oracle32, s["ren"], s["tgt"], m, 0.2)
    lo, cot = _np(lo), _np(cot)
    rel = ge._rel(cot, c32)
    print(f"{mask}: loss {lo[0]:.9g} mirror {l32:.9g} (diff {abs(float(lo[0]) - l32):.3g}); cotangent {rel:.3g} of the largest component")
    assert abs(float(lo[0]) - l32) <= LOSS_BAR and abs(float(lo[1]) - l1) <= LOSS_BAR and abs(float(lo[2]) - ss) <= LOSS_BAR
    assert rel <= GRAD_BAR


# ------------------------------------------------------------------------------------------------------------ corrections
def _masked_plain(s, mask_d, image):
    r = s["r"]
    r.setLossMask(mask_d)
    try:
        return _loss(r, image, s["tgt_d"])
    finally:
        r.setLossMask(None)


def test_identity_corrections_under_a_mask():
    H, W = 37, 53
    s = _scene(H, W)
    r = s["r"]
    mask_d = _dev(s["masks"]["binary"])
    want = _masked_plain(s, mask_d, s["ren_d"])
    M, grad = ge._exposure(en.IDENTITY)
    shape = (4, 3, 2)
    G = _dev(bgn.identity(shape).astype(np.float32).reshape(-1))
    gG = torch.full_like(G, float("nan"))
    try:
        r.setLossMask(mask_d)
        r.setExposure(M, grad)
        assert _same(_loss(r, s["ren_d"], s["tgt_d"]), want)
        assert bool(torch.isfinite(grad).all())
        r.setExposure(None, None)
        r.setBilateralGrid(G, gG, shape, tv_weight=0.0)
        assert _same(_loss(r, s["ren_d"], s["tgt_d"]), want)
        assert bool(torch.isfinite(gG).all())
    finally:
        r.setExposure(None, None)
        r.setBilateralGrid(None, None)
        r.setLossMask(None)


def test_random_exposure_under_a_mask():
    H, W = 37, 53
    s = _scene(H, W)
    r = s["r"]
    m = s["masks"]["binary"]
    mask_d = _dev(m)
    Mh = en.random_exposure(np.random.default_rng(5))
    M, grad = ge._exposure(Mh)
    exposed = r.applyExposure(s["ren_d"], M)
    want = _masked_plain(s, mask_d, exposed)                    # its cotangent: cotE = dL/d(exposed render), weighted
    try:
        r.setLossMask(mask_d)
        r.setExposure(M, grad)
        lo, cot = _loss(r, s["ren_d"], s["tgt_d"])
        g = _np(grad).copy()
    finally:
        r.setExposure(None, None)
        r.setLossMask(None)
    assert torch.equal(lo, want[0]), (_np(lo), _np(want[0]))
    dr, dM = en.vjp(Mh, _np(want[1]), s["ren"])                 # float64 sums of cotE_p (x) [r_p, 1]
    print(f"dL/dM {ge._rel(g, dM):.3g}, dL/dr {ge._rel(_np(cot), dr):.3g} of the largest component")
    assert ge._rel(g, dM) <= GRAD_BAR, (g, dM)
    assert ge._rel(_np(cot), dr) <= GRAD_BAR
    assert not _np(cot)[m == 0].any()                           # the correction's backward keeps the zeros


# ------------------------------------------------------------------------------------------------------------ the trainer
SW, SH, SN = 64, 64, 300


def _step_scene():
    if "step" not in _scenes:
        _scenes["step"] = traj._scene(71, SN, SW, SH, 0.06)
    return _scenes["step"]


def _block_scene():
    """320 Gaussians of scale 0.02, twenty per 16 x 16 block of the 64 x 64 image of one camera, each centred within 1 pixel of
    its block's centre at depth 3 .. 4 (radii 3 and 6 pixels; the float32 oracle puts every splat's rectangle between 1.0 and
    15.0 pixels of its block's origin): no splat reaches a second block -- the test checks the radii and the pair count -- so the
    backward's sums have one term per Gaussian (see the header)."""
    if "block" not in _scenes:
        from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
        rng = np.random.default_rng(71)
        fx, fy = 0.9 * SW, 0.9 * SW * 1.02
        cam = Camera(SW, SH, fx, fy, look_at_c2w([2.2, -2.6, 1.7]))
        by, bx, _ = np.meshgrid(np.arange(SH // 16), np.arange(SW // 16), np.arange(20), indexing="ij")
        n = bx.size
        px = 8.5 + 16.0 * bx.reshape(-1) + rng.uniform(-1, 1, n)          # (a pixel's centre is at its index + 0.5)
        py = 8.5 + 16.0 * by.reshape(-1) + rng.uniform(-1, 1, n)
        z = rng.uniform(3.0, 4.0, n)
        pc = np.stack([(px - SW / 2) * z / fx, (py - SH / 2) * z / fy, z, np.ones(n)], 1)
        p = dict(xyz=(pc @ cam.c2w.T)[:, :3], features_dc=rng.normal(0, 1, (n, 1, 3)), features_rest=rng.normal(0, 0.004, (n, 24, 3)),
                 scales=np.full((n, 3), np.log(0.02)), rotation=rng.normal(0, 1, (n, 4)), opacity=rng.normal(0.3, 1.5, n))
        _scenes["block"] = ({k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, cam)
    return _scenes["block"]


def _params(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _trainer(r, p, **kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    model = GaussModel(p, r.device)
    kw.setdefault("densify", False)
    return GaussianTrainer(model, r, iterationCount=1000, **kw), model


def _half_mask():
    m = torch.full((SH, SW), 255, dtype=torch.uint8, device="cuda")
    m[:, SW // 2:] = 0
    return m


def _manual_step(p, cam, target, mask, fuse):
    """bind, renderForward, lossForwardBackward, the backward with Adam, unbind -- on a renderer and a model of its own."""
    from gaussiansplattingmlx_amd.trainer import GaussModel, arenaLearningRates, getLearningRates
    r = _renderer(SW, SH)
    m = GaussModel(p, r.device)
    r.setTuning(depth_gradient=0)
    r.setLossMask(mask)
    res = r.renderForward(m.getParams(), cam, wantDepth=False)
    loss, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    if fuse:
        r.renderBackwardAdam(cot, m.arena, m.m, m.v, getLearningRates(0, 1000))
    else:
        r.renderBackward(cot, out=m.getGrads())
        lrs = (C.c_float * 6)(*arenaLearningRates(0, 1000))
        seg = (C.c_longlong * 6)(*[int(x) for x in m.seg_end])
        p_ = lambda t: C.c_void_p(t.data_ptr())
        r._check(r.lib.gs_adam_step(r.ctx, m.numel, p_(m.arena), p_(m.grad), p_(m.m), p_(m.v), 6, seg, lrs, C.c_float(0.9),
                                    C.c_float(0.999), C.c_float(1e-15), C.c_float(1.0)))
    r.setLossMask(None)
    return loss.clone(), m


@pytest.mark.parametrize("fuse", [True, False])
def test_one_masked_step_is_the_manual_sequence(fuse):
    p, cam = _block_scene()
    cams = [cam]
    r = _renderer(SW, SH)
    res = r.renderForward(_params(p), cam, want_radii=True)
    r.sync()
    n = p["xyz"].shape[0]
    # what the scene is built for: a centre within 1.5 pixels of the block's and a radius of at most 6 keep a splat in its block
    assert int((res.radii > 0).sum()) == n and float(res.radii.max()) <= 6 and r.stats()["M"] <= n
    target = r.renderForward(_params(traj_perturbed(p)), cam).render.reshape(SH, SW, 3).clone()
    mask = _half_mask()
    was = torch.full((SH, SW), 255, dtype=torch.uint8, device="cuda")
    was[:8] = 0
    r.setLossMask(was)                                           # the renderer's own mask: put back behind the step
    tr, model = _trainer(r, p, fuse_adam=fuse)
    loss = tr.trainStep(cams[0], target, lossMask=mask).clone()
    assert r.lossMask is was
    loss2, m2 = _manual_step(p, cams[0], target, mask, fuse)
    again, m3 = _manual_step(p, cams[0], target, mask, fuse)
    print(f"fuse={fuse}: two manual runs bit-identical: arena {torch.equal(m2.arena, m3.arena)} m {torch.equal(m2.m, m3.m)} "
          f"v {torch.equal(m2.v, m3.v)}; trainStep vs manual max diff: arena {float((model.arena - m2.arena).abs().max()):.3g} "
          f"m {float((model.m - m2.m).abs().max()):.3g} v {float((model.v - m2.v).abs().max()):.3g}")
    assert torch.equal(loss, loss2) and float(loss2[0]) > 0
    assert bool(m2.m.any())
    assert torch.equal(model.arena, m2.arena) and torch.equal(model.m, m2.m) and torch.equal(model.v, m2.v)
    # the mask did its work: without it the step is another one
    tr0, model0 = _trainer(_renderer(SW, SH), p, fuse_adam=fuse)
    loss0 = tr0.trainStep(cams[0], target)
    assert not torch.equal(loss0, loss) and not torch.equal(model0.m, model.m)
    r.setLossMask(None)
    tr.trainStep(cams[0], target, lossMask=_np(mask) > 0)        # a host bool array
    assert r.lossMask is None
    for bad in (torch.zeros(SH, SW, device="cuda"), np.zeros((SH, SW + 1), np.uint8)):
        with pytest.raises(ValueError):
            tr.trainStep(cams[0], target, lossMask=bad)
        assert r.lossMask is None


def traj_perturbed(p):
    from gaussiansplattingmlx_amd.scenes import perturb
    return perturb(p, 5, 0.1)


def test_multi_view_steps_refuse_a_mask():
    p, cams = _step_scene()
    r = _renderer(SW, SH)
    tr, model = _trainer(r, p, views_per_rank=2)
    before = model.arena.clone()
    target = torch.zeros(SH, SW, 3, device="cuda")
    with pytest.raises(ValueError):
        tr.trainStep(cams[:2], [target, target], lossMask=_half_mask())
    assert r.lossMask is None and torch.equal(model.arena, before)


def test_a_masked_distractor_does_not_leak_into_the_kept_pixels():
    """The targets are the scene's own renders with a saturated rectangle painted over a quarter of the image: a distractor.
    Thirty steps with the rectangle masked out against thirty without a mask, both scored by the L1 distance from the CLEAN
    targets over the kept pixels."""
    p, cams = _step_scene()
    r = _renderer(SW, SH)
    clean = [r.renderForward(_params(p), c).render.reshape(SH, SW, 3).clone() for c in cams]
    mask = torch.full((SH, SW), 255, dtype=torch.uint8, device="cuda")
    mask[16:48, 16:48] = 0
    keep = mask == 255
    dirty = []
    for t in clean:
        d = t.clone()
        d[16:48, 16:48] = torch.tensor([1.0, 0.0, 1.0], device="cuda")
        dirty.append(d)
    score = {}
    for masked in (True, False):
        rr = _renderer(SW, SH)
        tr, model = _trainer(rr, p)
        for it in range(30):
            v = it % len(cams)
            loss = tr.trainStep(cams[v], dirty[v], viewKey=v, lossMask=mask if masked else None)
        assert np.isfinite(float(loss[0])) and bool(torch.isfinite(model.arena).all())
        out = [rr.renderForward(model.getParams(), c).render.reshape(SH, SW, 3) for c in cams]
        score[masked] = float(np.mean([float((o - t)[keep].abs().mean()) for o, t in zip(out, clean)]))
    print(f"L1 from the clean targets over the kept pixels after 30 steps: masked {score[True]:.3g}, unmasked {score[False]:.3g}")
    assert score[True] < score[False], score


@pytest.mark.parametrize("variant", ["background", "absgrad", "sparse_adam", "mcmc"])
def test_a_masked_step_composes(variant):
    p, cams = _step_scene()
    r = _renderer(SW, SH)
    res = r.renderForward(_params(traj_perturbed(p)), cams[0])
    target, alpha = res.render.reshape(SH, SW, 3).clone(), res.alpha.reshape(SH, SW).clone()
    step_kw = {}
    if variant == "background":
        from gaussiansplattingmlx_amd.background import BackgroundConfig
        kw = dict(background=BackgroundConfig(seed=3))
        step_kw = dict(targetAlpha=alpha)
    elif variant == "absgrad":
        from gaussiansplattingmlx_amd.absgrad import AbsGradConfig
        kw = dict(absgrad=AbsGradConfig(), densify=True)
    elif variant == "sparse_adam":
        kw = dict(sparse_adam=True)
    else:
        from gaussiansplattingmlx_amd.mcmc import MCMCConfig
        kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=int(SN * 1.2)))
    tr, model = _trainer(r, p, **kw)
    before = model.arena.clone()
    loss = tr.trainStep(cams[0], target, viewKey=0, lossMask=_half_mask(), **step_kw)
    assert np.isfinite(float(loss[0])) and float(loss[0]) > 0
    assert bool(torch.isfinite(model.arena[: model.numel]).all()) and not torch.equal(model.arena, before)
    assert r.lossMask is None
