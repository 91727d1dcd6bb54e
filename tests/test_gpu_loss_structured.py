"""The loss and SSIM kernels (csrc/ssim.hip) on structured images and at the fused kernel's tile edges, against the float64
oracle.  Images, shapes and bars are tests/loss_numpy.py's; tests/test_loss_numpy_cpu.py shows on the
CPU that they reject six deliberate mistakes and that the allowance cannot swallow a failure.

Every bar is  error against Oracle(np.float64)  <=  1.5 err32 + floor,  err32 the float32 oracle's error in the same quantity
on the same input, and the floor one the suite already has: 2e-6 for loss, L1, mean ssim and the op-level maps
(test_loss_forward_backward, test_ssim_forward_backward), GRAD_RTOL u for the colour cotangent (u = (1 - lambda) / (3 P), the
L1 term at a pixel), GRAD_RTOL max|g64| for the op-level gradients.  None is taken from what the kernels give.

Each case prints what it measured -- error, err32, allowance -- and, where GS_TEST_REPORT_DIR names a directory, appends it to
loss_structured.json there (DESIGN.md's tables are that file's numbers)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT_DIR = os.environ.get("GS_TEST_REPORT_DIR", "")


def _load(name):
    spec = importlib.util.spec_from_file_location("_lsg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ln = _load("loss_numpy")
lmn = _load("loss_mask_numpy")
LAM = ln.LAMBDA
_renderers, _report = {}, []


def _renderer(H, W):
    """One renderer per shape, kept."""
    if (H, W) not in _renderers:
        if not torch.cuda.is_available():
            pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
        from gaussiansplattingmlx_amd.renderer import GaussianRenderer
        _renderers[(H, W)] = GaussianRenderer(4, W, H, (16, 16), False)
    return _renderers[(H, W)]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.as_tensor(np.array(a), device="cuda")          # (a copy: the shared references are read-only)


def _record(test, H, W, pair, measured, **extra):
    """Append one case to the report (rewritten whole each time: the file is this session's cases) and print it."""
    rec = dict(test=test, H=H, W=W, pair=pair, **extra,
               measured={k: dict(err=float(e), err32=float(e32), allow=float(a)) for k, (e, e32, a) in measured.items()})
    _report.append(rec)
    print(json.dumps(rec))
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "loss_structured.json"), "w") as f:
            json.dump(_report, f, indent=0)


def _fused(r, render, target, **kw):
    """dict(loss, l1, ssim, cot) of the fused kernel, plus the raw tensors (clones)."""
    lo, cot, cd = r.lossForwardBackward(render, target, LAM, **kw)
    lo, cot = lo.clone(), cot.clone()
    l = _np(lo)
    return dict(loss=l[0], l1=l[1], ssim=l[2], depth=l[3], cot=_np(cot)), lo, cot, (None if cd is None else cd.clone())


# ------------------------------------------------------------------------------------------------------------ fused loss
@pytest.mark.parametrize("H,W,name", ln.CASES)
def test_fused_loss_against_float64(oracle32, oracle64, H, W, name):
    ref = ln.reference(oracle32, oracle64, name, H, W)
    r = _renderer(H, W)
    ren, tgt = _dev(ref["render"]), _dev(ref["target"])
    got, lo, cot, _ = _fused(r, ren, tgt)
    b = ln.bars(got, ref["ref64"], ref["ref32"])
    _record("fused_loss", H, W, name, b, unit=ln.unit((H, W, 3)), max_cot64=float(np.abs(ref["ref64"]["cot"]).max()))
    assert np.isfinite(got["cot"]).all() and np.isfinite(_np(lo)).all()
    _, lo2, cot2, _ = _fused(r, ren, tgt)
    assert torch.equal(lo, lo2) and torch.equal(cot, cot2)
    assert ln.misses(b) == [], b


# ------------------------------------------------------------------------------------------------------------ target cache
@pytest.mark.parametrize("H,W", [(33, 65), (97, 161)])
@pytest.mark.parametrize("name", ["step_edge", "white_bg", "flat_equal"])
def test_target_cache_modes_are_bit_identical_on_structured_targets(oracle32, oracle64, name, H, W):
    """loss_fused_kernel's TCACHE = 1 (fills) and 2 (reads) against 0, on targets with flat regions and a step on the tile seam."""
    render, target = ln.reference(oracle32, oracle64, name, H, W, images_only=True)
    r = _renderer(H, W)
    ren, tgt = _dev(render), _dev(target)
    key = ("structured", name)
    try:
        _, lo0, cot0, _ = _fused(r, ren, tgt)
        _, lo1, cot1, _ = _fused(r, ren, tgt, targetKey=key)            # fills
        assert r._target_cache[key][2] == 1
        _, lo2, cot2, _ = _fused(r, ren, tgt, targetKey=key)            # reads
        assert torch.equal(lo1, lo0) and torch.equal(cot1, cot0), "filling"
        assert torch.equal(lo2, lo0) and torch.equal(cot2, cot0), "reading"
        _, lo3, cot3, _ = _fused(r, tgt.clone(), tgt, targetKey=key)    # reads, for another render: the target itself
        _, lo4, cot4, _ = _fused(r, tgt.clone(), tgt)
        assert torch.equal(lo3, lo4) and torch.equal(cot3, cot4), "reading for another render"
    finally:
        r._target_cache.pop(key, None)


# ------------------------------------------------------------------------------------------------------------ mask
def band_mask(H, W):
    """uint8: 0 on columns 27 ... 37, random 0 ... 255 elsewhere."""
    m = np.random.default_rng(H * 7 + W).integers(0, 256, (H, W), dtype=np.uint8)
    m[:, ln.ZERO_BAND[0]:ln.ZERO_BAND[1]] = 0
    return m


@pytest.mark.parametrize("H,W", ln.SHAPES_ALL_PAIRS)
@pytest.mark.parametrize("name", ["noise", "blobs_near", "white_bg", "step_edge"])
def test_masked_loss_against_float64(oracle32, oracle64, name, H, W):
    render, target = ln.reference(oracle32, oracle64, name, H, W, images_only=True)
    mask = band_mask(H, W)
    refs = []
    for o in (oracle32, oracle64):
        loss, cot, l1, ssim = lmn.masked_loss(o, render, target, mask, LAM)
        refs.append(dict(loss=loss, l1=l1, ssim=ssim, cot=np.asarray(cot, np.float64)))
    r = _renderer(H, W)
    try:
        r.setLossMask(mask)
        got, _, _, _ = _fused(r, _dev(render), _dev(target))
    finally:
        r.setLossMask(None)
    b = ln.bars(got, refs[1], refs[0])
    _record("masked_loss", H, W, name, b, unit=ln.unit((H, W, 3)), max_cot64=float(np.abs(refs[1]["cot"]).max()))
    assert np.isfinite(got["cot"]).all()
    assert (got["cot"][:, ln.ZERO_BAND[0]:ln.ZERO_BAND[1]] == 0).all() and (got["cot"][mask == 0] == 0).all()
    assert np.abs(refs[1]["cot"]).max() < ln.unit((H, W, 3)) or np.abs(got["cot"][mask != 0]).max() > 0     # (step_edge: the band hides the step)
    assert ln.misses(b) == [], b


# ------------------------------------------------------------------------------------------------------------ depth term
@pytest.mark.parametrize("H,W", [(32, 32), (33, 65)])
@pytest.mark.parametrize("kind", ["all_true", "all_false", "random"])
def test_depth_term_of_the_fused_loss(oracle32, oracle64, kind, H, W):
    """launch_loss with lambda_depth != 0 where depth_reduce_kernel's grid is nb = 3 and 18 blocks, not 512; an all-false mask is
    the 1e-6 guard of the denominator."""
    render, target = ln.reference(oracle32, oracle64, "blobs_near", H, W, images_only=True)
    rng = np.random.default_rng(H + W)
    rd, td = rng.uniform(1, 4, (H, W)).astype(np.float32), rng.uniform(1, 4, (H, W)).astype(np.float32)
    td[::3, ::4] = rd[::3, ::4]                                       # equal depths: sign(0) = 0
    mask = dict(all_true=np.ones((H, W), bool), all_false=np.zeros((H, W), bool), random=rng.uniform(size=(H, W)) > 0.5)[kind]
    lam_d = 0.3
    refs, cds = [], []
    for o in (oracle32, oracle64):
        dt = o.dtype
        loss, cot, cd, l1, ssim = o.loss_forward_backward(render.astype(dt), target.astype(dt), LAM, rd.astype(dt), td.astype(dt),
                                                          mask, lam_d)
        refs.append(dict(loss=loss, l1=l1, ssim=ssim, cot=np.asarray(cot, np.float64)))
        cds.append(np.asarray(cd, np.float64))
    r = _renderer(H, W)
    got, _, _, gd = _fused(r, _dev(render), _dev(target), renderDepth=_dev(rd), targetDepth=_dev(td),
                           depthMask=torch.as_tensor(mask), lambda_depth=lam_d)
    gd = _np(gd)
    b = ln.bars(got, refs[1], refs[0])
    rel = float(np.abs(gd - cds[1]).max() / (np.abs(cds[1]).max() + 1e-30))
    _record("depth_term", H, W, "blobs_near", b, mask=kind, depth_cot_rel=rel, depth_loss=float(got["depth"]))
    assert np.isfinite(gd).all() and (gd[~mask] == 0).all() and (gd[rd == td] == 0).all()
    if kind == "all_false":
        assert got["depth"] == 0.0 and (gd == 0).all()
    else:
        assert np.abs(gd).max() > 0 and got["depth"] > 0.5            # (the term is in the loss the bars hold: mean |U(1,4) - U(1,4)| ~ 1)
    assert rel <= ln.GRAD_RTOL, rel
    assert ln.misses(b) == [], b


# ------------------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("H,W", ln.SHAPES_SSIM_OP)
@pytest.mark.parametrize("name", list(ln.PAIRS))
def test_op_level_ssim_against_float64(oracle32, oracle64, name, H, W):
    a, b = ln.reference(oracle32, oracle64, name, H, W, images_only=True)
    up = ln.ssim_upstream(H, W)
    m32, m64 = ln.ssim_maps(oracle32, a, b), ln.ssim_maps(oracle64, a, b)
    g32, g64 = ln.ssim_gradients(oracle32, a, b, up), ln.ssim_gradients(oracle64, a, b, up)
    r = _renderer(H, W)
    maps = [_np(m) for m in r.ssim(_dev(a), _dev(b))]
    g = [_np(x) for x in r.ssimVJP(_dev(up))]
    measured = {k: ln.map_bar(maps[i], m64[i], m32[i], ln.ABS_FLOOR) for i, k in enumerate(ln.SSIM_MAPS)}
    for i, k in enumerate(("g1", "g2")):
        measured[k] = ln.map_bar(g[i], g64[i], g32[i], ln.GRAD_RTOL * float(np.abs(g64[i]).max()))
    _record("ssim_op", H, W, name, measured, max_g64=[float(np.abs(x).max()) for x in g64])
    assert all(np.isfinite(x).all() for x in maps + g)
    assert ln.misses(measured) == [], measured
