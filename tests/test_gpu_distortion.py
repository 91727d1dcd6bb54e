"""The depth distortion loss on the device (include/gsplat.h gs_blend_distortion / gs_render_distortion and their _backward,
gs_distortion_loss, gs_arm_distortion, GaussianTrainer(distortion=...)) against gaussiansplattingmlx_amd/distortion.py in float64
on the oracle's lists.

Bars, fixed before the first run on the card.  R is the range of the mapped depth m over the records that are in a list.
  forward   2e-4 R^2 absolute.  A stop that falls one entry later in float32 moves D by at most w (A R^2 + S) <= 1.25e-4 R^2,
            since the entry behind a stop weighs under 1e-4 (A <= 1, S <= R^2 / 4); the rest is rounding.  The float32 host
            statement's own distance is printed beside the device's.
  gradient  test_gpu_parity's gradient metric, max |a - b| / max |b| <= 1e-3, per column (mean, conic, opacity, depth) against
            the float64 VJP with a cotangent drawn in [-1, 1]: per-Gaussian sums over pixels accumulated with float atomics.
  Rows of occluded and off-screen Gaussians: exactly 0.  The colour columns and columns 11 .. 15: their bits as they were.
  Pixels whose list is empty: exactly 0, and no pixel of images pre-filled with NaN is left unwritten.  Two forwards: the same bits.
  Fused     renderBackward with a ZERO colour cotangent and the term armed: the six raw-parameter gradients against the oracle's
            projection backward applied to the float64 rows, 1e-3 in the gradient metric.
  ADC       the statistic of one backward against hypot(W/2 g_x, H/2 g_y) of the float64 oracle's colour rows plus the term's
            rows read back from the device: 1e-3 of the largest value.
  Loss      gs_distortion_loss against the float64 statement: 1e-6 relative (a double sum of float32 products) and the
            cotangent image to 2 ulps (two float32 operations).
  Trainer   the first step at `start`: the loss word and distortionTerm() within max(4 d32, 1e-6) relative of float64, d32 the
            float32 host statement's distance (the bar of the feature training test).  Bit-for-bit comparisons run on the
            one-block-per-splat scene of test_gpu_loss_mask's kind, where the blend backward's sums have one order.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import distortion as ds

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
GRAD_BAR = 1e-3
W, H = 160, 120
MAP_KW = {"ndc": dict(map="ndc", near=0.2, far=1000.0), "linear": dict(map="linear")}
SENTINEL = 3.25


def _load(name):
    spec = importlib.util.spec_from_file_location("_dsg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gcp = _load("test_gpu_contrib_prune")
cpu, traj, aacpu = gcp.cpu, gcp.traj, gcp.aacpu
_renderer, _dev, _np, _rel = gcp._renderer, gcp._dev, gcp._np, gcp._rel


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The renderers and images of this module are freed and their cached blocks released when it ends, so that the modules
    behind it allocate as they do without it."""
    yield
    import gc
    for cache in (_op_cache, _fused_cache, _block):
        cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _draw(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _range(lists, kw):
    """R: the range of m over the records that are in a list."""
    m = ds.map_depth(np.asarray(lists[0], np.float64)[:, 10], **kw)[0]
    seen = np.unique(np.asarray(lists[1]).astype(np.int64))
    return float(m[seen].max() - m[seen].min())


def _statement(lists, kw, seed, n_rows):
    """The float64 statement and, for the printout, the float32 one: D, totals, a cotangent in [-1, 1] and the rows."""
    Hc, Wc = lists[4], lists[3]
    D, totals = ds.tile_distortion(*lists, **kw)
    cot = _draw(seed, Hc, Wc)
    rows = ds.tile_distortion_vjp(*lists, cot, totals=totals, N=n_rows, **kw)
    D32, t32 = ds.tile_distortion(*lists, dtype=np.float32, **kw)
    rows32 = ds.tile_distortion_vjp(*lists, cot, dtype=np.float32, totals=t32, N=n_rows, **kw)
    return dict(D=D, totals=totals, cot=cot, rows=rows, D32=D32, rows32=rows32, R=_range(lists, kw))


def _check_forward(tag, got_D, got_totals, st):
    bar = 2e-4 * st["R"] ** 2
    assert not bool(got_D.isnan().any()) and not bool(got_totals.isnan().any())           # every pixel is written
    e = np.abs(_np(got_D).astype(np.float64) - st["D"]).max()
    e32 = np.abs(st["D32"].astype(np.float64) - st["D"]).max()
    print(f"{tag}: D err {e:.3e} (float32 statement {e32:.3e}, bar {bar:.3e}, R {st['R']:.4f}, max D {st['D'].max():.4e})")
    assert e <= bar and st["D"].max() > 0
    assert torch.equal(got_D, got_totals[..., 0] * got_totals[..., 2])
    assert np.abs(_np(got_totals[..., 0]).astype(np.float64) - st["totals"][..., 0]).max() <= 1e-4


def _check_rows(tag, got, st):
    got = _np(got).astype(np.float64)
    for col in ds.GRAD_COLUMNS:
        e, e32 = _rel(got[:, col], st["rows"][:, col]), _rel(st["rows32"][:, col], st["rows"][:, col])
        print(f"{tag} column {col}: rel {e:.3e} (float32 statement {e32:.3e}, bar {GRAD_BAR:.0e}, max {np.abs(st['rows'][:, col]).max():.3e})")
        assert e <= GRAD_BAR, col


def _fresh_rows(n):
    """Rows whose gradient columns are zero and whose other columns hold a sentinel."""
    rows = torch.full((n, 16), SENTINEL, device="cuda")
    rows[:, list(ds.GRAD_COLUMNS)] = 0.0
    return rows


def _others_untouched(rows):
    others = [c for c in range(16) if c not in ds.GRAD_COLUMNS]
    return bool((rows[:, others] == SENTINEL).all())


# --------------------------------------------------------------------------------------------------------- 1. op level
_op_cache = {}


def _op_case(name, mapname, oracle64):
    if (name, mapname) not in _op_cache:
        c, s, bn, _ = gcp._op_case(name, oracle64)
        lists = (s["packed"], bn.sortedIdx, bn.tileRanges, c["W"], c["H"], c["tile"][0], c["tile"][1])
        _op_cache[(name, mapname)] = (c, s, bn, lists, _statement(lists, MAP_KW[mapname], 11, c["N"]))
    return _op_cache[(name, mapname)]


def _bin(r, s, bn):
    info = r.buildGlobalTileSliceInfo((s["rectMin"], s["rectMax"]), s["radii"], s["depths"])
    if bn is not None:        # both sides sweep identical lists
        assert np.array_equal(_np(info["sortedGaussIdx"]).astype(np.uint32), bn.sortedIdx)
        assert np.array_equal(_np(info["tileRanges"]).astype(np.uint32), bn.tileRanges)


@pytest.mark.parametrize("mapname", list(MAP_KW))
@pytest.mark.parametrize("name", list(gcp.OP_CASES))
def test_op_level_matches_float64(oracle64, name, mapname):
    c, s, bn, lists, st = _op_case(name, mapname, oracle64)
    if name == "deep_lists":      # longer than one LDS chunk, and the pixels stop inside the list
        first_layer = int(np.where(s["packed"][:, 9] == np.float32(0.95))[0][0])
        pos = [int(np.where(bn.sortedIdx[a:b] == first_layer)[0][0]) for a, b in bn.tileRanges]
        assert min(pos) > 256 and bn.B > max(pos) + 256
    prm = MAP_KW[mapname]
    r = _renderer(c["W"], c["H"], c["tile"])
    _bin(r, s, bn)
    out, tot = _nan(c["H"], c["W"]), _nan(c["H"], c["W"], 3)
    D, T = r.blendDistortion(s["packed"], prm, out, tot)
    assert D is out and T is tot
    _check_forward(f"{name} {mapname}", D, T, st)
    _bin(r, s, None)
    D2, T2 = r.blendDistortion(s["packed"], prm)
    assert torch.equal(D, D2) and torch.equal(T, T2)                    # two runs: the same bits
    rows = _fresh_rows(c["N"])
    assert r.blendDistortionVJP(s["packed"], _cuda(st["cot"]), T, prm, rows) is rows
    _check_rows(f"{name} {mapname}", rows, st)
    assert _others_untouched(rows)                                      # the colour columns and 11 .. 15: their bits
    for what in ("occluded", "offscreen"):
        assert not st["rows"][s[what]].any()
        assert not bool(rows[torch.as_tensor(s[what], device="cuda")][:, list(ds.GRAD_COLUMNS)].any()), what
    assert float(rows[s["spanning"], 10].abs()) > 0
    first = rows.clone()
    r.blendDistortionVJP(s["packed"], _cuda(st["cot"]), T, prm, rows)   # once more into the same buffer: it accumulates
    for col in ds.GRAD_COLUMNS:
        assert _rel(_np(rows[:, col]), 2.0 * _np(first[:, col]).astype(np.float64)) <= GRAD_BAR, col
    assert _others_untouched(rows)
    fresh = r.blendDistortionVJP(s["packed"], _cuda(st["cot"]), T, prm)  # rows=None: zeros are allocated
    assert tuple(fresh.shape) == (c["N"], 16) and not bool(fresh[:, 6:9].any()) and not bool(fresh[:, 11:].any())


def test_pixels_outside_every_list_are_written_as_zeros(oracle64):
    """Only two splats keep a radius, both in the top left tile: every other tile of the 48 x 40 image (partial blocks at both
    edges) has an empty list.  A pixel with one entry has D = 0 too, exactly."""
    Wc, Hc, N = 48, 40, 300
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
    r = _renderer(Wc, Hc)
    _bin(r, s, bn)
    D, T = r.blendDistortion(s["packed"], MAP_KW["linear"], _nan(Hc, Wc), _nan(Hc, Wc, 3))
    got, tot = _np(D), _np(T)
    assert not np.isnan(got).any() and not np.isnan(tot).any()
    assert not got[empty].any() and not tot[empty].any()
    want = ds.tile_distortion(*lists, **MAP_KW["linear"])[0]
    R = _range(lists, MAP_KW["linear"])
    assert np.abs(got - want).max() <= 2e-4 * R * R and want.max() > 0
    # nothing to sweep at all: both images are zeros, no row is touched
    cot = _cuda(_draw(1, Hc, Wc))
    rows = r.blendDistortionVJP(s["packed"], torch.zeros(Hc, Wc, device="cuda"), T, MAP_KW["linear"], _fresh_rows(N))
    assert not bool(rows[:, list(ds.GRAD_COLUMNS)].any())               # a zero cotangent: exact zeros
    rows = r.blendDistortionVJP(s["packed"], cot, T, MAP_KW["linear"], _fresh_rows(N))
    untouched = torch.as_tensor(~np.isin(np.arange(N), [1, 4]), device="cuda")
    assert not bool(rows[untouched][:, list(ds.GRAD_COLUMNS)].any()) and bool(rows[1].any())


# ------------------------------------------------------------------------------------------------------------- 2. the loss
@pytest.mark.parametrize("Hc,Wc", [(40, 48), (363, 367)])        # one block of partials / more pixels than 512 x 256: strides
def test_loss_kernel_matches_float64(Hc, Wc):
    rng = np.random.default_rng([5, Hc, Wc])
    D = rng.uniform(0, 2, (Hc, Wc)).astype(np.float32)
    mask = rng.integers(0, 256, (Hc, Wc)).astype(np.uint8)
    mask[0, :7] = (0, 255, 1, 254, 0, 255, 128)
    r = _renderer(Wc, Hc)
    for m in (None, mask):
        want_L, want_cot = ds.loss_and_cotangent(D, 7.5, m)
        loss = torch.tensor([0.25, -1.0, -2.0, -3.0], device="cuda")
        cot = _nan(Hc, Wc)
        out = r.distortionLoss(_cuda(D), 7.5, None if m is None else torch.as_tensor(m, device="cuda"), loss, cot)
        assert out[0] is loss and out[1] is cot
        got = _np(loss).astype(np.float64)
        print(f"{Hc} x {Wc} mask {m is not None}: loss word {got[0]:.8f}, float64 {0.25 + want_L:.8f}")
        assert abs(got[0] - (0.25 + want_L)) <= 1e-6 * (0.25 + want_L) and tuple(got[1:]) == (-1.0, -2.0, -3.0)
        assert np.abs(_np(cot).astype(np.float64) - want_cot).max() <= 2 * np.spacing(np.float32(want_cot.max()))
        if m is not None:
            assert not bool(cot[torch.as_tensor(m == 0, device="cuda")].any())
        loss2, cot2 = r.distortionLoss(_cuda(D), 7.5, None if m is None else torch.as_tensor(m, device="cuda"),
                                       torch.tensor([0.25], device="cuda"))
        assert torch.equal(loss2[0], loss[0]) and torch.equal(cot2, cot)      # two calls: the same bits
    for bad in (dict(distort=torch.zeros(Hc, Wc)), dict(distort=torch.zeros(Hc, Wc + 1, device="cuda")),
                dict(mask=torch.zeros(Hc, Wc, device="cuda")), dict(loss=torch.zeros(0, device="cuda")),
                dict(cot=torch.zeros(Hc, Wc, 2, device="cuda"))):
        args = dict(distort=_cuda(D), weight=1.0, mask=None, loss=None, cot=None)
        args.update(bad)
        with pytest.raises(ValueError):
            r.distortionLoss(**args)
    d = _cuda(D)
    z = torch.zeros(1, device="cuda")
    import ctypes
    assert r.lib.gs_distortion_loss(r.ctx, ctypes.c_float(float("nan")), Hc * Wc, d.data_ptr(), None, z.data_ptr(), d.data_ptr()) == 1
    assert r.lib.gs_distortion_loss(r.ctx, ctypes.c_float(1.0), -1, d.data_ptr(), None, z.data_ptr(), d.data_ptr()) == 1
    assert r.lib.gs_distortion_loss(r.ctx, ctypes.c_float(1.0), Hc * Wc, None, None, z.data_ptr(), d.data_ptr()) == 1
    assert r.lib.gs_distortion_loss(r.ctx, ctypes.c_float(1.0), 0, d.data_ptr(), None, z.data_ptr(), d.data_ptr()) == 0
    assert float(z) == 0.0


# -------------------------------------------------------------------------------------------------------- 3. fused path
_fused_cache = {}
VARIANTS = {"plain": ((16, 16), "ndc"), "aa": ((16, 16), "ndc"), "block_lists": ((50, 38), "linear")}


class _RowsOracle:
    """An oracle whose blend backward returns the rows it is given: its render_backward is then the projection backward (and
    the activations') applied to them."""

    def __init__(self, o, rows):
        self._o, self._rows = o, rows

    def __getattr__(self, k):
        return getattr(self._o, k)

    def blend_backward(self, *a, **k):
        return np.ascontiguousarray(self._rows, self._o.dtype)

    def render_backward(self, *a, **k):
        return type(self._o).render_backward(self, *a, **k)


def _want_fused(oracle64, variant):
    if variant not in _fused_cache:
        tile, mapname = VARIANTS[variant]
        p, cams = gcp._scene()
        cam = cams[0].as_dict()
        o = aacpu.AAOracle(oracle64) if variant == "aa" else oracle64
        fw = o.render_forward(p, cam, W, H, tile[0], tile[1], 4)
        lists = (fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, W, H, tile[0], tile[1])
        st = _statement(lists, MAP_KW[mapname], 42, 3000)
        shim = _RowsOracle(oracle64, st["rows"])
        back = aacpu.AAOracle(shim) if variant == "aa" else shim
        z = np.zeros(W * H)
        st["grads"] = back.render_backward(p, cam, W, H, tile[0], tile[1], 4, fw, np.zeros((W * H, 3)), z, z)
        _fused_cache[variant] = (fw, lists, st)
    return _fused_cache[variant]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_matches_float64_and_the_armed_backward_reaches_the_parameters(oracle64, variant):
    tile, mapname = VARIANTS[variant]
    p, cams = gcp._scene()
    fw, lists, st = _want_fused(oracle64, variant)
    prm = MAP_KW[mapname]
    r = _renderer(W, H, tile, aa=variant == "aa")
    assert r.blockLists == (variant == "block_lists")
    r.renderChecked(_dev(p), cams[0], wantDepth=False)                 # (the term needs no depth image)
    D, T = r.renderDistortion(prm, _nan(H, W), _nan(H, W, 3))
    _check_forward("fused " + variant, D, T, st)
    rows = r.renderDistortionVJP(_cuda(st["cot"]), T, prm, _fresh_rows(3000))
    _check_rows("fused " + variant, rows, st)
    assert _others_untouched(rows)
    unseen = ~st["rows"].any(axis=1)
    assert unseen.sum() > 0 and not bool(rows[torch.as_tensor(unseen, device="cuda")][:, list(ds.GRAD_COLUMNS)].any())
    # armed, with a zero colour cotangent: the raw-parameter gradients are the projection backward of the rows
    cot = _cuda(st["cot"])
    r.armDistortion(cot, T, prm)
    g = r.renderBackward(torch.zeros(H, W, 3, device="cuda"))
    for k in KEYS:
        e = _rel(_np(g[k]), st["grads"][k])
        print(f"fused {variant} armed backward {k}: rel {e:.3e} (bar {GRAD_BAR:.0e}, max {np.abs(st['grads'][k]).max():.3e})")
        assert e <= GRAD_BAR, k
    assert np.abs(st["grads"]["xyz"]).max() > 0 and np.abs(st["grads"]["opacity"]).max() > 0
    assert not np.asarray(st["grads"]["features_dc"]).any() and not bool(g["features_dc"].any())


# -------------------------------------------------------------------------------------- 4. arming, on the one-block scene
BW, BH = 64, 48
_block = {}


def _block_scene():
    """300 Gaussians of scale 0.02, twenty-five per 16 x 16 block of the 64 x 48 image of one camera, each centred within 1 pixel
    of its block's centre at depth 3 .. 4 (test_gpu_loss_mask's construction): no splat reaches a second block -- the tests check
    the radii and the pair count -- so the blend backward's sums have one term per Gaussian and one order."""
    if "scene" not in _block:
        from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
        rng = np.random.default_rng(71)
        fx, fy = 0.9 * BW, 0.9 * BW * 1.02
        cam = Camera(BW, BH, fx, fy, look_at_c2w([2.2, -2.6, 1.7]))
        by, bx, _ = np.meshgrid(np.arange(BH // 16), np.arange(BW // 16), np.arange(25), indexing="ij")
        n = bx.size
        px = 8.5 + 16.0 * bx.reshape(-1) + rng.uniform(-1, 1, n)          # (a pixel's centre is at its index + 0.5)
        py = 8.5 + 16.0 * by.reshape(-1) + rng.uniform(-1, 1, n)
        z = rng.uniform(3.0, 4.0, n)
        pc = np.stack([(px - BW / 2) * z / fx, (py - BH / 2) * z / fy, z, np.ones(n)], 1)
        p = dict(xyz=(pc @ cam.c2w.T)[:, :3], features_dc=rng.normal(0, 1, (n, 1, 3)), features_rest=rng.normal(0, 0.004, (n, 24, 3)),
                 scales=np.full((n, 3), np.log(0.02)), rotation=rng.normal(0, 1, (n, 4)), opacity=rng.normal(0.3, 1.5, n))
        p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
        r = _renderer(BW, BH)
        res = r.renderForward(_dev(p), cam, want_radii=True)
        r.sync()
        assert int((res.radii > 0).sum()) == n and float(res.radii.max()) <= 6 and r.stats()["M"] <= n
        from gaussiansplattingmlx_amd.scenes import perturb
        target = r.renderForward(_dev(perturb(p, 5, 0.1)), cam).render.reshape(BH, BW, 3).clone()
        r.close()
        _block["scene"] = (p, cam, target)
    return _block["scene"]


def _grads(r, params, cam, target, between=None):
    res = r.renderChecked(params, cam, wantDepth=False)
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    cot = cot.clone()
    if between is not None:
        between()
    return {k: v.clone() for k, v in r.renderBackward(cot).items()}


def test_arming_and_disarming():
    import ctypes
    p, cam, target = _block_scene()
    params = _dev(p)
    r = _renderer(BW, BH)
    g0 = _grads(r, params, cam, target)
    again = _grads(r, params, cam, target)
    assert all(torch.equal(g0[k], again[k]) for k in KEYS)               # (the scene is built for it)
    held = {}

    def distortion_pass(arm, then=None):
        def body():
            D, T = r.renderDistortion(MAP_KW["linear"])
            _, c = r.distortionLoss(D, 5.0)
            held.update(D=D, T=T, c=c)
            if arm:
                r.armDistortion(c, T, MAP_KW["linear"])
            if then is not None:
                then()
        return body
    # a pass that is not armed changes nothing: the same bits
    g1 = _grads(r, params, cam, target, distortion_pass(False))
    assert all(torch.equal(g0[k], g1[k]) for k in KEYS) and float(held["D"].max()) > 0
    # armed: another step
    g2 = _grads(r, params, cam, target, distortion_pass(True))
    assert not torch.equal(g2["xyz"], g0["xyz"]) and not torch.equal(g2["opacity"], g0["opacity"])
    assert torch.equal(g2["features_dc"], g0["features_dc"])            # (the term has no colour gradient)
    # armed and disarmed again: today's bits
    g3 = _grads(r, params, cam, target, distortion_pass(True, lambda: r.armDistortion(None)))
    assert all(torch.equal(g0[k], g3[k]) for k in KEYS)
    # a new forward disarms
    r.renderChecked(params, cam, wantDepth=False)
    distortion_pass(True)()
    g4 = _grads(r, params, cam, target)
    assert all(torch.equal(g0[k], g4[k]) for k in KEYS)
    # the data-parallel backwards refuse an armed context, with the reason
    res = r.renderChecked(params, cam, wantDepth=False)
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    distortion_pass(True)()
    n = p["xyz"].shape[0]
    cc = torch.zeros(3 * n + 16, device="cuda")
    gg = [torch.zeros(n, k, device="cuda") for k in (3, 3, 4, 1)]
    assert r.lib.gs_render_backward_dp_begin(r.ctx, cot.data_ptr(), None, None, cc.data_ptr()) == 1
    reason = r.lib.gs_last_error(r.ctx).decode()
    assert "gs_render_backward_dp_begin" in reason and "distortion term is armed" in reason
    own = torch.zeros(n, 3, device="cuda")
    assert r.lib.gs_render_backward_dp_geom(r.ctx, cot.data_ptr(), None, None, cc.data_ptr(), *[t.data_ptr() for t in gg],
                                            own.data_ptr()) == 1
    assert "distortion term is armed" in r.lib.gs_last_error(r.ctx).decode()
    assert not bool(cc.any()) and not any(bool(t.any()) for t in gg)
    r.armDistortion(None)
    assert r.lib.gs_render_backward_dp_begin(r.ctx, cot.data_ptr(), None, None, cc.data_ptr()) == 0


def test_refusals(oracle64):
    import ctypes
    from gaussiansplattingmlx_amd import _lib
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cam, target = _block_scene()
    n = p["xyz"].shape[0]
    r = _renderer(BW, BH)
    D, T, c = torch.zeros(BH, BW, device="cuda"), torch.zeros(BH, BW, 3, device="cuda"), torch.zeros(BH, BW, device="cuda")
    rows = torch.zeros(n, 16, device="cuda")
    prm = _lib.gs_distortion_params(1, 0.0, 0.0)
    ref = ctypes.byref(prm)
    f, fo = torch.zeros(n, 4, device="cuda"), torch.zeros(BH, BW, 4, device="cuda")
    # no forward: gs_render_features' code
    want = r.lib.gs_render_features(r.ctx, 4, f.data_ptr(), fo.data_ptr())
    assert want == 5                                                                       # GS_ERR_NO_FORWARD
    assert r.lib.gs_render_distortion(r.ctx, ref, D.data_ptr(), T.data_ptr()) == want
    assert r.lib.gs_render_distortion_backward(r.ctx, ref, c.data_ptr(), T.data_ptr(), rows.data_ptr()) == want
    assert r.lib.gs_arm_distortion(r.ctx, ref, c.data_ptr(), T.data_ptr()) == want
    assert r.lib.gs_arm_distortion(r.ctx, None, None, None) == 0                           # disarming needs no forward
    for call in (lambda: r.renderDistortion(), lambda: r.renderDistortionVJP(c, T)):
        with pytest.raises(GsplatError) as e:
            call()
        assert e.value.code == 5
    model = GaussModel(p, r.device)
    res = r.renderChecked(model.getParams(), cam, wantDepth=False)
    # arguments
    assert r.lib.gs_render_distortion(r.ctx, None, D.data_ptr(), T.data_ptr()) == 1        # GS_ERR_INVALID_ARG
    assert r.lib.gs_render_distortion(r.ctx, ref, None, T.data_ptr()) == 1
    assert r.lib.gs_render_distortion(r.ctx, ref, D.data_ptr(), None) == 1
    assert r.lib.gs_render_distortion_backward(r.ctx, ref, None, T.data_ptr(), rows.data_ptr()) == 1
    assert r.lib.gs_render_distortion_backward(r.ctx, ref, c.data_ptr(), T.data_ptr(), None) == 1
    assert r.lib.gs_arm_distortion(r.ctx, ref, c.data_ptr(), None) == 1
    for bad in (_lib.gs_distortion_params(2, 0.2, 1000.0), _lib.gs_distortion_params(0, 0.0, 1000.0),
                _lib.gs_distortion_params(0, 5.0, 5.0), _lib.gs_distortion_params(0, 0.2, float("inf")),
                _lib.gs_distortion_params(-1, 0.2, 1000.0)):
        assert r.lib.gs_render_distortion(r.ctx, ctypes.byref(bad), D.data_ptr(), T.data_ptr()) == 1
        assert r.lib.gs_arm_distortion(r.ctx, ctypes.byref(bad), c.data_ptr(), T.data_ptr()) == 1
    for call in (lambda: r.renderDistortion(dict(map="log")), lambda: r.renderDistortion(None, torch.zeros(BH, BW)),
                 lambda: r.renderDistortion(None, D, torch.zeros(BH, BW, 2, device="cuda")),
                 lambda: r.renderDistortionVJP(c, T, None, torch.zeros(n, 11, device="cuda")),
                 lambda: r.renderDistortionVJP(torch.zeros(BH, BW + 1, device="cuda"), T),
                 lambda: r.armDistortion(c, None), lambda: r.armDistortion(c, torch.zeros(BH, BW, device="cuda"))):
        with pytest.raises(ValueError):
            call()
    # a consumed forward: gs_render_features' code again
    _, cot, _ = r.lossForwardBackward(res.render, target, 0.2)
    r.renderDistortion(prm, D, T)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, getLearningRates(0, 1000))
    want = r.lib.gs_render_features(r.ctx, 4, f.data_ptr(), fo.data_ptr())
    assert want == 5
    assert r.lib.gs_render_distortion(r.ctx, ref, D.data_ptr(), T.data_ptr()) == want
    assert r.lib.gs_render_distortion_backward(r.ctx, ref, c.data_ptr(), T.data_ptr(), rows.data_ptr()) == want
    assert r.lib.gs_arm_distortion(r.ctx, ref, c.data_ptr(), T.data_ptr()) == want
    # the op-level pair: a binning first, the binned N, no null buffer
    cc, s, bn, _ = gcp._op_case("partial_blocks", oracle64)
    r2 = _renderer(cc["W"], cc["H"], cc["tile"])
    packed = r2._t(s["packed"])
    D2, T2 = torch.zeros(cc["H"], cc["W"], device="cuda"), torch.zeros(cc["H"], cc["W"], 3, device="cuda")
    rows2 = torch.zeros(cc["N"], 16, device="cuda")
    assert r2.lib.gs_blend_distortion(r2.ctx, cc["N"], packed.data_ptr(), ref, D2.data_ptr(), T2.data_ptr()) == 5
    _bin(r2, s, bn)
    assert r2.lib.gs_blend_distortion(r2.ctx, cc["N"] - 1, packed.data_ptr(), ref, D2.data_ptr(), T2.data_ptr()) == 2
    assert r2.lib.gs_blend_distortion(r2.ctx, cc["N"], packed.data_ptr(), None, D2.data_ptr(), T2.data_ptr()) == 1
    assert r2.lib.gs_blend_distortion(r2.ctx, cc["N"], packed.data_ptr(), ref, None, T2.data_ptr()) == 1
    assert r2.lib.gs_blend_distortion_backward(r2.ctx, cc["N"], packed.data_ptr(), ref, D2.data_ptr(), T2.data_ptr(), None) == 1
    assert r2.lib.gs_blend_distortion_backward(r2.ctx, cc["N"], packed.data_ptr(), ref, None, T2.data_ptr(), rows2.data_ptr()) == 1
    assert not bool(rows2.any())


# ----------------------------------------------------------------------------------------------------------------- 5. ADC
def test_adc_statistic_includes_the_term(oracle64):
    p, cams = gcp._scene()
    fw, lists, st = _want_fused(oracle64, "plain")
    prm = MAP_KW["ndc"]
    bn = fw["bin"]
    cotc = (np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)).astype(np.float32)
    z = np.zeros(W * H)
    gp = oracle64.blend_backward(fw["packed"], bn.sortedIdx, bn.tileRanges, W, H, 16, 16, False,
                                 cotc.astype(np.float64).reshape(-1, 3), z, z, fw["color"], fw["depth"], fw["alpha"], fw["last"])
    r = _renderer(W, H)
    acc = torch.zeros(3, 3000, device="cuda")
    r.setADCStats(acc[0], acc[1], acc[2])
    res = r.renderChecked(_dev(p), cams[0], want_radii=True, wantDepth=False)
    vis = _np(res.radii) > 0
    D, T = r.renderDistortion(prm)
    # the term's rows, read back; the cotangent is scaled so that the term weighs on the means as the colour does
    unit = _np(r.renderDistortionVJP(_cuda(st["cot"]), T, prm)).astype(np.float64)
    scale = np.abs(gp[:, 0:2]).max() / np.abs(unit[:, 0:2]).max()
    cot = _cuda(st["cot"] * np.float32(scale))
    rows = _np(r.renderDistortionVJP(cot, T, prm)).astype(np.float64)
    r.armDistortion(cot, T, prm)
    r.renderBackward(_cuda(cotc))
    r.setADCStats(None)
    got = _np(acc)
    gx, gy = gp[:, 0] + rows[:, 0], gp[:, 1] + rows[:, 1]
    want = np.where(vis, np.hypot(0.5 * W * gx, 0.5 * H * gy), 0.0)
    colour_only = np.where(vis, np.hypot(0.5 * W * gp[:, 0], 0.5 * H * gp[:, 1]), 0.0)
    err = np.abs(got[0] - want).max() / want.max()
    apart = np.abs(colour_only - want).max() / want.max()
    print(f"gradSum with the term armed against hypot(W/2 g_x, H/2 g_y) including it: {err:.3e} of the largest (bar {GRAD_BAR:.0e}); "
          f"the colour rows alone are {apart:.3e} away")
    assert err <= GRAD_BAR and apart > 100 * GRAD_BAR
    assert np.array_equal(got[1], vis.astype(np.float32))
    r.close()


# ------------------------------------------------------------------------------------------------------------- 6. trainer
def _trainer(r, p, **kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    model = GaussModel(p, r.device)
    kw.setdefault("densify", False)
    return GaussianTrainer(model, r, iterationCount=1000, **kw), model


def _same(a, b):
    return torch.equal(a.arena, b.arena) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


@pytest.mark.parametrize("fuse", [True, False])
def test_none_and_before_start_are_todays_step(fuse):
    p, cam, target = _block_scene()
    base_tr, base = _trainer(_renderer(BW, BH), p, fuse_adam=fuse)
    base_losses = [base_tr.trainStep(cam, target, viewKey=0).clone() for _ in range(3)]
    assert bool(base.m.any())
    for kw in (dict(distortion=None), dict(distortion=ds.DistortionConfig(weight=10.0, start=3, map="linear"))):
        r = _renderer(BW, BH)
        tr, model = _trainer(r, p, fuse_adam=fuse, **kw)
        losses = [tr.trainStep(cam, target, viewKey=0).clone() for _ in range(3)]
        assert all(torch.equal(a, b) for a, b in zip(losses, base_losses))
        assert _same(model, base)
        assert tr.distortionTerm() is None and tr._distortionBufs is None and r._distortion_armed is None      # no buffer, no setter call
        if kw["distortion"] is not None:
            tr.trainStep(cam, target, viewKey=0)                       # iteration 3 = start: the term runs
            assert float(tr.distortionTerm()) > 0 and r._distortion_armed is not None


@pytest.mark.parametrize("fuse", [True, False])
def test_first_step_at_start_against_float64(oracle32, oracle64, fuse):
    p, cam, target = _block_scene()
    cfg = ds.DistortionConfig(weight=10.0, start=1, map="linear")
    r = _renderer(BW, BH)
    tr, model = _trainer(r, p, fuse_adam=fuse, distortion=cfg)
    plain_tr, plain = _trainer(_renderer(BW, BH), p, fuse_adam=fuse)
    tr.trainStep(cam, target, viewKey=0)
    plain_tr.trainStep(cam, target, viewKey=0)
    assert _same(model, plain) and tr.distortionTerm() is None
    now = {k: _np(v).copy() for k, v in model.getParams().items()}      # what the step at `start` renders
    loss = _np(tr.trainStep(cam, target, viewKey=0)).astype(np.float64)
    plain_loss = _np(plain_tr.trainStep(cam, target, viewKey=0)).astype(np.float64)
    term = float(tr.distortionTerm())
    tgt = _np(target)
    host = {}
    for name, o in (("f64", oracle64), ("f32", oracle32)):
        fw = o.render_forward(now, cam.as_dict(), BW, BH, 16, 16, 4)
        colour = o.loss_forward_backward(fw["color"].reshape(BH, BW, 3), tgt, 0.2)[0]
        D = ds.tile_distortion(fw["packed"], fw["bin"].sortedIdx, fw["bin"].tileRanges, BW, BH, 16, 16, map="linear", dtype=o.dtype)[0]
        mean = float(D.astype(np.float64).mean()) if name == "f64" else float(D.mean(dtype=np.float32))
        host[name] = (float(colour) + 10.0 * mean, mean, float(colour))
    d32_loss = abs(host["f32"][0] - host["f64"][0]) / host["f64"][0]
    d32_term = abs(host["f32"][1] - host["f64"][1]) / host["f64"][1]
    e_loss, e_term = abs(loss[0] - host["f64"][0]) / host["f64"][0], abs(term - host["f64"][1]) / host["f64"][1]
    print(f"fuse={fuse}: loss word {loss[0]:.8f} float64 {host['f64'][0]:.8f} (colour {host['f64'][2]:.8f}) distance {e_loss:.3e} "
          f"d32 {d32_loss:.3e}; mean D {term:.8e} float64 {host['f64'][1]:.8e} distance {e_term:.3e} d32 {d32_term:.3e}")
    assert 10.0 * host["f64"][1] > 0.01 * host["f64"][2]               # the term is a visible part of the word
    assert e_loss <= max(4 * d32_loss, 1e-6)
    assert e_term <= max(4 * d32_term, 1e-6)
    assert abs((loss[0] - plain_loss[0]) - 10.0 * term) <= 1e-6 * loss[0]      # colour loss + weight mean D, on the device's own numbers
    assert not _same(model, plain)                                      # the term moved the step


@pytest.mark.parametrize("fuse", [True, False])
def test_a_fully_masked_step_gets_nothing_from_the_term(fuse):
    p, cam, target = _block_scene()
    mask = torch.zeros(BH, BW, dtype=torch.uint8, device="cuda")
    out = []
    for kw in ({}, dict(distortion=ds.DistortionConfig(weight=10.0, start=0, map="linear"))):
        r = _renderer(BW, BH)
        tr, model = _trainer(r, p, fuse_adam=fuse, **kw)
        model.m.fill_(1e-4)                                            # (moments that move the parameters whatever the gradient)
        model.v.fill_(1e-8)
        before = model.arena.clone()
        loss = tr.trainStep(cam, target, viewKey=0, lossMask=mask).clone()
        assert not torch.equal(model.arena, before)
        out.append((loss, model, tr))
    assert float(out[1][2].distortionTerm()) > 0                       # the term ran, and saw D
    assert torch.equal(out[0][0], out[1][0])                            # ... weighted by v = 0 everywhere
    assert _same(out[0][1], out[1][1])


def test_a_masked_step_weighs_the_term_by_the_mask():
    """Half the image masked out: the loss word gains weight mean(v D), v the mask's weights, against the device's own D."""
    p, cam, target = _block_scene()
    mask = torch.full((BH, BW), 255, dtype=torch.uint8, device="cuda")
    mask[:, BW // 2:] = 0
    mask[:3] = 51
    words = []
    for kw in ({}, dict(distortion=ds.DistortionConfig(weight=10.0, start=0, map="linear"))):
        tr, model = _trainer(_renderer(BW, BH), p, **kw)
        words.append((float(tr.trainStep(cam, target, viewKey=0, lossMask=mask)[0]), tr))
    D = _np(words[1][1]._distortionBufs[0]).astype(np.float64)
    want = ds.loss_and_cotangent(D, 10.0, _np(mask))[0]
    print(f"masked step: loss word gains {words[1][0] - words[0][0]:.8f}, weight mean(v D) = {want:.8f}")
    assert want > 1e-3 and abs((words[1][0] - words[0][0]) - want) <= 1e-6 * words[1][0]
