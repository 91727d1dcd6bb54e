"""The fused Adam step, element by element against a float64 Adam: gs_render_backward_adam's seven ways
of walking a wave's features_rest span (csrc/projection.hip: adam_rows with its scalar head and tail, adam_rows<SPARSE>,
adam_rows_kept and its SPARSE form, adam_band_rows_kept, adam_band_rows, the 14 small per-lane elements) and the stand-alone
kernels of csrc/optim.hip (gs_adam_step past its grid-stride seam, gs_adam_step_visible, gs_adam_step_add).

What makes an element-wise bar possible: on an image of at most two 16 x 16 blocks every gradAcc16 entry takes at most two
atomic addends, and 0 + a + b = 0 + b + a exactly (test_gpu_parity.test_backward_wave_count_leaves_the_same_bits), so the unfused
gradient g of gs_render_backward is the same bits on every run (section 1 holds each scene to that).  projection.hip is built
without contraction, so the fused step of the same forward is Adam of that g: every element of the six tensors is held to
tests/fused_adam_numpy.py's bars -- rounding alone, no share, no tolerance relative to a tensor's maximum --, and every other
element of the three arenas (pads, rows from N to the stride, a hand-laid arena's gaps, invisible rows under sparse Adam,
inactive columns under a lower SH degree) to its bits, having been filled with random values (the inactive moments with NaN).

Arenas: GaussModel's packed and capacity-strided layouts (every tensor on a 16-byte boundary), and fused_adam_numpy.hand_arena,
whose features_rest starts 1, 2 or 3 floats off one.  The library serves such a tensor at every K: neither gs_render_forward nor
gs_render_backward_adam asks for an alignment, the staging loads are dword-aligned 16-byte global accesses there, and the
backward's `kept` test sends the span to adam_rows (head, body, tail) or adam_band_rows instead of the kept registers.

Each test prints, per tensor and arena, the largest ratio error / bar and its element, and the module keeps them all in
fused_adam_elementwise.json where GSPLAT_TEST_REPORTS names a directory (tests/test_gpu_dp_kernels.py's convention).

Measured (MI355X), the largest error / bar over every case of a form, for p / m / v (no element of any case beyond 1, and
no bar carries a margin for a gradient that differs between the unfused and the fused kernel: none was needed):
  dense, GaussModel arena (kept, adam_rows with a tail, the small elements)    0.994 / 0.486 / 0.391
  dense, hand arena (adam_rows: head, body, tail; K = 25 leaves the kept form)  0.996 / 0.485 / 0.395
  sparse, GaussModel arena (adam_rows<SPARSE>, adam_rows_kept<SPARSE>)         0.987 / 0.481 / 0.385
  sparse, hand arena at offset 2                                               0.981 / 0.485 / 0.380
  banded, GaussModel arena (adam_band_rows_kept, adam_band_rows at K = 16)     0.997 / 0.483 / 0.389
  banded, hand arena at offset 1 (adam_band_rows at K = 25)                    0.987 / 0.485 / 0.382
  gs_adam_step, n = 8 392 707                                                  0.999 / 0.467 / 0.396
  gs_adam_step_visible, n = 8 392 707                                          0.997 / 0.463 / 0.396
  gs_adam_step_add, n = 10 007                                                 0.976 / 0.335 / 0.378
The parameter ratio sits near 1 because the bar is 8u of the step where the derivation allows 7u (3.5 x 2^-23): measured where
p0 = 0, the step lies 2.88 x 2^-23 of its size from the float64 step (the IEEE float32 step: 1.68).  Subnormal second moments
were kept (v0 = 0, |g| = 1e-20 gives v = 1e-43, not 0); no scene stored a subnormal v.
Teeth (experiment builds of projection.hip, not committed): adam_rows without its tail fails the 26 cases whose span has one and no
other; without its head, the 13 hand-arena cases of the dense and sparse steps; a straddling float4 stored back as it came, the
six banded cases with one (K = 25 at degree 1 and 3, K = 9 at degree 1); lr[1] for features_rest, every case with K > 1 whose
degree moves a features_rest element (60).
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gaussiansplattingmlx_amd import sparse_adam as sa  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GRAD_RTOL = 1e-3


def _load(name):
    spec = importlib.util.spec_from_file_location("_fae_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fan = _load("fused_adam_numpy")
KEYS = fan.KEYS
REPORT = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")


def _renderer(K, W, H):
    _need_gpu()
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(fan.DEGREE[K], W, H, (16, 16), False)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _write_report():
    """Every ratio recorded so far, as a file where GSPLAT_TEST_REPORTS names a directory (never fails a test)."""
    out = os.environ.get("GSPLAT_TEST_REPORTS")
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, "fused_adam_elementwise.json"), "w") as f:
                json.dump(REPORT, f, indent=1, sort_keys=True)
        except OSError:
            pass


def _size(N, inv=None):
    """The image of a case: both sizes of fused_adam_numpy.SIZES are used across the cases."""
    return fan.SIZES[1] if (N in (63, 129, 65) or inv == "blocked") else fan.SIZES[0]


# ------------------------------------------------------------------------------------------------------------------ the arenas
class _Arena:
    """Three flat device buffers of one layout and the six parameter tensors as views of the first."""

    def __init__(self, arena, m, v, starts, N, K, model=None):
        self.arena, self.m, self.v, self.starts, self.N, self.K, self.model = arena, m, v, starts, N, K, model
        self.numel = int(arena.numel())
        self.ids = fan.tensor_ids(self.numel, starts, N, K)
        self.rows = fan.element_rows(self.ids, starts, N, K)
        self.cols = fan.rest_columns(self.ids, starts, N, K)
        self.params = fan.carve(arena, starts, N, K)

    def state(self):
        return {name: _np(getattr(self, name)).copy() for name in ("arena", "m", "v")}


def _model_arena(p, device, capacity=None):
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER, GaussModel
    model = GaussModel(p, device)
    if capacity is not None:
        model.restride(capacity)
        assert model.stride == capacity
    N, K = model.N, model.K
    A = _Arena(model.arena, model.m, model.v, dict(zip(ARENA_ORDER, (int(s) for s in model.seg_start))), N, K, model)
    on = sa.element_mask(np.ones(N, bool), model.seg_end, sa.model_row_floats(model), N)
    assert np.array_equal(on, A.ids >= 0)                      # the library's own map of the layout says the same
    for k in KEYS:
        assert not A.params[k].numel() or A.params[k].data_ptr() == model.getParams()[k].data_ptr(), k
    # the pads (and the rows from N to the stride): random in the parameter arena too; the moments are filled per step
    off = torch.as_tensor(~on, device=device)
    model.arena[off] = torch.randn(int((~on).sum()), device=device)
    return A


def _hand_arena(p, N, K, res):
    h = fan.hand_arena(p, N, K, res)
    A = _Arena(_dev(h["arena"]), _dev(h["m"]), _dev(h["v"]), h["starts"], N, K)
    assert np.array_equal(A.ids >= 0, h["mask"]) and A.arena.data_ptr() % 16 == 0
    assert (A.params["features_rest"].data_ptr() - A.arena.data_ptr()) // 4 % 4 == res
    return A


def _make_arena(p, N, K, layout, device):
    if layout == "packed":
        return _model_arena(p, device)
    if layout.startswith("stride"):
        return _model_arena(p, device, int(layout[6:]))
    assert layout.startswith("hand")
    return _hand_arena(p, N, K, int(layout[4:]))


# ----------------------------------------------------------------------------------------------------------------- the judging
def _describe(A, e, lact=None):
    i = int(A.ids[e])
    if i < 0:
        return f"arena element {e} (of no tensor)"
    k = KEYS[i]
    s = f"{k}[{int(A.rows[e])}, {e - A.starts[k] - int(A.rows[e]) * fan.row_floats(A.K)[k]}] (arena element {e})"
    if k == "features_rest" and lact is not None and 0 < lact < 3 * (A.K - 1) and lact % 4:
        c = int(A.cols[e])
        if c // 4 == lact // 4:
            s += f" -- in the float4 that straddles the last active column, columns {4 * (lact // 4)} to {4 * (lact // 4) + 3}"
    return s


def _implied_gradient(A, before, after, g_flat, on, scale):
    """The gradient the stored m implies, (m - b1 m0) / ((1 - b1) scale), against g in ulps of g: per row of features_rest the
    smallest and the largest distance (a gradient that differs between the unfused and the fused kernel shows here)."""
    b1 = np.float32(0.9)
    c1 = float(np.float32(1) - b1)
    sel = on & (A.ids == 2) & (g_flat != 0)
    if not sel.any():
        return "no features_rest element with a gradient"
    imp = (after["m"][sel].astype(np.float64) - float(b1) * before["m"][sel].astype(np.float64)) / (c1 * float(np.float32(scale)))
    ulp = np.spacing(np.abs(g_flat[sel])).astype(np.float64)
    dist = np.abs(imp - g_flat[sel].astype(np.float64)) / ulp
    rows = A.rows[sel]
    worst = int(rows[np.argmax(dist)])
    r = dist[rows == worst]
    return f"implied gradient against g: largest distance {dist.max():.3g} ulp (row {worst}: {r.min():.3g} .. {r.max():.3g} over its columns)"


def _judge(tag, A, before, after, g_flat, on, lrs, scale=1.0, lact=None):
    """Every element of `on` against the bars, every other element against its bits; prints and records the worst ratios."""
    off = ~on
    for name in ("arena", "m", "v"):
        same = fan.bits(after[name]) == fan.bits(before[name])
        bad = np.flatnonzero(off & ~same)
        assert bad.size == 0, (f"{tag}: {bad.size} elements of {name} that the step must leave alone changed bits, the first "
                               f"{_describe(A, int(bad[0]), lact)}: {before[name][bad[0]]!r} -> {after[name][bad[0]]!r}")
    lr_el = np.zeros(A.numel, np.float32)
    lr_el[A.ids >= 0] = np.asarray(lrs, np.float32)[A.ids[A.ids >= 0]]
    idx = np.flatnonzero(on)
    b = fan.bars(before["arena"][idx], before["m"][idx], before["v"][idx], g_flat[idx], after["arena"][idx], after["m"][idx],
                 after["v"][idx], lr_el[idx], scale=scale, **fan.ADAM)
    rec = REPORT.setdefault(tag, {})
    fails = []
    for i, k in enumerate(KEYS):
        sel = A.ids[idx] == i
        if not sel.any():
            continue
        for name, rk in (("p", "ratio_p"), ("m", "ratio_m"), ("v", "ratio_v")):
            r = b[rk][sel]
            j = int(np.argmax(r))
            e = int(idx[sel][j])
            rec[f"{k}.{name}"] = dict(ratio=float(r[j]), element=_describe(A, e, lact), beyond=int((r > 1).sum()), of=int(sel.sum()))
            print(f"{tag} {k}.{name}: largest error / bar {r[j]:.3f} at {_describe(A, e, lact)}; {int((r > 1).sum())} of {int(sel.sum())} beyond")
            if r[j] > 1:
                fails.append(f"{k}.{name}: {int((r > 1).sum())} of {int(sel.sum())} elements beyond the bar, the worst {r[j]:.3g} x at "
                             f"{_describe(A, e, lact)}")
    sub = (after["v"][idx] > 0) & (after["v"][idx] < fan.TINY)
    rec["subnormal_v_stored"] = int(sub.sum())
    _write_report()
    if fails:
        fails.append(_implied_gradient(A, before, after, g_flat, on, scale))
    assert not fails, f"{tag}: " + "; ".join(fails)
    return b


def _gradient(r, A, cot):
    """The unfused gradient of the last forward as a flat buffer of the arena's layout -- taken under both wave counts: the
    same bits, or the bars below have no ground to stand on."""
    out = []
    for waves in (1, 16):
        r.setTuning(bwd_waves_per_cu=waves)
        g = r.renderBackward(cot)
        out.append({k: _np(g[k]).copy() for k in KEYS})
    for k in KEYS:
        assert np.array_equal(fan.bits(out[0][k]), fan.bits(out[1][k])), k
    return fan.scatter(out[0], A.numel, A.starts, A.N, A.K)


def _set(buf, sel, values):
    buf[torch.as_tensor(sel, device=buf.device)] = _dev(np.asarray(values, np.float32))


def _steps(tag, r, A, cams, cot, on, lact=None, grad_scale=1.0, seed=1):
    """Two fused steps, each judged: camera A from random moments, camera B from the state the first step left."""
    from gaussiansplattingmlx_amd.trainer import getLearningRates
    lrs = getLearningRates(0, 1000)
    rng = np.random.default_rng(seed)
    for step, cam in enumerate(cams):
        r.renderForward(A.params, cam, wantDepth=False)
        g_flat = _gradient(r, A, cot)
        assert not g_flat[~on].any()                    # what the step must leave alone has no gradient to begin with
        if step == 0:
            m0, v0 = fan.start_moments(g_flat, A.ids, seed)
            A.m.copy_(_dev(m0))
            A.v.copy_(_dev(v0))
            if lact is not None:                        # the inactive columns' moments: NaN, so that a stray load shows
                inactive = (A.ids == 2) & (A.cols >= lact)
                _set(A.m, inactive, np.full(int(inactive.sum()), np.nan))
                _set(A.v, inactive, np.full(int(inactive.sum()), np.nan))
        else:                                           # fresh values where nothing may be written, for the second step too
            for buf in (A.arena, A.m, A.v):
                _set(buf, A.ids < 0, rng.normal(0, 1, int((A.ids < 0).sum())))
        before = A.state()
        r.renderBackwardAdam(cot, A.arena, A.m, A.v, lrs, grad_scale=grad_scale)
        after = A.state()
        assert np.isfinite(after["arena"][A.ids >= 0]).all()
        moved = fan.bits(after["arena"][on]) != fan.bits(before["arena"][on])
        assert moved.mean() > 0.9, (tag, step, float(moved.mean()))
        _judge(f"{tag} step {step}", A, before, after, g_flat, on, lrs, grad_scale, lact)


# ------------------------------------------------------------------------------------------------------------ 2. the case lists
NS = (1, 63, 64, 65, 129, 321)
DENSE = [(K, N, "packed", 1.0) for K in (1, 4, 9, 16, 25) for N in NS]
DENSE += [(K, 321, "stride512", 1.0) for K in (25, 16)]
DENSE += [(K, N, f"hand{res}", 1.0) for K in (25, 16) for N in (65, 321) for res in (1, 2, 3)]
DENSE += [(25, 129, "packed", 0.5)]
SPARSE = [(K, 321, inv, "packed") for K in (25, 16, 4, 1) for inv in ("scattered", "blocked")] + [(16, 321, "scattered", "hand2")]
BANDS = [(K, d, N, "packed") for K, ds in ((25, (0, 1, 2, 3)), (16, (0, 1, 2)), (9, (1,))) for d in ds for N in (65, 321)]
BANDS += [(25, d, 321, "hand1") for d in (1, 3)]
SCENES = sorted({(*_size(N), N, K, "") for K, N, _, _ in DENSE} | {(*_size(N, inv), N, K, inv) for K, N, inv, _ in SPARSE}
                | {(*_size(N), N, K, "") for K, _, N, _ in BANDS})
SEED = 7


# ------------------------------------------------------------------------------------------------------------ 1. the precondition
@pytest.mark.parametrize("W,H,N,K,inv", SCENES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-' + c[4] if c[4] else ''}" for c in SCENES])
def test_scene_gradient_is_bit_reproducible(oracle32, W, H, N, K, inv):
    """The unfused gradient of every scene used below: the same bits under GS_TUNE_BWD_WAVES_PER_CU 1, 16, 1, 16 (the call
    pattern of test_backward_wave_count_leaves_the_same_bits), and the float32 oracle's at the suite's bar."""
    p, cams, _ = fan.scene(W, H, N, K, SEED, invisible=inv or None)
    cot = _dev(fan.cotangent(W, H))
    r = _renderer(K, W, H)
    tp = {k: _dev(v) for k, v in p.items()}
    z = np.zeros(W * H, np.float32)
    for ci, cam in enumerate(cams):
        r.renderForward(tp, cam, wantDepth=False)
        out = []
        for waves in (1, 16, 1, 16):
            r.setTuning(bwd_waves_per_cu=waves)
            out.append({k: v.clone() for k, v in r.renderBackward(cot).items()})
        for o in out[1:]:
            for k in KEYS:
                assert torch.equal(o[k], out[0][k]), (ci, k)
        fw = oracle32.render_forward(p, cam.as_dict(), W, H, 16, 16, fan.DEGREE[K])
        want = oracle32.render_backward(p, cam.as_dict(), W, H, 16, 16, fan.DEGREE[K], fw, _np(cot).reshape(-1, 3), z, z)
        for k in KEYS:
            got, w = _np(out[0][k]).astype(np.float64).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
            if got.size:
                rel = np.abs(got - w).max() / (np.abs(w).max() + 1e-30)
                print(f"camera {ci} {k}: max |g| {np.abs(got).max():.3e}, against the float32 oracle {rel:.2e} (bar {GRAD_RTOL:.0e})")
                assert np.abs(got).max() > 0 and rel <= GRAD_RTOL, (ci, k, rel)
    r.close()


# ------------------------------------------------------------------------------------------------------------ 2. the dense step
@pytest.mark.parametrize("K,N,layout,scale", DENSE, ids=[f"K{c[0]}-N{c[1]}-{c[2]}" + ("" if c[3] == 1.0 else f"-scale{c[3]}") for c in DENSE])
def test_dense_fused_step(K, N, layout, scale):
    W, H = _size(N)
    p, cams, _ = fan.scene(W, H, N, K, SEED)
    r = _renderer(K, W, H)
    A = _make_arena(p, N, K, layout, r.device)
    tag = f"dense K{K} N{N} {layout}" + ("" if scale == 1.0 else f" scale{scale}")
    _steps(tag, r, A, cams, _dev(fan.cotangent(W, H)), A.ids >= 0, grad_scale=scale)
    r.close()


# ----------------------------------------------------------------------------------------------------------- 3. the sparse step
@pytest.mark.parametrize("K,N,inv,layout", SPARSE, ids=[f"K{c[0]}-N{c[1]}-{c[2]}-{c[3]}" for c in SPARSE])
def test_sparse_fused_step(K, N, inv, layout):
    W, H = _size(N, inv)
    p, cams, invisible = fan.scene(W, H, N, K, SEED, invisible=inv)
    r = _renderer(K, W, H)
    r.setSparseAdam(True)
    A = _make_arena(p, N, K, layout, r.device)
    for cam in cams:
        r.renderForward(A.params, cam, wantDepth=False)
        assert np.array_equal(_np(r.visibility()), ~invisible)
    on = (A.ids >= 0) & (~invisible)[np.maximum(A.rows, 0)]
    assert int(on.sum()) == int((~invisible).sum()) * sum(fan.row_floats(K).values())
    _steps(f"sparse K{K} N{N} {inv} {layout}", r, A, cams, _dev(fan.cotangent(W, H)), on)
    r.close()


# ----------------------------------------------------------------------------------------------------------- 4. the banded step
@pytest.mark.parametrize("K,d,N,layout", BANDS, ids=[f"K{c[0]}-d{c[1]}-N{c[2]}-{c[3]}" for c in BANDS])
def test_banded_fused_step(K, d, N, layout):
    W, H = _size(N)
    p, cams, _ = fan.scene(W, H, N, K, SEED)
    lact = fan.active_columns(d)
    assert lact < 3 * (K - 1)
    r = _renderer(K, W, H)
    r.setSHDegree(d)
    A = _make_arena(p, N, K, layout, r.device)
    on = (A.ids >= 0) & ~((A.ids == 2) & (A.cols >= lact))
    _steps(f"bands K{K} d{d} N{N} {layout}", r, A, cams, _dev(fan.cotangent(W, H)), on, lact=lact)
    r.close()


# ------------------------------------------------------------------------------------------------------ 5. stand-alone kernels
BIG = 8192 * 256 * 4 + 4099            # adam_kernel's grid is capped at 8192 x 256 float4: a second trip of 1024 float4, a tail of 3
SEAM = 8192 * 256 * 4


def _plain_inputs(n, seed, table_at=()):
    """Random p, g, m, v over ten decades of size, non-zero moments, a stretch of p = 0 (there p = -step exactly) and
    fused_adam_numpy.value_table planted at the given offsets."""
    rng = np.random.default_rng(seed)
    size = (10.0 ** rng.uniform(-9, 0, n)).astype(np.float32)
    g = size * rng.standard_normal(n, dtype=np.float32)
    m = size * rng.standard_normal(n, dtype=np.float32) * np.float32(0.5)
    v = size * size * rng.uniform(0.01, 1, n).astype(np.float32)
    p = rng.standard_normal(n, dtype=np.float32)
    p[n // 5:n // 5 + min(n // 10, 200000)] = 0.0
    t = fan.value_table([1.0])
    T = t["g"].shape[0]
    for at in table_at:
        at = min(max(at, 0), n - T)
        p[at:at + T], m[at:at + T], v[at:at + T], g[at:at + T] = t["p0"], t["m0"], t["v0"], t["g"]
    return p, g, m, v, T


def _judge_flat(tag, before, after, g_eff, on, lr_el, scale):
    idx = np.flatnonzero(on)
    for name in ("p", "m", "v"):
        bad = np.flatnonzero(~on & (fan.bits(after[name]) != fan.bits(before[name])))
        assert bad.size == 0, f"{tag}: {bad.size} elements of {name} outside the step changed bits, the first {int(bad[0])}"
    b = fan.bars(before["p"][idx], before["m"][idx], before["v"][idx], g_eff[idx], after["p"][idx], after["m"][idx], after["v"][idx],
                 lr_el[idx], scale=scale, **fan.ADAM)
    rec = REPORT.setdefault(tag, {})
    fails = []
    for name, rk in (("p", "ratio_p"), ("m", "ratio_m"), ("v", "ratio_v")):
        j = int(np.argmax(b[rk]))
        rec[name] = dict(ratio=float(b[rk][j]), element=int(idx[j]), beyond=int((b[rk] > 1).sum()), of=int(idx.size))
        print(f"{tag} {name}: largest error / bar {b[rk][j]:.3f} at element {int(idx[j])}; {int((b[rk] > 1).sum())} of {idx.size} beyond")
        if b[rk][j] > 1:
            fails.append(f"{name}: {int((b[rk] > 1).sum())} elements beyond the bar, the worst {b[rk][j]:.3g} x at element {int(idx[j])} "
                         f"(p0 {before['p'][idx[j]]!r} m0 {before['m'][idx[j]]!r} v0 {before['v'][idx[j]]!r} g {g_eff[idx[j]]!r} -> "
                         f"p {after['p'][idx[j]]!r} m {after['m'][idx[j]]!r} v {after['v'][idx[j]]!r})")
    # did the multiply-adds keep subnormals?  (v0 = 0, |g| = 1e-20: v is 1e-43 exactly where they do, 0 where they flush)
    probe = on & (before["v"] == 0) & (np.abs(g_eff) == np.float32(1e-20))
    if probe.any():
        kept = bool((after["v"][probe] > 0).all())
        rec["subnormal_moments_kept"] = kept
        print(f"{tag}: subnormal second moments {'kept' if kept else 'flushed to zero'} ({int(probe.sum())} probes)")
    # the step against the IEEE float32 step where p0 = 0 (p = -step, no subtraction rounding), in units of 2^-23 of the step
    zero = on & (before["p"] == 0) & (after["p"] != 0)
    if zero.any():
        lr64 = lr_el[zero].astype(np.float64)
        M, V = after["m"][zero].astype(np.float64), after["v"][zero].astype(np.float64)
        d64 = lr64 * M / (np.sqrt(V) + float(np.float32(1e-15)))
        ieee = (lr_el[zero] * after["m"][zero]) / (np.sqrt(after["v"][zero]) + np.float32(1e-15))
        dev = -after["p"][zero].astype(np.float64)
        ok = np.abs(d64) > 1e-30
        rec["step_vs_float64_in_2^-23"] = float((np.abs(dev - d64)[ok] / np.abs(d64[ok])).max() * 2.0 ** 23)
        rec["step_vs_ieee_float32_in_2^-23"] = float((np.abs(dev - ieee.astype(np.float64))[ok] / np.abs(d64[ok])).max() * 2.0 ** 23)
        rec["ieee_float32_vs_float64_in_2^-23"] = float((np.abs(ieee.astype(np.float64) - d64)[ok] / np.abs(d64[ok])).max() * 2.0 ** 23)
        print(f"{tag}: the step where p0 = 0 ({int(ok.sum())} elements), in units of 2^-23 of its size: against float64 "
              f"{rec['step_vs_float64_in_2^-23']:.3f}, against the IEEE float32 step {rec['step_vs_ieee_float32_in_2^-23']:.3f} "
              f"(that step against float64 {rec['ieee_float32_vs_float64_in_2^-23']:.3f}; derived worst case 3.5)")
    _write_report()
    assert not fails, f"{tag}: " + "; ".join(fails)


def _run_flat(r, fn, n, p, g, m, v, seg_end, lrs, scale, extra=()):
    tp, tg, tm, tv = (_dev(a) for a in (p, g, m, v))
    k = len(seg_end)
    rc = getattr(r.lib, fn)(r.ctx, n, C.c_void_p(tp.data_ptr()), C.c_void_p(tg.data_ptr()), C.c_void_p(tm.data_ptr()),
                            C.c_void_p(tv.data_ptr()), k, (C.c_longlong * k)(*[int(x) for x in seg_end]),
                            (C.c_float * k)(*[float(x) for x in lrs]), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-15),
                            C.c_float(scale), *extra)
    r._check(rc)
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(fan.bits(_np(tg)), fan.bits(g)), f"{fn} wrote the gradient buffer"
    return dict(p=_np(tp), m=_np(tm), v=_np(tv))


LRS8 = [1.6e-4, 5e-3, 1e-3, 2.5e-2, 2.5e-3, 1.25e-4, 2e-3, 1e-2]


def test_adam_step_past_the_grid_stride_seam():
    r = _renderer(1, 32, 16)
    n = BIG
    assert (n >> 2) > 8192 * 256 and n % 4 == 3
    p, g, m, v, T = _plain_inputs(n, 31, table_at=(0, SEAM - 70, n))      # start, across the seam, the tail (clamped to end at n)
    assert SEAM - 70 + T > SEAM + 64
    # eight segments; the second, fourth and seventh end off a multiple of four, the sixth sits on the seam
    seg_end = [1_000_000, 2_000_003, 3_100_000, 4_200_001, 6_000_000, SEAM, n - 2, n]
    assert [e % 4 for e in seg_end[:-1]].count(0) < 6
    before = dict(p=p, m=m, v=v)
    after = _run_flat(r, "gs_adam_step", n, p, g, m, v, seg_end, LRS8, 0.5)
    lr_el = np.asarray(LRS8, np.float32)[np.searchsorted(np.asarray(seg_end), np.arange(n), side="right")]
    _judge_flat("gs_adam_step n 8392707", before, after, g, np.ones(n, bool), lr_el, 0.5)
    assert (fan.bits(after["p"][SEAM:]) != fan.bits(p[SEAM:])).mean() > 0.9              # the second trip and the tail ran
    r.close()


def test_adam_step_visible_past_the_grid_stride_seam():
    r = _renderer(1, 32, 16)
    n = BIG
    widths = (3, 45, 1)
    S = n // sum(widths)
    N = S - 1000                                               # rows N .. S - 1 of every segment: the strided tail
    seg_end = [3 * S, 48 * S, n]                               # (the last segment takes the 36 floats left over: rows >= N)
    assert seg_end[0] % 4 and N < S
    p, g, m, v, T = _plain_inputs(n, 32, table_at=(0, SEAM - 70, seg_end[1] + 5))
    vis = np.random.default_rng(33).random(N) < 0.4
    on = sa.element_mask(vis, np.asarray(seg_end, np.int64), widths, N)
    assert int(on.sum()) == int(vis.sum()) * sum(widths) and on[SEAM:].any() and (~on[SEAM:]).any()
    tvis = _dev(vis.astype(np.uint8))
    lrs = LRS8[:3]
    before = dict(p=p, m=m, v=v)
    tp, tg, tm, tv = (_dev(a) for a in (p, g, m, v))
    r.adamStepVisible(tp, tg, tm, tv, seg_end, lrs, widths, N, tvis, 0.9, 0.999, 1e-15, 1.0)
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(fan.bits(_np(tg)), fan.bits(g))
    after = dict(p=_np(tp), m=_np(tm), v=_np(tv))
    lr_el = np.asarray(lrs, np.float32)[np.searchsorted(np.asarray(seg_end), np.arange(n), side="right")]
    _judge_flat("gs_adam_step_visible n 8392707", before, after, g, on, lr_el, 1.0)
    r.close()


@pytest.mark.parametrize("mode", ["null", "addN0", "addN4k", "addN4k+1"])
def test_adam_step_add(mode):
    r = _renderer(1, 32, 16)
    n = 10_007
    p, g, m, v, T = _plain_inputs(n, 34, table_at=(0, n))
    seg_end = [3001, 7002, n]
    lrs = LRS8[:3]
    addN = {"null": 0, "addN0": 0, "addN4k": 4 * 1200, "addN4k+1": 4 * 1200 + 1}[mode]
    add = np.zeros((addN + 3) // 4 * 4 + 4, np.float32)        # readable and zero up to the next multiple of four (and past it)
    add[:addN] = (np.abs(g[:addN]) * np.random.default_rng(35).standard_normal(addN)).astype(np.float32)
    tadd = _dev(add)
    assert tadd.data_ptr() % 16 == 0
    extra = (None, C.c_longlong(0)) if mode == "null" else (C.c_void_p(tadd.data_ptr()), C.c_longlong(addN))
    before = dict(p=p, m=m, v=v)
    after = _run_flat(r, "gs_adam_step_add", n, p, g, m, v, seg_end, lrs, 0.5, extra=extra)
    assert np.array_equal(_np(tadd), add)
    g_eff = g.copy()
    g_eff[:addN] = g[:addN] + add[:addN]                        # (the kernel's own float32 sum: one IEEE add)
    lr_el = np.asarray(lrs, np.float32)[np.searchsorted(np.asarray(seg_end), np.arange(n), side="right")]
    _judge_flat(f"gs_adam_step_add n 10007 {mode}", before, after, g_eff, np.ones(n, bool), lr_el, 0.5)
    if addN:
        assert (g_eff[:addN] != g[:addN]).mean() > 0.9
    else:                                                       # nothing to add: the bits of gs_adam_step
        plain = _run_flat(r, "gs_adam_step", n, p, g, m, v, seg_end, lrs, 0.5)
        for name in ("p", "m", "v"):
            assert np.array_equal(fan.bits(after[name]), fan.bits(plain[name])), name
    r.close()
