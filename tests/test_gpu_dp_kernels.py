"""The data-parallel backward kernels against the float64 restatement of tests/dp_numpy.py and the oracle.

Every kernel of the data-parallel step takes the R views' gathered colour cotangents as a plain input array, so what a
multi-rank run would feed them is reproduced here on one GPU:
  op level (synthetic inputs, no render, no atomics): gs_sh_grad_from_views, gs_sh_grad_from_views_adam and
    gs_sh_grad_from_views_adam_dir (sh_grad_from_views_kernel<false / true>, sh_views_dir_adam_kernel) at the row counts around
    the wave (64) and the workgroup (128), R = 1, 3, 16, every (K, degree) pair, in a GaussModel arena and in hand-built arenas
    with features_rest off the 16-byte grid;
  the gates: gs_set_update_gate, gs_set_gathered_gate (more than one block on a device), gs_set_gate_seen, gs_set_overflow_rider;
  per view on a rendered scene: gs_render_backward_dp_geom and gs_render_backward_dp_begin + _finish_geom
    (proj_bwd_geom_kernel<false / true>) against the oracle, the view-direction term of the xyz gradient from the restatement.

Bars.  SH gradient, xyz_add, densify statistic: the project's for gradShs / gradMeans3d (test_projection_forward_backward), rtol 2e-4
and atol 2e-5 max|want|, against float64.  Adam: test_adam_step_matches_numpy's (rtol 2e-6; atol 1e-7 / 1e-9 / 1e-12 for p / m / v)
against the float32 numpy Adam fed the gradient gs_sh_grad_from_views returned.  Rendered scene: GRAD_RTOL = 1e-3 of the tensor's
largest magnitude against the float32 oracle, 1e-4 max between two runs of the blend backward's float atomics.

Worst observed share of a bar (1.0 = the whole bar) on an MI355X, over the op-level cases; beside it the float32-vs-float64
qualification share of the same inputs (tests/test_dp_numpy_cpu.py: the float32 walk of the restatement, which may use half a bar):
  bar                           GPU vs reference            float32 walk vs float64 (qualification)
  SH gradient, dc               0.0034  N1000_R16_K16_deg3  }
  SH gradient, rest             0.0043  N129_R16_K16_deg3   }  0.0043  N129_R16_K16_deg3
  xyz_add                       0.0060  N63_R16_K25_deg4       0.0067  N129_R3_K25_deg4
  densify statistic             0.0015  N128_R3_K25_deg4       0.0013  N333_R16_K25_deg4
  Adam p (dc / rest)            0.087 / 0.053  N333_R1_K1_deg0 / N1000_R16_K16_deg3     (the kernel's hardware sqrt and reciprocal)
  Adam m, v                     0 (the same bits as numpy's float32: projection.hip is built without FMA contraction)
  features_rest off the 16-byte grid (K = 16, 4; N = 1, 65, 129): the same shares at the offsets 1, 2 and 3; none above 0.05
  gates (N333_R3_K25_deg4)      SH gradient 0.0016, xyz_add 0.0023; everything else there is a comparison of bits
Rendered scene (3001 Gaussians, 176 x 128, three views), worst share over the views, per configuration
(default / antialiased / white / block lists / depth and alpha cotangents):
  scales, rotation, opacity vs the oracle (1e-3 max)     0.006 0.013 0.004 / 0.010 0.014 0.005 / 0.007 0.013 0.004 / 0.008 0.012 0.003 / 0.020 0.013 0.001
  grad_xyz + d_r vs the oracle's xyz (1e-3 max)          0.0044 / 0.0053 / 0.0044 / 0.0048 / 0.0014
  color_cot vs the oracle's gradPacked (1e-3 max)        0.0064 / 0.0028 / 0.0064 / 0.0075 / 0.0014      (no channel entry left out)
  begin + finish_geom vs dp_geom (1e-4 max)              0.039 / 0.086 / 0.040 / 0.029 / 0.135            (worst of the five tensors)
  begin + finish vs dp_geom (1e-4 max)                   0.041 / 0.086 / 0.040 / 0.090 / 0.089
  summed SH gradient vs the oracle (rtol 1e-3)           0.25 / 0.19 / 0.25 / 0.077 / 0.066
  sum grad_xyz + xyz_add vs the oracle (1e-3 max)        0.0035 / 0.0047 / 0.0036 / 0.0039 / 0.0014
Zero raw quaternion: gs_render_backward, _dp, _dp_geom and _dp_begin + _finish_geom all leave NaN in the four rotation entries of
the visible and of the invisible row and finite values everywhere else; so does the float32 oracle.  No form had to change.
With GSPLAT_TEST_REPORTS=<directory> in the environment every test writes its shares to <directory>/dp_kernels_<case>.json.
"""
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_dpk_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dn = _load("dp_numpy")
LR_DC, LR_REST, B1, B2, EPS = 2.5e-3, 1.25e-4, 0.9, 0.999, 1e-15
GRAD_RTOL = 1e-3
INVALID_ARG, SIZE_MISMATCH = 1, 2
GEOM = ("xyz", "scales", "rotation", "opacity")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _record(case, shares):
    """Worst observed share of every bar of a case: printed, and kept as a file where GSPLAT_TEST_REPORTS names a directory
    (never fails the test)."""
    out = os.environ.get("GSPLAT_TEST_REPORTS")
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, f"dp_kernels_{case}.json"), "w") as f:
                json.dump({k: (v if isinstance(v, (str, list, dict)) else float(v)) for k, v in shares.items()}, f, indent=1, sort_keys=True)
        except OSError:
            pass
    print("dp_kernels", case, " ".join(f"{k}={v:.4g}" for k, v in shares.items() if isinstance(v, float)))


@pytest.fixture(scope="module")
def renderer_of():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    made = {}

    def get(degree, W=64, H=48, tile=(16, 16), white=False, aa=False):
        key = (degree, W, H, tile, white, aa)
        if key not in made:
            made[key] = GaussianRenderer(degree, W, H, tile, white, antialiased=aa)
        return made[key]

    yield get
    for r in made.values():
        r.close()


@functools.lru_cache(maxsize=None)
def _oracles():
    from oracle.oracle import Oracle
    return Oracle(np.float32), Oracle(np.float64)


@functools.lru_cache(maxsize=None)
def _ref(case):
    """A case's inputs and float64 reference, computed once and shared (read only)."""
    N, R, K, degree = case
    inp = dn.op_inputs(*case)
    b, gb = dn.basis64(_oracles()[1], degree, inp["xyz"], inp["centres"])
    dc, rest = dn.sh_grad(b, inp["cc"], K)
    return dict(inp=inp, b=b, gb=gb, dc=dc, rest=rest)


def _model(inp, device, seed=1):
    """The case's SH tensors and moments in a GaussModel arena (the real segment offsets); every other element, pad and moment
    random, so that a stray store shows."""
    from gaussiansplattingmlx_amd.trainer import GaussModel
    N, K = inp["N"], inp["K"]
    rng = np.random.default_rng(seed)
    p = dict(xyz=inp["xyz"], features_dc=inp["features_dc"], features_rest=inp["features_rest"],
             scales=rng.normal(-3, 0.5, (N, 3)).astype(np.float32), rotation=rng.normal(0, 1, (N, 4)).astype(np.float32),
             opacity=rng.normal(0, 1, N).astype(np.float32))
    model = GaussModel(p, device)
    g = torch.Generator().manual_seed(seed)
    model.m.copy_(torch.randn(model.numel, generator=g))
    model.v.copy_(torch.rand(model.numel, generator=g) * 0.99 + 0.01)
    for name, buf in (("m", model.m), ("v", model.v)):
        views = model._carve(buf, N)
        views["features_dc"].copy_(torch.as_tensor(inp[name + "_dc"]))
        views["features_rest"].copy_(torch.as_tensor(inp[name + "_rest"]))
    torch.cuda.synchronize()
    return model


def _state(model):
    return model.arena.clone(), model.m.clone(), model.v.clone()


def _sh_mask(model, N, K):
    """True on the elements of features_dc / features_rest in the arena layout."""
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    mask = torch.zeros(model.numel, dtype=torch.bool, device=model.arena.device)
    for k, off in zip(ARENA_ORDER, model.seg_start):
        if k == "features_dc":
            mask[off:off + 3 * N] = True
        if k == "features_rest":
            mask[off:off + 3 * (K - 1) * N] = True
    return mask


def _adam_bars(shares, tag, got, want):
    for name, atol, g, w in zip("pmv", (1e-7, 1e-9, 1e-12), got, want):
        s = dn.bar_ratio(g, w, 2e-6, atol)
        shares[f"{tag}_{name}"] = max(shares.get(f"{tag}_{name}", 0.0), s)
        assert s <= 1.0, (tag, name, s)


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def _xyz_add_buffer(N, device):
    """[3 N rounded up to four floats], 16-byte aligned, the pad zero."""
    return torch.zeros((3 * N + 3) & ~3, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------------------------------ op level
def _sh_grad_checks(r, ref, case, shares):
    N, R, K, degree = case
    inp = ref["inp"]
    xyz, cc = _dev(inp["xyz"], r.device), _dev(inp["cc"], r.device)
    g = r.shGradFromViews(xyz, cc, inp["centres"], K)
    dc, rest = _np(g["features_dc"]), _np(g["features_rest"])
    again = r.shGradFromViews(xyz, cc, inp["centres"], K)
    assert torch.equal(again["features_dc"], g["features_dc"]) and torch.equal(again["features_rest"], g["features_rest"])
    assert dc.shape == (N, 1, 3) and rest.shape == (N, K - 1, 3)
    shares["sh_grad_dc"], shares["sh_grad_rest"] = dn.max_bar_ratio(dc, ref["dc"]), dn.max_bar_ratio(rest, ref["rest"])
    assert np.abs(ref["dc"]).max() > 0
    assert shares["sh_grad_dc"] <= 1.0 and shares["sh_grad_rest"] <= 1.0, shares
    if K > (degree + 1) ** 2:
        assert not rest[:, (degree + 1) ** 2 - 1:, :].any()          # bands above the degree: exactly zero
    if degree > 0 and K > 1:
        assert np.abs(rest[:, :(degree + 1) ** 2 - 1, :]).max() > 0
    return xyz, cc, dc, rest


@pytest.mark.parametrize("case", dn.OP_CASES, ids=dn.case_id)
def test_sh_rebuild_kernels_against_float64(renderer_of, case):
    N, R, K, degree = case
    ref = _ref(case)
    inp = ref["inp"]
    r = renderer_of(degree)
    shares = {}
    xyz, cc, gdc, grest = _sh_grad_checks(r, ref, case, shares)
    own_t = [_dev(inp["own"][v], r.device) for v in range(R)]
    try:
        for scale in (1.0, 0.125):
            tag = "adam_s%g" % scale
            # gs_sh_grad_from_views_adam, two steps: the second starts from moments this kernel wrote
            model = _model(inp, r.device)
            before = _state(model)
            mask = _sh_mask(model, N, K)
            want = dict(dc=(inp["features_dc"], inp["m_dc"], inp["v_dc"]), rest=(inp["features_rest"], inp["m_rest"], inp["v_rest"]))
            steps = []
            for step in range(2):
                r.shGradFromViewsAdam(model.getParams(), cc, inp["centres"], model.arena, model.m, model.v, LR_DC, LR_REST, scale)
                want["dc"] = dn.adam32(*want["dc"], gdc, LR_DC, B1, B2, EPS, scale)
                want["rest"] = dn.adam32(*want["rest"], grest, LR_REST, B1, B2, EPS, scale)
                mv, vv = model._carve(model.m, N), model._carve(model.v, N)
                for k, key in (("dc", "features_dc"), ("rest", "features_rest")):
                    _adam_bars(shares, f"{tag}_{k}", (_np(model.getParams()[key]), _np(mv[key]), _np(vv[key])), want[k])
                now = _state(model)
                for a, b in zip(before, now):
                    assert torch.equal(a[~mask], b[~mask])              # every other element and moment: untouched
                steps.append(now)
            assert not torch.equal(steps[0][0][mask], before[0][mask])
            # gs_sh_grad_from_views_adam_dir: the same SH update bit for bit + xyz_add + the densify statistic
            for pat in dn.own_patterns(R):
                model = _model(inp, r.device)
                accum = _dev(inp["accum"], r.device).clone()
                r.setGradNormAccum(accum)
                xyz_add = _xyz_add_buffer(N, r.device)
                own = [own_t[v] if v in pat else None for v in range(R)]
                acc_want = inp["accum"].astype(np.float64)
                for step in range(2):
                    rest_now = _np(model.getParams()["features_rest"]).copy()
                    r.shGradFromViewsAdamDir(model.getParams(), cc, inp["centres"], own, model.arena, model.m, model.v, LR_DC,
                                             LR_REST, scale, xyz_add)
                    for a, b in zip(steps[step], _state(model)):
                        assert torch.equal(a, b), (pat, step)           # == gs_sh_grad_from_views_adam, bit for bit
                    d = dn.dir_terms(ref["gb"], inp["cc"], rest_now)
                    s = dn.max_bar_ratio(_np(xyz_add)[:3 * N].reshape(N, 3), d.sum(0))
                    shares["xyz_add"] = max(shares.get("xyz_add", 0.0), s)
                    assert s <= 1.0, ("xyz_add", pat, step, s)
                    assert not _np(xyz_add)[3 * N:].any()
                    if not pat:
                        assert torch.equal(accum, _dev(inp["accum"], r.device))      # no own view: the accumulator is not touched
                    else:
                        acc_want = acc_want + dn.statistic(d, inp["own"], pat)
                        s = dn.max_bar_ratio(_np(accum), acc_want)
                        shares["statistic"] = max(shares.get("statistic", 0.0), s)
                        assert s <= 1.0, ("statistic", pat, step, s)
                        acc_want = _np(accum).astype(np.float64)      # before + statistic: the next step's `before` is this one's result
    finally:
        r.setGradNormAccum(None)
    _record(dn.case_id(case), shares)


# --------------------------------------------------------------------------------------------------------- arena placements
def _hand_arena(inp, off_mod, device, seed=3):
    """features_dc and features_rest at hand-picked float offsets of three arenas (parameters, m, v) of one layout:
    features_rest at an offset = off_mod (mod 4), guard floats around both."""
    N, K = inp["N"], inp["K"]
    L = 3 * (K - 1)
    dc_off = 5                                            # (12-byte rows, packed stores: any float offset)
    rest_off = ((dc_off + 3 * N + 8 + 3) & ~3) + off_mod
    n = rest_off + N * L + 9
    g = torch.Generator().manual_seed(seed)
    bufs = [torch.randn(n + 4, generator=g).to(device), torch.randn(n + 4, generator=g).to(device),
            (torch.rand(n + 4, generator=g) * 0.99 + 0.01).to(device)]
    for b in bufs:
        assert b.data_ptr() % 16 == 0
    views = []
    for b, names in zip(bufs, (("features_dc", "features_rest"), ("m_dc", "m_rest"), ("v_dc", "v_rest"))):
        dc, rest = b[dc_off:dc_off + 3 * N].view(N, 1, 3), b[rest_off:rest_off + N * L].view(N, K - 1, 3)
        dc.copy_(torch.as_tensor(inp[names[0]]))
        rest.copy_(torch.as_tensor(inp[names[1]]))
        views.append((dc, rest))
    mask = torch.zeros(n, dtype=torch.bool, device=device)
    mask[dc_off:dc_off + 3 * N] = True
    mask[rest_off:rest_off + N * L] = True
    params = dict(xyz=_dev(inp["xyz"], device), features_dc=views[0][0], features_rest=views[0][1])
    assert (params["features_rest"].data_ptr() // 4) % 4 == off_mod
    return params, [b[:n] for b in bufs], views, mask


@pytest.mark.parametrize("off_mod", [1, 2, 3])
@pytest.mark.parametrize("case", dn.PLACEMENT_CASES, ids=dn.case_id)
def test_features_rest_off_the_16_byte_grid(renderer_of, case, off_mod):
    """adam_rows' scalar head and tail: K = 16 (45 floats a row) and K = 4 (9), features_rest starting 1, 2, 3 floats past a
    16-byte boundary; sh_rows_out's element-wise path for the gradient written to such an address."""
    N, R, K, degree = case
    ref = _ref(case)
    inp = ref["inp"]
    r = renderer_of(degree)
    shares = {}
    xyz, cc, gdc, grest = _sh_grad_checks(r, ref, case, shares)
    # the gradient into a misplaced tensor: the same bits
    spare = torch.full((N * 3 * (K - 1) + 16,), 7.0, device=r.device)
    out = dict(features_dc=torch.empty(N, 1, 3, device=r.device),
               features_rest=spare[4 + off_mod:4 + off_mod + N * 3 * (K - 1)].view(N, K - 1, 3))
    r.shGradFromViews(xyz, cc, inp["centres"], K, out=out)
    assert np.array_equal(_np(out["features_rest"]), grest) and np.array_equal(_np(out["features_dc"]), gdc)
    assert bool((spare[:4 + off_mod] == 7.0).all()) and bool((spare[4 + off_mod + N * 3 * (K - 1):] == 7.0).all())
    scale = 0.125
    pat = dn.own_patterns(R)[1]
    own = [_dev(inp["own"][v], r.device) if v in pat else None for v in range(R)]
    results = {}
    try:
        for form in ("adam", "adam_dir"):
            params, (arena, m, v), views, mask = _hand_arena(inp, off_mod, r.device)
            before = [b.clone() for b in (arena, m, v)]
            want = dict(dc=(inp["features_dc"], inp["m_dc"], inp["v_dc"]), rest=(inp["features_rest"], inp["m_rest"], inp["v_rest"]))
            accum = _dev(inp["accum"], r.device).clone()
            r.setGradNormAccum(accum if form == "adam_dir" else None)
            xyz_add = _xyz_add_buffer(N, r.device)
            acc_want = inp["accum"].astype(np.float64)
            for step in range(2):
                rest_now = _np(params["features_rest"]).copy()
                if form == "adam":
                    r.shGradFromViewsAdam(params, cc, inp["centres"], arena, m, v, LR_DC, LR_REST, scale)
                else:
                    r.shGradFromViewsAdamDir(params, cc, inp["centres"], own, arena, m, v, LR_DC, LR_REST, scale, xyz_add)
                    d = dn.dir_terms(ref["gb"], inp["cc"], rest_now)
                    shares["xyz_add"] = max(shares.get("xyz_add", 0.0), dn.max_bar_ratio(_np(xyz_add)[:3 * N].reshape(N, 3), d.sum(0)))
                    acc_want = acc_want + dn.statistic(d, inp["own"], pat)
                    shares["statistic"] = max(shares.get("statistic", 0.0), dn.max_bar_ratio(_np(accum), acc_want))
                    acc_want = _np(accum).astype(np.float64)
                    assert shares["xyz_add"] <= 1.0 and shares["statistic"] <= 1.0, shares
                want["dc"] = dn.adam32(*want["dc"], gdc, LR_DC, B1, B2, EPS, scale)
                want["rest"] = dn.adam32(*want["rest"], grest, LR_REST, B1, B2, EPS, scale)
                for i, k in enumerate(("dc", "rest")):
                    _adam_bars(shares, f"{form}_{k}", tuple(_np(views[j][i]) for j in range(3)), want[k])
                for a, b in zip(before, (arena, m, v)):
                    assert torch.equal(a[~mask], b[~mask])              # guards and every other float: untouched
            results[form] = [b.clone() for b in (arena, m, v)]
        for a, b in zip(results["adam"], results["adam_dir"]):
            assert torch.equal(a, b)
    finally:
        r.setGradNormAccum(None)
    _record(f"{dn.case_id(case)}_offset{off_mod}", shares)


@pytest.mark.parametrize("K,degree", [(25, 4), (9, 2)])
def test_rows_of_whole_float4_off_the_16_byte_grid_are_refused(renderer_of, K, degree):
    """With 3 (K - 1) a multiple of four the kernels move the rows as 16-byte words (sh_rows_in / sh_rows_out / the kept
    registers), whatever the tensor's address: such a layout is refused by all three entry points, nothing is launched."""
    from gaussiansplattingmlx_amd._lib import GsplatError
    N, R = 65, 3
    inp = dn.op_inputs(N, R, K, degree)
    r = renderer_of(degree)
    cc = _dev(inp["cc"], r.device)
    for off_mod in (1, 2, 3):
        params, (arena, m, v), views, mask = _hand_arena(inp, off_mod, r.device)
        before = [b.clone() for b in (arena, m, v)]
        with pytest.raises(GsplatError) as ei:
            r.shGradFromViewsAdam(params, cc, inp["centres"], arena, m, v, LR_DC, LR_REST, 1.0)
        assert ei.value.code == INVALID_ARG and "16-byte" in str(ei.value)
        with pytest.raises(GsplatError) as ei:
            r.shGradFromViewsAdamDir(params, cc, inp["centres"], [None] * R, arena, m, v, LR_DC, LR_REST, 1.0, _xyz_add_buffer(N, r.device))
        assert ei.value.code == INVALID_ARG
        out = dict(features_dc=torch.empty(N, 1, 3, device=r.device), features_rest=params["features_rest"])
        with pytest.raises(GsplatError) as ei:
            r.shGradFromViews(params["xyz"], cc, inp["centres"], K, out=out)
        assert ei.value.code == INVALID_ARG
        torch.cuda.synchronize()
        for a, b in zip(before, (arena, m, v)):
            assert torch.equal(a, b)
    # a moment arena off the grid (adam_rows takes its head from the parameter offset alone)
    model = _model(inp, r.device)
    m_off = torch.zeros(model.numel + 8, device=r.device)[1:1 + model.numel]
    with pytest.raises(GsplatError) as ei:
        r.shGradFromViewsAdam(model.getParams(), cc, inp["centres"], model.arena, m_off, model.v, LR_DC, LR_REST, 1.0)
    assert ei.value.code == INVALID_ARG


# ----------------------------------------------------------------------------------------------------------------- the gates
def _gate_setup(renderer_of):
    case = dn.GATE_CASE
    ref = _ref(case)
    inp = ref["inp"]
    r = renderer_of(case[3])
    return case, ref, inp, r


def _step_both(r, inp, cc, scale=0.125, pat=None):
    """One step of both Adam forms from the same start: (states after, xyz_add, accumulator)."""
    N, R = inp["N"], inp["R"]
    pat = tuple(range(R)) if pat is None else pat
    own = [_dev(inp["own"][v], r.device) if v in pat else None for v in range(R)]
    out = {}
    for form in ("adam", "adam_dir"):
        model = _model(inp, r.device)
        accum = _dev(inp["accum"], r.device).clone()
        r.setGradNormAccum(accum)
        xyz_add = _xyz_add_buffer(N, r.device)
        if form == "adam":
            r.shGradFromViewsAdam(model.getParams(), cc, inp["centres"], model.arena, model.m, model.v, LR_DC, LR_REST, scale)
        else:
            r.shGradFromViewsAdamDir(model.getParams(), cc, inp["centres"], own, model.arena, model.m, model.v, LR_DC, LR_REST,
                                     scale, xyz_add)
        torch.cuda.synchronize()
        out[form] = dict(state=_state(model), xyz_add=xyz_add, accum=accum, model=model)
    return out


def _reset(r):
    r.lib.gs_set_update_gate(r.ctx, None)
    r.lib.gs_set_gathered_gate(r.ctx, 0, 0, None)
    r.lib.gs_set_gate_seen(r.ctx, None)
    r.lib.gs_set_overflow_rider(r.ctx, None)
    r.setGradNormAccum(None)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_update_gate_raised_freezes_both_adam_forms(renderer_of):
    case, ref, inp, r = _gate_setup(renderer_of)
    N = case[0]
    cc = _dev(inp["cc"], r.device)
    start = _state(_model(inp, r.device))
    acc0 = _dev(inp["accum"], r.device)
    gate = torch.zeros(4, dtype=torch.int32, device=r.device)
    seen = torch.zeros(4, dtype=torch.int32, device=r.device)
    try:
        free = _step_both(r, inp, cc)
        assert not _same(free["adam"]["state"], start) and _same(free["adam"]["state"], free["adam_dir"]["state"])
        assert not torch.equal(free["adam_dir"]["accum"], acc0)
        r._check(r.lib.gs_set_update_gate(r.ctx, C.c_void_p(gate.data_ptr())))
        r._check(r.lib.gs_set_gate_seen(r.ctx, C.c_void_p(seen.data_ptr())))
        open_ = _step_both(r, inp, cc)                               # the word is 0: the ungated step, and nothing is seen
        for form in ("adam", "adam_dir"):
            assert _same(open_[form]["state"], free[form]["state"])
        assert torch.equal(open_["adam_dir"]["xyz_add"], free["adam_dir"]["xyz_add"]) and int(seen[0]) == 0
        for form in ("adam", "adam_dir"):
            gate[0] = 1
            seen.zero_()
            model = _model(inp, r.device)
            accum = acc0.clone()
            r.setGradNormAccum(accum)
            xyz_add = _xyz_add_buffer(N, r.device)
            if form == "adam":
                r.shGradFromViewsAdam(model.getParams(), cc, inp["centres"], model.arena, model.m, model.v, LR_DC, LR_REST, 0.125)
            else:
                own = [_dev(inp["own"][v], r.device) for v in range(case[1])]
                r.shGradFromViewsAdamDir(model.getParams(), cc, inp["centres"], own, model.arena, model.m, model.v, LR_DC, LR_REST,
                                         0.125, xyz_add)
                assert torch.equal(xyz_add, free["adam_dir"]["xyz_add"])      # the geometry slice's gradient is still complete
            torch.cuda.synchronize()
            assert _same(_state(model), start), form                 # arena, m, v: bit-identical
            assert torch.equal(accum, acc0), form
            assert int(seen[0]) == 1, form
        gate[0] = 0
        again = _step_both(r, inp, cc)
        for form in ("adam", "adam_dir"):
            assert _same(again[form]["state"], free[form]["state"])
        assert torch.equal(again["adam_dir"]["accum"], free["adam_dir"]["accum"])
    finally:
        _reset(r)
    xa = _np(free["adam_dir"]["xyz_add"])[:3 * N].reshape(N, 3)
    _record("gate_update", dict(xyz_add=dn.max_bar_ratio(xa, dn.dir_terms(ref["gb"], inp["cc"], inp["features_rest"]).sum(0))))


def _gathered(inp, device, words):
    """The R blocks of 3 N + 4 floats a multi-rank all-gather would leave: a rank's cotangents, then its gate word."""
    N, R = inp["N"], inp["R"]
    bf = 3 * N + 4
    blocks = torch.zeros(R, bf, dtype=torch.float32, device=device)
    blocks[:, :3 * N] = _dev(inp["cc"], device).reshape(R, 3 * N)
    blocks[:, 3 * N + 1:] = 5.0                                       # (the pad is nobody's word)
    for rnk, w in words.items():
        blocks[rnk, 3 * N] = w
    return blocks, bf


@pytest.mark.parametrize("raised", ["none", "last", "first"])
def test_gathered_gate_ors_the_words_of_every_block(renderer_of, raised):
    """More than one block on a device: the kernels find rank r's cotangents at r * block_floats and OR the words at [3 N]."""
    case, ref, inp, r = _gate_setup(renderer_of)
    N, R, K = case[:3]
    cc = _dev(inp["cc"], r.device)
    start = _state(_model(inp, r.device))
    acc0 = _dev(inp["accum"], r.device)
    words = {"none": {}, "last": {R - 1: 1.0}, "first": {0: 1.0}}[raised]
    blocks, bf = _gathered(inp, r.device, words)
    reduced = torch.full((4,), 77, dtype=torch.int32, device=r.device)
    seen = torch.zeros(4, dtype=torch.int32, device=r.device)
    shares = {}
    try:
        free = _step_both(r, inp, cc)
        g_free = r.shGradFromViews(_dev(inp["xyz"], r.device), cc, inp["centres"], K)
        r._check(r.lib.gs_set_gathered_gate(r.ctx, bf, R, C.c_void_p(reduced.data_ptr())))
        r._check(r.lib.gs_set_gate_seen(r.ctx, C.c_void_p(seen.data_ptr())))
        # gs_sh_grad_from_views under the layout: the full gradients, and the reduced word published
        g = r.shGradFromViews(_dev(inp["xyz"], r.device), blocks, inp["centres"], K)
        torch.cuda.synchronize()
        assert torch.equal(g["features_dc"], g_free["features_dc"]) and torch.equal(g["features_rest"], g_free["features_rest"])
        assert (int(reduced[0]) != 0) == bool(words) and int(reduced[1]) == 77
        shares["sh_grad_rest"] = dn.max_bar_ratio(_np(g["features_rest"]), ref["rest"])
        assert shares["sh_grad_rest"] <= 1.0
        for form in ("adam", "adam_dir"):
            reduced.fill_(77)
            seen.zero_()
            model = _model(inp, r.device)
            accum = acc0.clone()
            r.setGradNormAccum(accum)
            xyz_add = _xyz_add_buffer(N, r.device)
            if form == "adam":
                r.shGradFromViewsAdam(model.getParams(), blocks, inp["centres"], model.arena, model.m, model.v, LR_DC, LR_REST, 0.125)
            else:
                own = [_dev(inp["own"][v], r.device) for v in range(R)]
                r.shGradFromViewsAdamDir(model.getParams(), blocks, inp["centres"], own, model.arena, model.m, model.v, LR_DC,
                                         LR_REST, 0.125, xyz_add)
                assert torch.equal(xyz_add, free["adam_dir"]["xyz_add"])
            torch.cuda.synchronize()
            if words:
                assert _same(_state(model), start), form             # nothing moves
                assert torch.equal(accum, acc0)
                assert int(reduced[0]) != 0 and int(seen[0]) == 1
            else:
                assert _same(_state(model), free[form]["state"]), form        # bit-identical to the run without a layout
                assert torch.equal(accum, free[form]["accum"])
                assert int(reduced[0]) == 0 and int(seen[0]) == 0
            assert int(reduced[1]) == 77 and int(seen[1]) == 0
    finally:
        _reset(r)
    _record(f"gate_gathered_{raised}", shares)


def test_gathered_gate_layout_and_xyz_add_refusals(renderer_of):
    from gaussiansplattingmlx_amd._lib import GsplatError
    case, ref, inp, r = _gate_setup(renderer_of)
    N, R, K = case[:3]
    blocks, bf = _gathered(inp, r.device, {})
    model = _model(inp, r.device)
    start = _state(model)
    xyz_add = _xyz_add_buffer(N + 2, r.device)
    own = [None] * R

    def all_three(cc_all):
        for call in (lambda: r.shGradFromViews(model.getParams()["xyz"], cc_all, inp["centres"][:cc_all.shape[0]], K),
                     lambda: r.shGradFromViewsAdam(model.getParams(), cc_all, inp["centres"][:cc_all.shape[0]], model.arena, model.m,
                                                   model.v, LR_DC, LR_REST, 1.0),
                     lambda: r.shGradFromViewsAdamDir(model.getParams(), cc_all, inp["centres"][:cc_all.shape[0]], own[:cc_all.shape[0]],
                                                      model.arena, model.m, model.v, LR_DC, LR_REST, 1.0, xyz_add)):
            with pytest.raises(GsplatError) as ei:
                call()
            assert ei.value.code == SIZE_MISMATCH, str(ei.value)

    try:
        r._check(r.lib.gs_set_gathered_gate(r.ctx, bf, R, None))
        all_three(blocks[:R - 1])                                     # R != count
        r._check(r.lib.gs_set_gathered_gate(r.ctx, 3 * N, R, None))
        all_three(blocks)                                             # block_floats < 3 N + 1: no room for the word
        r._check(r.lib.gs_set_gathered_gate(r.ctx, 0, 0, None))
        with pytest.raises(GsplatError) as ei:                        # xyz_add off the 16-byte grid
            r.shGradFromViewsAdamDir(model.getParams(), _dev(inp["cc"], r.device), inp["centres"], own, model.arena, model.m, model.v,
                                     LR_DC, LR_REST, 1.0, xyz_add[1:])
        assert ei.value.code == INVALID_ARG and "16-byte" in str(ei.value)
        assert r.lib.gs_set_gathered_gate(r.ctx, bf, 17, None) == INVALID_ARG
        assert r.lib.gs_set_gathered_gate(r.ctx, -1, 1, None) == INVALID_ARG
        torch.cuda.synchronize()
        assert _same(_state(model), start)
    finally:
        _reset(r)


def test_overflow_rider_writes_the_forwards_word(renderer_of):
    """gs_set_overflow_rider + gs_render_backward_dp_geom: 0.0f after a forward that fitted, 1.0f after one that overflowed a
    too-small pair reserve (the recipe of test_block_lists_overflow_is_reported_and_regrown)."""
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    p, cams, W, H = dn.e2e_scene()
    N = p["xyz"].shape[0]
    r0 = renderer_of(4, W, H)
    tp = {k: _dev(v, r0.device) for k, v in p.items()}
    cot = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(r0.device)

    def backward(r):
        blk = torch.full((3 * N + 4,), 7.0, device=r.device)          # a rank's gather block: cotangents, then the word
        out = {k: torch.empty_like(tp[k]) for k in GEOM}
        r._check(r.lib.gs_set_overflow_rider(r.ctx, C.c_void_p(blk.data_ptr() + 12 * N)))
        r.renderBackwardDPGeom(cot, blk[:3 * N].view(N, 3), out, torch.empty(N, 3, device=r.device))
        torch.cuda.synchronize()
        return blk

    try:
        r0.renderForward(tp, cams[0])
        M = r0.stats()["M"]
        blk = backward(r0)
        assert float(blk[3 * N]) == 0.0 and bool((blk[3 * N + 1:] == 7.0).all()) and bool((blk[:3 * N] != 7.0).all())
    finally:
        _reset(r0)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    try:
        r.reserve(N, M // 3)                                          # too small on purpose
        r.setTuning(host_overflow_errors=0)                           # as a data-parallel host: no rank leaves a step alone
        res = r.renderForward(tp, cams[0])
        blk = backward(r)
        assert float(blk[3 * N]) == 1.0 and bool((blk[3 * N + 1:] == 7.0).all())
        assert not bool(res.render.any())
        with pytest.raises(GsplatError) as ei:
            r.sync()
        assert ei.value.code == 3
    finally:
        _reset(r)
        r.close()


# ------------------------------------------------------------------------------------------------ per view, on a rendered scene
CONFIGS = dict(default=dict(), antialiased=dict(aa=True), white=dict(white=True), block_lists=dict(tile=(50, 38)),
               depth_alpha=dict(cots=True))


@functools.lru_cache(maxsize=None)
def _scene_basis():
    p, cams, W, H = dn.e2e_scene()
    centres = np.stack([c.cameraCenter for c in cams]).astype(np.float32)
    return dn.basis64(_oracles()[1], 4, p["xyz"], centres)


def _oracle_view(o, p, cam, W, H, tile, white, cots, alpha=None):
    c = cam.as_dict()
    fw = o.render_forward(p, c, W, H, tile[0], tile[1], 4, white)
    if alpha is not None:          # hand the oracle the HIP forward's saved state so both sides undo the same T
        fw = dict(fw)
        fw["alpha"] = alpha
    return fw, o.render_backward(p, c, W, H, tile[0], tile[1], 4, fw, *cots, white)


def _geom_out(tp):
    return {k: torch.empty_like(tp[k]) for k in GEOM}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_per_view_backward_forms_against_the_oracle(renderer_of, oracle32, config):
    cfg = CONFIGS[config]
    tile, white, aa = cfg.get("tile", (16, 16)), cfg.get("white", False), cfg.get("aa", False)
    p, cams, W, H = dn.e2e_scene()
    N, K = p["xyz"].shape[0], 25
    o = oracle32
    if aa:
        o = _load("test_antialiasing_cpu").AAOracle(oracle32)
    r = renderer_of(4, W, H, tile, white, aa)
    tp = {k: _dev(v, r.device) for k, v in p.items()}
    gb = _scene_basis()[1]
    rng = np.random.default_rng(5)
    shares, ccs, left_out = {}, [], 0.0
    sums = {k: 0.0 for k in ("xyz", "features_dc", "features_rest")}
    sum_geom_xyz = torch.zeros(N, 3, device=r.device)
    owns = []

    def worst(k, v):
        shares[k] = max(shares.get(k, 0.0), v)

    for v, cam in enumerate(cams):
        cC = rng.normal(0, 1, (W * H, 3)).astype(np.float32)
        if cfg.get("cots"):
            cD, cA = rng.normal(size=W * H).astype(np.float32) * 0.1, rng.normal(size=W * H).astype(np.float32)
        else:
            cD = cA = np.zeros(W * H, np.float32)
        tC = _dev(cC.reshape(H, W, 3), r.device)
        tD, tA = (_dev(cD.reshape(H, W), r.device), _dev(cA.reshape(H, W), r.device)) if cfg.get("cots") else (None, None)
        res = r.renderForward(tp, cam, want_radii=True)
        radii, alpha = _np(res.radii).copy(), _np(res.alpha).reshape(-1).copy()
        fw, want = _oracle_view(o, p, cam, W, H, tile, white, (cC, cD, cA), alpha if cfg.get("cots") else None)
        # the one-call form
        g, cc, own = _geom_out(tp), torch.full((N, 3), 9.0, device=r.device), torch.full((N, 3), 9.0, device=r.device)
        r.renderBackwardDPGeom(tC, cc, g, own, tD, tA)
        assert torch.equal(own, g["xyz"])                              # xyz_own == grad_xyz, bit for bit
        off = torch.as_tensor(radii == 0, device=r.device)
        assert 0 < int(off.sum()) < N
        for name, t in (("color_cot", cc), ("xyz_own", own)) + tuple(g.items()):
            assert not bool(t[off].any()), name                        # radius 0: exactly zero in all six outputs
            assert bool(torch.isfinite(t).all()), name
        for k in ("scales", "rotation", "opacity"):
            worst(k, _rel(_np(g[k]), want[k].reshape(_np(g[k]).shape)) / GRAD_RTOL)
        d = dn.dir_terms(gb[v:v + 1], _np(cc)[None], p["features_rest"])[0]
        worst("xyz_plus_d", _rel(_np(g["xyz"]).astype(np.float64) + d, want["xyz"]) / GRAD_RTOL)
        assert np.abs(d).max() > 1e-3 * np.abs(want["xyz"]).max()      # (the term matters on this scene)
        # the colour cotangent: g where the oracle's clamped colour is above the cap, 0 where it is exactly 0
        col, gcol = fw["proj"]["color"], want["gradPacked"][:, 6:9]
        expect = np.where(col > 1e-5, gcol, 0.0)
        judged = (col > 1e-5) | (col == 0)
        left_out = max(left_out, 1.0 - judged.mean())
        worst("color_cot", float(np.abs(np.where(judged, _np(cc) - expect, 0.0)).max() / np.abs(gcol).max()) / GRAD_RTOL)
        assert not _np(cc)[col == 0].any()
        # begin + finish_geom, and begin + finish, each with a blend backward of its own (float atomics: 1e-4 max)
        r.renderForward(tp, cam)
        cc2 = r.renderBackwardDPBegin(tC, tD, tA)
        g2, own2 = _geom_out(tp), torch.empty(N, 3, device=r.device)
        r.renderBackwardDPFinishGeom(g2, own2)
        assert torch.equal(own2, g2["xyz"])
        worst("two_halves_color_cot", _rel(_np(cc2), _np(cc)) / 1e-4)
        for k in GEOM:
            worst("two_halves_" + k, _rel(_np(g2[k]), _np(g[k])) / 1e-4)
        r.renderForward(tp, cam)
        r.renderBackwardDPBegin(tC, tD, tA)
        g3 = r.renderBackwardDPFinish()
        for k in ("scales", "rotation", "opacity"):
            worst("finish_" + k, _rel(_np(g3[k]), _np(g[k])) / 1e-4)
        worst("finish_xyz", _rel(_np(g3["xyz"]).astype(np.float64), _np(g["xyz"]).astype(np.float64) + d) / GRAD_RTOL)
        ccs.append(cc)
        owns.append(own)
        sum_geom_xyz += g["xyz"]
        for k in sums:
            sums[k] = sums[k] + want[k].astype(np.float64)
    assert left_out <= 1e-3
    # summed over the three views
    cc_all = torch.stack(ccs)
    centres = np.stack([c.cameraCenter for c in cams])
    sh = r.shGradFromViews(tp["xyz"], cc_all, centres, K)
    for k in ("features_dc", "features_rest"):
        wk = sums[k].reshape(_np(sh[k]).shape)
        worst("summed_" + k, dn.bar_ratio(_np(sh[k]), wk, 1e-3, 1e-5 * np.abs(wk).max()))
    model = _model(dict(N=N, K=K, xyz=p["xyz"], features_dc=p["features_dc"], features_rest=p["features_rest"],
                        m_dc=np.zeros_like(p["features_dc"]), v_dc=np.zeros_like(p["features_dc"]),
                        m_rest=np.zeros_like(p["features_rest"]), v_rest=np.zeros_like(p["features_rest"])), r.device)
    xyz_add = _xyz_add_buffer(N, r.device)
    accum = torch.zeros(N, device=r.device)
    try:
        r.setGradNormAccum(accum)
        r.shGradFromViewsAdamDir(model.getParams(), cc_all, centres, owns, model.arena, model.m, model.v, LR_DC, LR_REST, 1.0, xyz_add)
    finally:
        r.setGradNormAccum(None)
    total = _np(sum_geom_xyz).astype(np.float64) + _np(xyz_add)[:3 * N].reshape(N, 3)
    worst("summed_xyz", _rel(total, sums["xyz"]) / GRAD_RTOL)
    _record("views_" + config, dict(shares, left_out=left_out))
    for k, s in shares.items():
        assert s <= 1.0, (k, s)


def test_zero_raw_quaternion_leaves_the_same_pattern_in_every_backward_form(renderer_of, oracle32):
    """A visible and an invisible Gaussian whose raw quaternion is exactly zero: the normalisation's VJP divides by |q| = 0 in
    proj_bwd_geom_kernel and in the fused body alike.  Every data-parallel form must leave the finite / non-finite pattern
    gs_render_backward leaves on those rows, every other row finite and within the bars.  The oracle (float32) gives NaN in all
    four rotation entries of such a row, visible or not (0 x inf), and finite values everywhere else."""
    p, cams, W, H = dn.e2e_scene()
    p = {k: v.copy() for k, v in p.items()}
    N, cam = p["xyz"].shape[0], cams[0]
    r = renderer_of(4, W, H)
    rng = np.random.default_rng(11)
    cC = rng.normal(0, 1, (W * H, 3)).astype(np.float32)
    z = np.zeros(W * H, np.float32)
    tC = _dev(cC.reshape(H, W, 3), r.device)
    res = r.renderForward({k: _dev(v, r.device) for k, v in p.items()}, cam, want_radii=True)
    radii = _np(res.radii)
    pull = np.abs(_np(r.renderBackward(tC)["rotation"])).sum(1)       # the visible one: the row the blend pulls hardest on
    vis, inv = int(np.argmax(pull)), int(np.flatnonzero(radii == 0)[0])
    assert radii[vis] > 0 and pull[vis] > 0
    p["rotation"][[vis, inv]] = 0.0
    tp = {k: _dev(v, r.device) for k, v in p.items()}
    fw, want = _oracle_view(oracle32, p, cam, W, H, (16, 16), False, (cC, z, z))
    oracle_rows = {k: want[k].reshape(N, -1)[[vis, inv]] for k in GEOM}
    assert fw["proj"]["radii"][vis] > 0 and fw["proj"]["radii"][inv] == 0
    forms = {}
    r.renderForward(tp, cam)
    forms["fused"] = {k: _np(v) for k, v in r.renderBackward(tC).items() if k in GEOM}
    r.renderForward(tp, cam)
    forms["dp"] = {k: _np(v) for k, v in r.renderBackwardDP(tC)[0].items()}
    r.renderForward(tp, cam)
    g = _geom_out(tp)
    cc = torch.empty(N, 3, device=r.device)
    r.renderBackwardDPGeom(tC, cc, g, torch.empty(N, 3, device=r.device))
    forms["dp_geom"] = {k: _np(v) for k, v in g.items()}
    r.renderForward(tp, cam)
    r.renderBackwardDPBegin(tC)
    g = _geom_out(tp)
    r.renderBackwardDPFinishGeom(g, torch.empty(N, 3, device=r.device))
    forms["two_halves"] = {k: _np(v) for k, v in g.items()}
    others = np.ones(N, bool)
    others[[vis, inv]] = False
    shares = {}
    for name, got in forms.items():
        for k in GEOM:
            a, f = got[k].reshape(N, -1), forms["fused"][k].reshape(N, -1)
            assert np.array_equal(np.isfinite(a[[vis, inv]]), np.isfinite(f[[vis, inv]])), (name, k)
            assert np.isfinite(a[others]).all(), (name, k)
            if k != "xyz" or name in ("fused", "dp"):          # (the geometry forms' xyz lacks the view-direction term)
                shares[f"{name}_{k}"] = _rel(a[others], want[k].reshape(N, -1)[others]) / GRAD_RTOL
    assert np.isfinite(_np(cc)).all()
    _record("zero_quaternion", dict(shares, oracle_rows={k: np.array2string(v) for k, v in oracle_rows.items()},
                                    fused_rows={k: np.array2string(forms["fused"][k].reshape(N, -1)[[vis, inv]]) for k in GEOM}))
    for k, s in shares.items():
        assert s <= 1.0, (k, s)
