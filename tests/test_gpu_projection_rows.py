"""The pinhole projection kernels, every row against float64, on the edge-case cloud of tests/projection_numpy.py.

project_geometry, project_geometry_bwd (csrc/gs_math.h) and color_backward (csrc/projection.hip) are the arithmetic under every
render and every train step.  tests/test_gpu_parity.py::test_projection_forward_backward feeds them prescribed cotangents on one
cloud whose depths all lie beyond the EWA clamp's limits, against the float32 oracle at atol = 2e-5 max|tensor|; the rendered
scenes reach the other branches only through the blend's float atomics at 1e-3 max|tensor|.  Here the cloud (631 Gaussians in
twelve groups: far, inside_clamp, between_lims, near_plane, behind, plane_zero, offscreen, needle, isotropic, tiny_q, big_q,
subpixel) sits on both sides of every branch, and the measure is per Gaussian: row_error = max|got - want| / max|want| over one
row, nothing taken from the tensor's largest entry.

a. op level (gs_projection_forward / gs_projection_backward: proj_fwd_op_kernel, proj_bwd_op_kernel), the cloud and its first
   1, 63 and 257 rows, (K, degree) = (25, 4), (25, 2), (16, 3), (9, 2), (4, 1), (1, 0), activations from the float32 oracle:
   means2d, depths, rects and radii bit-equal to the float32 oracle; colour, cov2d, conic and the five gradients row-wise against
   float64 at 2e-4 (the project's rtol for these tensors; tests/test_projection_numpy_cpu.py qualifies it: the float32 oracle
   uses at most half, and no (tensor, group) needed the 4 x rule); isotropic gradRot absolutely, at 4 x 2^-11; gradShs exactly
   zero beyond (degree + 1)^2; plane_zero by the float32 oracle's finite / non-finite pattern.
b. fused forward on raw parameters (gs_render_forward, K = 25: two-phase SH staging, K = 16: whole rows; the last wave partial):
   radii equal the float32 oracle's (a row is exempt only with its float64 sqrt(lambdaMax) within 1e-4 of an integer; none is),
   visibility() is radii > 0, stats()["N_visible"] agrees, and GS_DEGENERATE_INVISIBLE touches no row of this cloud.
c. fused backward (gs_render_backward) under a seeded normal cotangent image: everything finite; the rows the float64 oracle's
   backward leaves untouched (all of behind and plane_zero, most of offscreen, what the close-ups hide) exactly zero in all six
   tensors; the touched rows under test_gpu_parity._elementwise_gradient_bar, imported and unchanged.

Worst row error over the op-level cases as a share of its bar (1.0 = the whole bar), per tensor with its worst group; beside it
the float32 oracle's share on the same inputs (the qualification, which may use 0.5):
  tensor               MI355X vs float64         float32 oracle vs float64
  color                0.14   far                0.14   far
  cov2d                0.017  near_plane         0.017  near_plane
  conic                0.077  needle             0.077  needle
  gradScales           0.041  needle             0.041  needle
  gradRot              0.055  subpixel           0.055  subpixel
  gradRot, isotropic   0.25   (absolute)         0.25
  gradMeans3d          0.044  behind             0.044  behind
  gradShs              0.0019 tiny_q             0.0019 tiny_q
  gradCamCenterPoint   0.0074 near_plane         0.0074 near_plane
-- the kernels sit exactly at the float32 oracle's shares: the same operations in the same order, without FMA contraction.
Fused forward: radii equal on all 631 rows (549 visible), no row exempt.  Fused backward, 405 touched rows, share of elements
beyond 1e-3 (floored), MI355X vs float32 oracle / float32 vs float64 oracle (the bar is 1.5 x the second + 5e-4):
  K = 25   xyz 0 / 0.021   features_dc 0.0008 / 0.012   features_rest 0 / 0.0042   scales 0 / 0.011   rotation 0.0006 / 0.0019
           opacity 0.0025 / 0.022
  K = 16   xyz 0.035 / 0.030   features_dc 0.0008 / 0.012   features_rest 0.0002 / 0.012   scales 0.0082 / 0.020
           rotation 0.0019 / 0.0031   opacity 0.022 / 0.025
Row by row against float64, 9 to 23 % of the touched rows of a tensor lie beyond 1e-3 of their own magnitude on the card and 6 to
15 % in the float32 oracle; with the projection itself within 3e-5 of a row (a), that is the blend's float32 sums over pixels.

What the file catches, on scratch builds with one line changed (never committed):
  `dt2 += dclipX` dropped (gs_math.h)           a: gradMeans3d of inside_clamp, between_lims, near_plane and behind at 1100 to
                                                1900 bars; c: xyz, 24 % of the elements beyond against the pair's 2 %
  cam.limX in the Y condition (gs_math.h)       a: gradMeans3d of between_lims at 1594 bars, of behind at 97; c: xyz, 6.7 %
  `+ 2.0f * rr[a] * dn2` dropped from the fused body's quaternion VJP (projection.hip): not in a (the op level never runs it),
    and c passes with every share unchanged.  project_geometry_bwd normalises the quaternion once more, so the gradient it
    returns is orthogonal to q and the dropped term is rounding alone: no bar on the fused output can see it.
With GSPLAT_TEST_REPORTS=<directory> in the environment every case writes its shares to <directory>/projection_rows_<case>.json.
"""
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
    spec = importlib.util.spec_from_file_location("_prr_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pn = _load("projection_numpy")
W, H = pn.W, pn.H
FUSED = ((25, 4), (16, 3))
GRAD_KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
BIT_EQUAL = ("means2d", "depths", "rectMin", "rectMax", "radii")


def _np(t):
    return t.detach().cpu().numpy()


def _id(case):
    return "K%d_deg%d" % case


def _record(case, shares):
    """Worst observed share of every bar of a case: printed, and kept as a file where GSPLAT_TEST_REPORTS names a directory
    (never fails the test)."""
    flat = {("%s/%s" % k if isinstance(k, tuple) else k): v for k, v in shares.items()}
    out = os.environ.get("GSPLAT_TEST_REPORTS")
    if out:
        try:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, f"projection_rows_{case}.json"), "w") as f:
                json.dump(flat, f, indent=1, sort_keys=True)
        except OSError:
            pass
    print("projection_rows", case, " ".join(f"{k}={v:.3g}" for k, v in flat.items() if isinstance(v, float)))


@pytest.fixture(scope="module")
def renderer_of():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    made = {}

    def get(degree):
        if degree not in made:
            made[degree] = GaussianRenderer(degree, W, H, (16, 16), False)
        return made[degree]

    yield get
    for r in made.values():
        r.close()


@functools.lru_cache(maxsize=None)
def _oracles():
    from oracle.oracle import Oracle
    return Oracle(np.float32), Oracle(np.float64)


@functools.lru_cache(maxsize=None)
def _ref(case):
    """A (K, degree)'s cloud, the float32 oracle's activations and both oracles' walks from them, computed once and shared
    (read only).  Rows are independent: the first n rows of a walk are the walk of the first n rows."""
    K, degree = case
    o32, o64 = _oracles()
    p, groups, cam, cots = pn.edge_cloud(pn.SEED, K)
    _, sc, rt = o32.activations_forward(p["opacity"], p["scales"], p["rotation"])
    f32, b32 = pn.walk(o32, sc, rt, p, cam, cots, degree)
    f64, b64 = pn.walk(o64, sc, rt, p, cam, cots, degree)
    pn.assert_cloud_does_its_job(p, groups, cam, f64, sc, degree)
    return dict(p=p, groups=groups, cam=cam, cots=cots, sc=sc, rt=rt, f32=f32, b32=b32, f64=f64, b64=b64)


def _same_pattern(got, want, rows):
    got, want = np.asarray(got), np.asarray(want)
    n = got.shape[0]
    return np.array_equal(np.isfinite(got.reshape(n, -1)[rows]), np.isfinite(want.reshape(n, -1)[rows]))


# ------------------------------------------------------------------------------------------------------------------ a. op level
@pytest.mark.parametrize("rows", [1, 63, 257, pn.N_TOTAL])
@pytest.mark.parametrize("case", pn.CASES, ids=_id)
def test_op_level_rows_against_float64(renderer_of, case, rows):
    K, degree = case
    ref = _ref(case)
    p, groups, cots, n = ref["p"], ref["groups"][:rows], ref["cots"], rows
    r = renderer_of(degree)
    c = ref["cam"].as_dict()
    gcam = r._camera(c["view"], c["proj"], c["camCenter"], c["fovX"], c["fovY"], c["focalX"], c["focalY"])
    shs = pn.shs_of(p)
    args = (ref["sc"][:n], ref["rt"][:n], p["xyz"][:n], shs[:n], gcam)
    got = {k: _np(v) for k, v in r.projectionScreenFused(*args).items()}
    # mean / depth / rect / radius arithmetic is compiled without FMA contraction: the float32 oracle's bits, on every row
    for k in BIT_EQUAL:
        np.testing.assert_array_equal(got[k], ref["f32"][k][:n], err_msg=k)
    gb = r.projectionScreenFusedVJP(*args, cots["means2d"][:n], cots["depths"][:n], cots["color"][:n], cots["cov2d"][:n],
                                    cots["conic"][:n])
    got.update({k: _np(gb[k]) for k in pn.BACKWARD})
    want = {k: v[:n] for k, v in dict(ref["f64"], **ref["b64"]).items()}
    tensors = pn.FORWARD_ROWWISE + pn.BACKWARD
    shares = pn.bar_shares(got, want, groups, tensors)
    assert len(shares) == len(tensors) * len(set(groups) - {"plane_zero"})
    _record(f"op_{_id(case)}_rows{n}", {k: s for k, (s, _) in shares.items()})
    for (t, g), (s, row) in shares.items():
        assert s <= 1.0, (t, g, row, s)
    coeff = (degree + 1) ** 2
    assert got["gradShs"].shape == (n, K, 3) and not got["gradShs"][:, coeff:, :].any()
    if degree > 0 and n > 1:
        assert np.abs(got["gradShs"][:, 1:coeff, :]).max() > 0
    # plane_zero: the op level keeps the reference's 1:1 arithmetic, 0 x inf included
    pz = np.flatnonzero(groups == "plane_zero")
    if pz.size:
        both32 = dict(ref["f32"], **ref["b32"])
        for t in tensors:
            assert _same_pattern(got[t], both32[t][:n], pz), t
        assert not got["radii"][pz].any()
        assert not all(np.isfinite(got[t][pz]).all() for t in pn.BACKWARD)         # (the region does overflow in float32)
    else:
        assert all(np.isfinite(got[t]).all() for t in tensors)


# ----------------------------------------------------------------------------------------------- b. fused forward, raw parameters
@functools.lru_cache(maxsize=None)
def _fused_ref(case):
    """The raw cloud through both oracles' whole chains (own activations, own forward) and a seeded normal cotangent image."""
    K, degree = case
    o32, o64 = _oracles()
    p, groups, cam, _ = pn.edge_cloud(pn.SEED, K)
    c = cam.as_dict()
    cot = np.random.default_rng(17).normal(0, 1, (W * H, 3)).astype(np.float32)
    z = np.zeros(W * H)
    out = dict(p=p, groups=groups, cam=cam, c=c, cot=cot)
    with np.errstate(all="ignore"):
        for name, o in (("32", o32), ("64", o64)):
            pp = {k: np.asarray(v, o.dtype) for k, v in p.items()}
            fw = o.render_forward(pp, c, W, H, 16, 16, degree)
            out["fw" + name] = fw
            out["bw" + name] = o.render_backward(pp, c, W, H, 16, 16, degree, fw, cot.astype(o.dtype), z.astype(o.dtype), z.astype(o.dtype))
    return out


@pytest.mark.parametrize("case", FUSED, ids=_id)
def test_fused_forward_radii_and_visibility(renderer_of, case):
    K, degree = case
    ref = _fused_ref(case)
    p, groups, N = ref["p"], ref["groups"], pn.N_TOTAL
    assert N % 64 != 0                                               # the last wave is partial
    want = ref["fw32"]["proj"]["radii"]
    exempt = pn.near_integer_sqrt_lambda(ref["fw64"]["proj"])
    assert exempt.mean() <= 0.01
    # the fused path's deliberate deviation (a covariance that is not positive definite is invisible) concerns no row here:
    # the float32 determinant, formed as the kernel forms it, is positive on every row the oracle gives a radius
    c2 = ref["fw32"]["proj"]["cov2d"].reshape(N, 4).astype(np.float32)
    with np.errstate(all="ignore"):                                  # (plane_zero's entries overflow; it has no radius)
        det = c2[:, 0] * c2[:, 3] - c2[:, 1] * c2[:, 2]
    assert det.dtype == np.float32 and (det[want > 0] > 0).all()
    r = renderer_of(degree)
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in p.items()}
    try:
        for sparse in (False, True):
            r.setSparseAdam(sparse)
            res = r.renderForward(tp, ref["cam"], want_radii=True)
            got = _np(res.radii)
            assert got.shape == (N,)
            same = got == want
            assert same[~exempt].all(), (sparse, np.flatnonzero(~same & ~exempt), groups[~same & ~exempt])
            r.sync()
            assert r.stats()["N_visible"] == int((got > 0).sum())
            assert 0 < int((got > 0).sum()) < N
            if sparse:
                vis = _np(r.visibility())
                assert vis.dtype == np.bool_ and np.array_equal(vis, got > 0)
            for g in ("behind", "plane_zero"):
                assert not got[pn.group_rows(groups, g)].any(), g
    finally:
        r.setSparseAdam(False)
    _record(f"fused_forward_{_id(case)}", dict(differing=float((~same).sum()), exempt=float(exempt.sum()), visible=float((got > 0).sum())))


# --------------------------------------------------------------------------------------------------------- c. fused backward
class _TouchedRows64:
    """The float64 oracle as _elementwise_gradient_bar calls it, at the case's SH degree (the helper names degree 4) and with
    the gradients cut to the given rows, so that the shares are taken over the touched rows alone."""

    def __init__(self, o64, degree, rows):
        self.o, self.degree, self.rows = o64, degree, rows

    def render_forward(self, p, c, w, h, tw, th, _degree, *a):
        return self.o.render_forward(p, c, w, h, tw, th, self.degree, *a)

    def render_backward(self, p, c, w, h, tw, th, _degree, *a):
        with np.errstate(all="ignore"):
            g = self.o.render_backward(p, c, w, h, tw, th, self.degree, *a)
        return {k: v.reshape(v.shape[0], -1)[self.rows] for k, v in g.items() if k in GRAD_KEYS}


@pytest.mark.parametrize("case", FUSED, ids=_id)
def test_fused_backward_zero_rows_and_elementwise_bar(renderer_of, case):
    from tests.test_gpu_parity import _elementwise_gradient_bar
    K, degree = case
    ref = _fused_ref(case)
    p, groups, N = ref["p"], ref["groups"], pn.N_TOTAL
    untouched = ~ref["bw64"]["gradPacked"].any(1)
    for g in ("behind", "plane_zero"):
        assert untouched[pn.group_rows(groups, g)].all(), g
    assert untouched[pn.group_rows(groups, "offscreen")].mean() > 0.5
    assert 0.2 * N < (~untouched).sum() < N
    r = renderer_of(degree)
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in p.items()}
    r.renderForward(tp, ref["cam"])
    got = {k: _np(v).reshape(N, -1) for k, v in r.renderBackward(torch.as_tensor(ref["cot"].reshape(H, W, 3), device=r.device)).items()}
    for k in GRAD_KEYS:
        assert np.isfinite(got[k]).all(), k
        # the zero-row rule of the fused body: a row no pixel blended leaves with an exactly zero gradient, at the camera plane too
        assert not got[k][untouched].any(), (k, groups[untouched & got[k].any(1)])
    rows = np.flatnonzero(~untouched)
    want32 = {k: ref["bw32"][k].reshape(N, -1)[rows] for k in GRAD_KEYS}
    assert all(np.isfinite(v).all() for v in want32.values())
    report = _elementwise_gradient_bar(f"projection_rows_{_id(case)}", {k: torch.as_tensor(got[k][rows]) for k in GRAD_KEYS}, want32,
                                       _TouchedRows64(_oracles()[1], degree, rows), p, ref["c"], W, H, None, cot_fixed=ref["cot"])
    shares = {}
    for k, v in report["tensors"].items():
        shares[k + "_hip_vs_32"], shares[k + "_32_vs_64"] = v["hip_vs_oracle32"], v["oracle32_vs_oracle64"]
        e = pn.row_error(got[k][rows], ref["bw64"][k].reshape(N, -1)[rows])
        shares[k + "_rows_beyond_1e-3"] = float((e > 1e-3).mean())
    _record(f"fused_backward_{_id(case)}", dict(shares, touched=float(rows.size)))
