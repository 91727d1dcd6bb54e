"""Qualifies the edge-case cloud and the row-wise bars of tests/projection_numpy.py without a GPU: the float32 oracle walks the
cloud against the float64 oracle, both from the float32 oracle's activations (the same bits, as in the op-level GPU test).

  the cloud does its job: every group sits where it is meant to sit (assert_cloud_does_its_job), for every (K, degree);
  forward: radii (and with them visibility) are equal on every row; a row is exempt only if its float64 sqrt(lambdaMax) lies
    within 1e-4 of an integer, and at most 1 % of the rows may be (this seed: none);
  backward and colour / cov2d / conic: per tensor and group the float32 oracle's worst row error is at most HALF the bar the
    kernels are held to (2e-4 everywhere: BARS, the table of exceptions under the 4 x rule, is empty; no bar above 1e-3);
  plane_zero (|z| < 1e-4: 1 / tz^2 of the order of 1e8 and more) has no relative bar: radius 0 in both precisions, and its
    float64 rows finite; isotropic gradRot is held absolutely.

Worst row error of the float32 oracle over the (K, degree) pairs and degrees 0 .. 4 at K = 25, per tensor (its worst group):
  color 2.7e-5 (far)  cov2d 3.5e-6 (near_plane)  conic 1.5e-5 (needle)  gradScales 8.3e-6 (needle)  gradRot 1.1e-5 (subpixel)
  gradMeans3d 8.9e-6 (behind)  gradShs 3.8e-7 (tiny_q)  gradCamCenterPoint 1.5e-6 (near_plane)
-- every one below a seventh of 2e-4, and the same to two digits when each oracle activates the raw parameters itself.  The
test prints the whole table.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_prc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pn = _load("projection_numpy")
WALKS = pn.CASES + tuple((25, d) for d in (3, 1, 0))          # the listed pairs, and degrees 0 .. 4 at K = 25


@functools.lru_cache(maxsize=None)
def _walks(case):
    """(cloud, activated scales, float32 walk, float64 walk) of a (K, degree), computed once and shared (read only)."""
    from oracle.oracle import Oracle
    K, degree = case
    cloud = pn.edge_cloud(pn.SEED, K)
    p, groups, cam, cots = cloud
    _, sc, rt = Oracle(np.float32).activations_forward(p["opacity"], p["scales"], p["rotation"])
    return cloud, sc, pn.walk(Oracle(np.float32), sc, rt, p, cam, cots, degree), pn.walk(Oracle(np.float64), sc, rt, p, cam, cots, degree)


def _id(case):
    return "K%d_deg%d" % case


def test_row_error_is_per_row_and_takes_nothing_from_the_tensor():
    want = np.array([[100.0, -50.0], [1e-3, 2e-3], [0.0, 0.0], [0.0, 0.0]])
    got = want + np.array([[1e-2, 0.0], [0.0, 1e-4], [0.0, 0.0], [0.0, 1e-30]])
    e = pn.row_error(got, want)
    np.testing.assert_allclose(e[:2], [1e-4, 0.05], rtol=1e-9)
    assert e[2] == 0 and e[3] == np.inf
    # the max-norm measure of the same pair: blind to the second row
    assert np.abs(got - want).max() / np.abs(want).max() == pytest.approx(1e-4)
    w = pn.worst_by_group(got, want, np.array(["a", "a", "b", "b"]))
    assert w["a"] == (pytest.approx(0.05), 1) and w["b"] == (np.inf, 3)


def test_cloud_layout():
    p, groups, cam, cots = pn.edge_cloud(pn.SEED, 25)
    N = p["xyz"].shape[0]
    assert N == pn.N_TOTAL == 631 and N % 64 != 0 and N % 128 != 0
    starts = np.cumsum([0] + [n for _, n in pn.GROUPS])
    assert sum(1 for s in starts[1:-1] if s % 64 == 0) == 0            # every group boundary lies inside a wave
    assert (cam.imageWidth, cam.imageHeight) == (200, 152) and float(cam.focalX) == pytest.approx(180.0)
    limX, limY = pn.limits(cam)
    assert limX == pytest.approx(0.7222, abs=1e-4) and limY == pytest.approx(0.5381, abs=1e-4)
    for k, v in p.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    p16 = pn.edge_cloud(pn.SEED, 16)[0]
    for k in ("xyz", "scales", "rotation", "opacity", "features_dc"):
        assert np.array_equal(p[k], p16[k]), k
    assert np.array_equal(p["features_rest"][:, :15], p16["features_rest"])
    again = pn.edge_cloud(pn.SEED, 25)
    assert all(np.array_equal(p[k], again[0][k]) for k in p) and all(np.array_equal(cots[k], again[3][k]) for k in cots)


@pytest.mark.parametrize("case", WALKS, ids=_id)
def test_cloud_does_its_job(case):
    (p, groups, cam, cots), sc, (f32, b32), (f64, b64) = _walks(case)
    info = pn.assert_cloud_does_its_job(p, groups, cam, f64, sc, case[1])
    print("projection_rows cloud", _id(case), info)
    if case[1] == 4:
        assert 0.25 <= info["colour_channels_at_zero"] <= 0.45          # "a third"


@pytest.mark.parametrize("case", WALKS, ids=_id)
def test_radii_and_visibility_are_equal_in_both_precisions(case):
    (p, groups, cam, cots), sc, (f32, b32), (f64, b64) = _walks(case)
    exempt = pn.near_integer_sqrt_lambda(f64)
    assert exempt.mean() <= 0.01, int(exempt.sum())
    same = f32["radii"].astype(np.float64) == f64["radii"]
    assert same[~exempt].all(), np.flatnonzero(~same & ~exempt)
    assert np.array_equal((f32["radii"] > 0)[~exempt], (f64["radii"] > 0)[~exempt])
    print("projection_rows radii", _id(case), "exempt rows", int(exempt.sum()), "differing", int((~same).sum()))


def test_no_bar_above_the_cap_and_none_below_the_projects_rtol():
    names = [g for g, _ in pn.GROUPS]
    for (t, g), b in pn.BARS.items():
        assert t in pn.FORWARD_ROWWISE + pn.BACKWARD and g in names and g != "plane_zero"
        assert pn.RTOL < b <= pn.CAP, (t, g, b)
    assert pn.bar("gradRot", "far") == 2e-4 and pn.CAP == 1e-3


@pytest.mark.parametrize("case", WALKS, ids=_id)
def test_float32_oracle_stays_within_half_of_every_bar(case):
    (p, groups, cam, cots), sc, (f32, b32), (f64, b64) = _walks(case)
    got, want = dict(f32, **b32), dict(f64, **b64)
    shares = pn.bar_shares(got, want, groups, pn.FORWARD_ROWWISE + pn.BACKWARD)
    for t in pn.FORWARD_ROWWISE + pn.BACKWARD:
        print("projection_rows float32_vs_float64", _id(case), t,
              " ".join("%s=%.3g" % (g, s * (pn.ISOTROPIC_GRADROT_ABS if (t, g) == ("gradRot", "isotropic") else pn.bar(t, g)))
                       for (tt, g), (s, _) in shares.items() if tt == t))
    assert len(shares) == 8 * (len(pn.GROUPS) - 1)
    for (t, g), (s, row) in shares.items():
        assert s <= 0.5, (t, g, row, s)
        # a bar under the 4 x rule is four times the worst error, not more: it may not sit idle above what it was made for
        if (t, g) in pn.BARS:
            assert s >= 0.125 or case != pn.CASES[0], (t, g, s)
    coeff = (case[1] + 1) ** 2
    assert not b32["gradShs"][:, coeff:].any() and not b64["gradShs"][:, coeff:].any()
    # the isotropic group's gradRot is rounding alone: in float64 it vanishes against every other group's
    iso = pn.group_rows(groups, "isotropic")
    assert np.abs(b64["gradRot"][iso]).max() < 1e-9 * np.median(np.abs(b64["gradRot"]).max(1))
    assert np.abs(b32["gradRot"][iso]).max() <= pn.ISOTROPIC_GRADROT_ABS / 4


def test_max_norm_bar_is_blind_on_this_cloud():
    """Why the measure is per row: an error of 3 % of its own row on every Gaussian of the cloud's quieter half passes the
    suite's max-norm gradient bar (1e-3 max|tensor|) in scales and rotations -- a close-up's row is that much larger."""
    (p, groups, cam, cots), sc, (f32, b32), (f64, b64) = _walks(pn.CASES[0])
    live = groups != "plane_zero"
    for t in ("gradScales", "gradRot"):
        w = b64[t][live]
        size = np.abs(w).max(1)
        quiet = size < np.median(size)
        off = w * np.where(quiet, 1.03, 1.0)[:, None]
        assert np.abs(off - w).max() / np.abs(w).max() < 1e-3, t
        assert np.nanmax(pn.row_error(off, w)) > 100 * pn.RTOL


def test_plane_zero_is_invisible_and_finite_in_float64():
    (p, groups, cam, cots), sc, (f32, b32), (f64, b64) = _walks(pn.CASES[0])
    rows = pn.group_rows(groups, "plane_zero")
    assert not f32["radii"][rows].any() and not f64["radii"][rows].any()
    assert np.abs(f64["depths"][rows]).max() < 2e-4
    for t in pn.BACKWARD:
        assert np.isfinite(b64[t][rows]).all(), t
    # the two precisions disagree wholesale here, as they should (1 / tz^4 times differences of rounded products)
    e = pn.row_error(b32["gradMeans3d"][rows], b64["gradMeans3d"][rows])
    print("projection_rows plane_zero float32 non-finite elements",
          {t: int((~np.isfinite(b32[t][rows])).sum()) for t in pn.BACKWARD}, "median row error gradMeans3d", float(np.nanmedian(e)))
    assert np.isfinite(b32["gradShs"][rows]).all() and np.isfinite(b32["gradCamCenterPoint"][rows]).all()
