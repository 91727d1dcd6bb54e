"""Pins tests/dp_numpy.py -- the float64 restatement of the data-parallel SH rebuild that tests/test_gpu_dp_kernels.py holds
the HIP kernels to -- against the oracle, and qualifies that file's op-level inputs.  Runs without a GPU.

Pins, on the 300-Gaussian scene and two of the cameras of tests/test_data_parallel_cpu.py:
  the restated SH gradient from cc = grad_features_dc / basis_0, summed over the views, equals the oracle's summed SH gradients
    (bars of test_sh_gradient_is_rank_one_in_colour_cotangent);
  the oracle's xyz gradient equals its geometry part (projection_backward with a zero colour cotangent) plus the restated
    view-direction term d_r, in float64 at rtol 1e-6 (atol 1e-8 max|want|: the central difference's rounding error,
    2^-53 |b| / h = 1e-10 |b| per basis value against gradients of order |b| / |direction|, summed over 24 bands).

Qualification: for every op-level input set of the GPU file the float32 walk of the restatement (the kernels' summation order)
must stay within HALF of the bar the kernels are held to against the float64 one -- rtol 2e-4, atol 2e-5 max|want| for the SH
gradient, xyz_add and the densify statistic.  Worst share of the bar (1.0 = the whole bar; 0.5 allowed) over the cases:
  SH gradient    0.0043  (N129_R16_K16_deg3)
  xyz_add        0.0067  (N129_R3_K25_deg4)
  statistic      0.0013  (N333_R16_K25_deg4)
per case: see test_float32_restatement_stays_within_half_of_the_bars (it prints the three shares of every case).
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_dpn_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dn = _load("dp_numpy")
dpc = _load("test_data_parallel_cpu")


def _view(o, p, cam, W=64, H=48):
    c = cam.as_dict()
    fw = o.render_forward(p, c, W, H, 16, 16, 4)
    tgt = np.full((H, W, 3), 0.3, o.dtype)
    _, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), tgt, 0.2)
    z = np.zeros(W * H, o.dtype)
    return c, fw, o.render_backward(p, c, W, H, 16, 16, 4, fw, cot.reshape(-1, 3), z, z)


def test_restated_sh_gradient_sums_to_the_oracles(oracle32, oracle64):
    p, cams = dpc._scene()
    cams = cams[:2]
    centres = np.stack([c.cameraCenter for c in cams]).astype(np.float32)
    b, _ = dn.basis64(oracle64, 4, p["xyz"], centres)
    total_dc, total_rest, cc = 0, 0, []
    for v, cam in enumerate(cams):
        g = _view(oracle32, p, cam)[2]
        gdc = g["features_dc"].reshape(-1, 3).astype(np.float64)
        total_dc, total_rest = total_dc + gdc, total_rest + g["features_rest"].astype(np.float64)
        cc.append(gdc / b[v][:, :1])
    got_dc, got_rest = dn.sh_grad(b, np.stack(cc), 25)
    assert np.abs(total_rest).max() > 0
    np.testing.assert_allclose(got_dc.reshape(-1, 3), total_dc, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(got_rest, total_rest, rtol=2e-5, atol=1e-6 * np.abs(total_rest).max())


def test_oracle_xyz_gradient_is_geometry_plus_restated_direction_term(oracle64):
    o = oracle64
    p, cams = dpc._scene()
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    for cam in cams[:2]:
        c, fw, g = _view(o, p64, cam)
        centre = np.asarray(c["camCenter"], np.float64).reshape(1, 3)
        # (float64 directions: the oracle's own, not the float32 ones the kernels form)
        d64 = p64["xyz"] - centre
        b = dn._basis_rows(o, 4, d64)[None]
        gb = np.zeros((1, len(d64), 25, 3))
        for a in range(3):
            e = np.zeros(3)
            e[a] = dn.FD_H
            gb[0, :, :, a] = (dn._basis_rows(o, 4, d64 + e) - dn._basis_rows(o, 4, d64 - e)) / (2 * dn.FD_H)
        cc = (g["features_dc"].reshape(-1, 3) / b[0][:, :1])[None]
        gp, N = g["gradPacked"], len(d64)
        geom = o.projection_backward(fw["scales"], fw["rot"], p64["xyz"], fw["shs"], c["camCenter"], c["view"], c["proj"],
                                     c["fovX"], c["fovY"], c["focalX"], c["focalY"], 64, 48, 4, gp[:, 10], gp[:, 0:2],
                                     np.zeros((N, 4)), np.zeros((N, 3)), gp[:, 2:6])["gradMeans3d"]
        d = dn.dir_terms(gb, cc, p64["features_rest"])[0]
        assert np.abs(d).max() > 1e-3 * np.abs(g["xyz"]).max()           # (the term is not negligible on this scene)
        np.testing.assert_allclose(geom + d, g["xyz"], rtol=1e-6, atol=1e-8 * np.abs(g["xyz"]).max())


def test_case_list_covers_what_the_kernels_branch_on():
    cases = dn.OP_CASES
    for N in dn.NS:
        assert {(25, 4), (16, 3)} <= {(K, d) for n, R, K, d in cases if n == N}, N
    for N in (129, 333):
        assert set(dn.KD) <= {(K, d) for n, R, K, d in cases if n == N}, N
        for K in (25, 16):
            assert set(dn.RS) <= {R for n, R, k, d in cases if n == N and k == K}, (N, K)
    assert len(set(cases)) == len(cases)
    inp = dn.op_inputs(333, 3, 25, 4)
    zero = (inp["cc"] == 0).all(-1)
    part = (inp["cc"] == 0).any(-1) & ~zero
    assert 0.2 < zero.mean() < 0.4 and part.mean() > 0.1
    assert np.allclose(np.linalg.norm(inp["centres"][:, :2], axis=1), 3.0)


def test_end_to_end_scene_has_few_colours_between_zero_and_the_cap(oracle32):
    """The per-view GPU test expects the colour cotangent g where the oracle's clamped colour is > 1e-5 and 0 where it is exactly
    0, and leaves out the channel entries in between: at most 1e-3 of them may be.  Some Gaussians are invisible in every view."""
    p, cams, W, H = dn.e2e_scene()
    op, sc, rt = oracle32.activations_forward(p["opacity"], p["scales"], p["rotation"])
    shs = np.concatenate([p["features_dc"], p["features_rest"]], 1)
    for cam in cams:
        c = cam.as_dict()
        pr = oracle32.projection_forward(sc, rt, p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"],
                                         c["focalX"], c["focalY"], W, H, 4)
        col = pr["color"]
        assert ((col > 0) & (col <= 1e-5)).mean() <= 1e-3
        assert (col == 0).mean() > 0.05 and (col > 1e-5).mean() > 0.05
        assert 0 < (pr["radii"] == 0).sum() < len(col) // 2


@pytest.mark.parametrize("case", dn.ALL_CASES, ids=dn.case_id)
def test_float32_restatement_stays_within_half_of_the_bars(oracle32, oracle64, case):
    N, R, K, degree = case
    inp = dn.op_inputs(*case)
    b, gb = dn.basis64(oracle64, degree, inp["xyz"], inp["centres"])
    b32 = dn.basis32(oracle32, degree, inp["xyz"], inp["centres"])
    dc, rest = dn.sh_grad(b, inp["cc"], K)
    dc32, rest32 = dn.sh_grad32(b32, inp["cc"], K)
    d, d32 = dn.dir_terms(gb, inp["cc"], inp["features_rest"]), dn.dir_terms32(gb, inp["cc"], inp["features_rest"])
    views = tuple(range(R))
    shares = dict(sh=max(dn.max_bar_ratio(dc32, dc), dn.max_bar_ratio(rest32, rest)),
                  xyz_add=dn.max_bar_ratio(dn.xyz_add32(d32), d.sum(0)),
                  stat=dn.max_bar_ratio(dn.statistic32(d32, inp["own"], views), dn.statistic(d, inp["own"], views)))
    print("qualification", dn.case_id(case), " ".join(f"{k}={v:.4f}" for k, v in shares.items()))
    if K > (degree + 1) ** 2:
        assert not rest[:, (degree + 1) ** 2 - 1:, :].any()
    for k, v in shares.items():
        assert v <= 0.5, (k, v)
