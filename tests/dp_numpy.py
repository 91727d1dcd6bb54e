"""A numpy restatement of the data-parallel SH rebuild (include/gsplat.h gs_sh_grad_from_views, gs_sh_grad_from_views_adam,
gs_sh_grad_from_views_adam_dir), for tests/test_dp_numpy_cpu.py and tests/test_gpu_dp_kernels.py.

From the R views' gathered colour cotangents cc[R,N,3] (after the max(., 0) gate) and camera centres, with b_k the SH basis
of the oracle (oracle.sh_basis, direction xyz - centre NOT normalised):
  grad_sh[n,k,:] = sum_r b_k(xyz_n - c_r) cc[r,n,:]                                  (zero for k >= (degree+1)^2)
  d[r,n,:]       = sum_{k>=1} grad b_k(xyz_n - c_r) sum_ch rest[n,k-1,ch] cc[r,n,ch]  (the xyz gradient's view-direction term)
  xyz_add        = sum_r d[r]
  stat[n]        = sum over the own views r of |own_r[n] + d[r,n]|_2                 (the densify statistic)
grad b_k is the central difference of the float64 sh_basis at h = 1e-6 (the oracle exposes no gradient hook): b_k is a
polynomial of degree <= 4 in a direction of length <= 5, so the truncation error h^2/6 |b'''| is below 1e-10 and the rounding
error 2^-53 |b| / h below 1e-7 |b| -- both far under the 2e-4 bars the restatement is used with.

The float32 variant walks the same sums in float32, in the kernels' order (views ascending, k ascending, the three channels
of d one after the other); it exists only to qualify inputs: a case whose float32 restatement is not within half a bar of the
float64 one cannot be asked of a float32 kernel at that bar.  Its grad b_k is the float64 one rounded to float32 (a central
difference has no float32 form).
"""
from __future__ import annotations

import zlib

import numpy as np

NS = (1, 63, 64, 65, 127, 128, 129, 333, 1000)        # wave = 64 rows, workgroup = 128
RS = (1, 3, 16)
KD = ((25, 4), (25, 2), (25, 0), (16, 3), (9, 2), (4, 1), (1, 0))
FD_H = 1e-6


def _op_cases():
    cases, i = [], 0
    for N in NS:                                       # every N meets K = 25 and K = 16
        for K, deg in ((25, 4), (16, 3)):
            for R in (RS if N in (129, 333) else (RS[i % 3],)):       # every R meets N = 129 and N = 333, at both K
                cases.append((N, R, K, deg))
            i += 1
    for N in (129, 333):                               # every (K, degree) meets N = 129 and N = 333
        for K, deg in KD:
            if (K, deg) not in ((25, 4), (16, 3)):
                cases.append((N, RS[i % 3], K, deg))
                i += 1
    return cases


OP_CASES = _op_cases()
# arena placements (features_rest at a float offset = 1, 2, 3 mod 4): K = 16 and K = 4 only, every access there is scalar or
# head / tail handled
PLACEMENT_CASES = [(N, 3, K, deg) for K, deg in ((16, 3), (4, 1)) for N in (1, 65, 129)]
GATE_CASE = (333, 3, 25, 4)
ALL_CASES = list(dict.fromkeys(OP_CASES + PLACEMENT_CASES + [GATE_CASE]))


def case_id(case):
    return "N%d_R%d_K%d_deg%d" % tuple(case)


def op_inputs(N, R, K, degree):
    """The synthetic inputs of one op-level case: cc ~ N(0,1) with about 30 % of the rows all zero and some rows zero in one
    or two channels, camera centres on a ring of radius 3, xyz ~ U(-1,1), features_rest ~ N(0, 0.3), moments m ~ N(0,1),
    v ~ U(0.01, 1), own-view tensors ~ N(0,1).  float32."""
    rng = np.random.default_rng(zlib.crc32(case_id((N, R, K, degree)).encode()))
    cc = rng.normal(0, 1, (R, N, 3))
    u = rng.uniform(size=(R, N))
    cc[u < 0.3] = 0.0
    one = (u >= 0.3) & (u < 0.4)                       # zero in one channel
    cc[one, rng.integers(0, 3, int(one.sum()))] = 0.0
    two = (u >= 0.4) & (u < 0.5)                       # zero in two channels
    keep = rng.integers(0, 3, int(two.sum()))
    rows = cc[two]
    kept = rows[np.arange(len(rows)), keep].copy()
    rows[:] = 0.0
    rows[np.arange(len(rows)), keep] = kept
    cc[two] = rows
    if not cc[:, 0].any():                             # (N = 1: the one row must not be skipped in every view)
        cc[0, 0] = (0.7, -1.1, 0.4)
    ang = 2 * np.pi * (np.arange(R) + 0.25) / R
    centres = np.stack([3 * np.cos(ang), 3 * np.sin(ang), 0.6 * np.cos(3 * ang)], 1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)        # noqa: E731
    return dict(N=N, R=R, K=K, degree=degree, cc=f32(cc), centres=f32(centres), xyz=f32(rng.uniform(-1, 1, (N, 3))),
                features_dc=f32(rng.normal(0, 1, (N, 1, 3))), features_rest=f32(rng.normal(0, 0.3, (N, K - 1, 3))),
                m_dc=f32(rng.normal(0, 1, (N, 1, 3))), v_dc=f32(rng.uniform(0.01, 1, (N, 1, 3))),
                m_rest=f32(rng.normal(0, 1, (N, K - 1, 3))), v_rest=f32(rng.uniform(0.01, 1, (N, K - 1, 3))),
                own=f32(rng.normal(0, 1, (R, N, 3))), accum=f32(rng.uniform(0, 2, N)))


def e2e_scene(N=3001, W=176, H=128, K=25, seed=71, spread=2.5, scale=0.05):
    """The rendered scene of the per-view end-to-end tests: test_gpu_parity._scene's cloud at spread 2.5 (some Gaussians are
    off screen or behind a camera) and the three cameras of test_sh_compressed_backward_matches_summed_view_gradients."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    rng = np.random.default_rng(seed)
    p = dict(xyz=rng.uniform(-spread, spread, (N, 3)), features_dc=rng.normal(0, 1, (N, 1, 3)),
             features_rest=rng.normal(0, 0.08, (N, K - 1, 3)), scales=rng.normal(np.log(scale), 0.5, (N, 3)),
             rotation=rng.normal(0, 1, (N, 4)), opacity=rng.normal(0.3, 1.5, N))
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    cams = [Camera(W, H, 0.9 * W, 0.9 * W * 1.02, look_at_c2w([2.2, -2.6, 1.7])),
            Camera(W, H, 0.8 * W, 0.8 * W, look_at_c2w([-2.4, 1.9, 1.2])),
            Camera(W, H, 1.1 * W, 1.1 * W, look_at_c2w([0.4, 2.9, -1.6]))]
    return p, cams, W, H


def own_patterns(R):
    """none, one, several and all of the R views."""
    pats = [(), (R // 2,), tuple(sorted({0, R // 2, R - 1})), tuple(range(R))]
    return list(dict.fromkeys(pats))


# ------------------------------------------------------------------------------------------------- basis and its gradient
def _basis_rows(o, degree, d):
    return np.stack([o.sh_basis(degree, *row) for row in d]) if len(d) else np.zeros((0, 25), o.dtype)


def basis64(o64, degree, xyz, centres):
    """b [R,N,25] and grad b [R,N,25,3] (central differences, h = 1e-6) in float64, of the float32 directions xyz - c_r as the
    kernels form them."""
    xyz, centres = np.asarray(xyz, np.float32), np.asarray(centres, np.float32)
    R, N = centres.shape[0], xyz.shape[0]
    b, g = np.zeros((R, N, 25)), np.zeros((R, N, 25, 3))
    for r in range(R):
        d = (xyz - centres[r][None, :]).astype(np.float64)
        b[r] = _basis_rows(o64, degree, d)
        for a in range(3):
            e = np.zeros(3)
            e[a] = FD_H
            g[r, :, :, a] = (_basis_rows(o64, degree, d + e) - _basis_rows(o64, degree, d - e)) / (2 * FD_H)
    return b, g


def basis32(o32, degree, xyz, centres):
    xyz, centres = np.asarray(xyz, np.float32), np.asarray(centres, np.float32)
    return np.stack([_basis_rows(o32, degree, xyz - centres[r][None, :]) for r in range(centres.shape[0])]).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- the restatement
def sh_grad(b, cc, K):
    """float64 (grad_dc [N,1,3], grad_rest [N,K-1,3]) from b [R,N,25]."""
    g = np.einsum("rnk,rnc->nkc", np.asarray(b, np.float64)[:, :, :K], np.asarray(cc, np.float64))
    return g[:, :1, :].copy(), g[:, 1:, :].copy()


def dir_terms(gb, cc, rest):
    """float64 d [R,N,3] from grad b [R,N,25,3] and features_rest [N,K-1,3]."""
    rest = np.asarray(rest, np.float64)
    K = rest.shape[1] + 1
    w = np.einsum("nkc,rnc->rnk", rest, np.asarray(cc, np.float64))            # sum_ch rest[n,k-1,ch] cc[r,n,ch]
    return np.einsum("rnka,rnk->rna", np.asarray(gb, np.float64)[:, :, 1:K, :], w)


def statistic(d, own, views):
    """sum over `views` of |own[r] + d[r]|_2: [N] float64."""
    s = np.zeros(d.shape[1])
    for r in views:
        s += np.sqrt(((np.asarray(own[r], np.float64) + d[r]) ** 2).sum(-1))
    return s


def sh_grad32(b32, cc, K):
    """The float32 walk of sh_grad: views ascending, k ascending, acc += b * g with both roundings."""
    cc = np.asarray(cc, np.float32)
    R, N = cc.shape[:2]
    g = np.zeros((N, K, 3), np.float32)
    for r in range(R):
        for k in range(K):
            g[:, k, :] = g[:, k, :] + b32[r][:, k, None] * cc[r]
    return g[:, :1, :].copy(), g[:, 1:, :].copy()


def dir_terms32(gb, cc, rest):
    """The float32 walk of dir_terms: per view, k ascending, the three channels' products added one after the other."""
    cc, rest, gb32 = np.asarray(cc, np.float32), np.asarray(rest, np.float32), np.asarray(gb, np.float64).astype(np.float32)
    R, N = cc.shape[:2]
    K = rest.shape[1] + 1
    d = np.zeros((R, N, 3), np.float32)
    for r in range(R):
        for k in range(1, K):
            for ch in range(3):
                w = rest[:, k - 1, ch] * cc[r][:, ch]
                d[r] = d[r] + gb32[r][:, k, :] * w[:, None]
    return d


def statistic32(d32, own, views):
    s = np.zeros(d32.shape[1], np.float32)
    for r in views:
        t = np.asarray(own[r], np.float32) + d32[r]
        s = s + np.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1] + t[:, 2] * t[:, 2])
    return s


def xyz_add32(d32):
    s = np.zeros(d32.shape[1:], np.float32)
    for r in range(d32.shape[0]):
        s = s + d32[r]
    return s


# ------------------------------------------------------------------------------------------------------------------- Adam
def adam32(p, m, v, g, lr, b1=0.9, b2=0.999, eps=1e-15, scale=1.0):
    """One float32 Adam step with the arithmetic of test_adam_step_matches_numpy: g * scale, (1 - beta) in float32,
    p - lr m / (sqrt(v) + eps); no bias correction.  Returns (p, m, v)."""
    f = np.float32
    p, m, v, g = (np.asarray(a, f) for a in (p, m, v, g))
    gs = g * f(scale)
    one = f(1)
    m = f(b1) * m + (one - f(b1)) * gs
    v = f(b2) * v + (one - f(b2)) * gs * gs
    p = p - f(lr) * m / (np.sqrt(v) + f(eps))
    return p, m, v


# ------------------------------------------------------------------------------------------------------------------- bars
def bar_ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): the share of an assert_allclose bar that is used (<= 1 passes)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def max_bar_ratio(got, want, rtol=2e-4, atol_rel=2e-5):
    """The project's bar for gradShs / gradMeans3d (test_projection_forward_backward): rtol 2e-4, atol 2e-5 max|want|."""
    want = np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    return bar_ratio(got, want, rtol, atol_rel * np.abs(want).max() + 1e-300)
