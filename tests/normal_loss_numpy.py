"""gs_normal_loss / gs_depth_normals (include/gsplat.h, csrc/normal_loss.hip) restated in numpy, in float64
or float32.

    pixel (i, j) = (column, row): rx = ((i + 0.5) - cx) / fx, ry = ((j + 0.5) - cy) / fy; depth-valid iff a >= alpha_min, a > 0,
    D > 0; z = D / a.  An interior pixel whose four neighbours and itself are depth-valid (and max(|A|, |B|) <= max_jump z when
    max_jump > 0) has
        A = z+ - z-,  S = (z+ + z-) / fx,  B = zd - zu,  T = (zd + zu) / fy,  m = (A T, B S, -((A T rx + B S ry) + S T)),  n = m / |m|
    L_l1 = sum_Vp |n - Nt|_1 / max(#Vp, 1e-6),  L_cos = sum_Vp (1 - n . Nt) / max(#Vp, 1e-6),
    L_s = sum_pairs w_pq (1 - n_p . n_q) / max(#pairs, 1e-6),  w_pq = exp(-gamma mean_c |I_p - I_q|)
    cotangents: g_n -> g_m -> (g_A, g_T, g_B, g_S) -> q = (q+, q-, qd, qu) -> gathered g_z -> (g_z / a, -g_z D / a^2)

The inputs are taken as they are given (float32 images stay the float32 values they are) and every operation runs in `dtype`, in
the order the kernels use; the camera, the weights, alpha_min, max_jump and gamma are first rounded to float32, as the C ABI takes
them.  The loss sums are taken in float64 in either dtype, as the kernels take them."""
import numpy as np


def _f32(x, dt):
    return dt(np.float32(x))


def depth_valid(D, a, alpha_min, dtype=np.float64):
    dt = np.dtype(dtype).type
    D, a = np.asarray(D, dt), np.asarray(a, dt)
    return (a >= _f32(alpha_min, dt)) & (a > 0) & (D > 0)


def _geometry(K, D, a, alpha_min, max_jump, dt):
    """has [H, W] bool and a dict of [H, W] arrays (A, B, S, T, rx, ry, len, n [H, W, 3]), zero where there is no normal."""
    fx, fy, cx, cy = (_f32(v, dt) for v in K)
    D, a = np.asarray(D, dt), np.asarray(a, dt)
    H, W = D.shape
    valid = depth_valid(D, a, alpha_min, dt)
    z = np.zeros((H, W), dt)
    z[valid] = D[valid] / a[valid]
    g = {k: np.zeros((H, W), dt) for k in ("A", "B", "S", "T", "rx", "ry", "len")}
    g["n"] = np.zeros((H, W, 3), dt)
    has = np.zeros((H, W), bool)
    if H < 3 or W < 3:
        return has, g, valid
    c = (slice(1, H - 1), slice(1, W - 1))
    zp, zm, zd, zu = z[1:-1, 2:], z[1:-1, :-2], z[2:, 1:-1], z[:-2, 1:-1]
    ok = valid[c] & valid[1:-1, 2:] & valid[1:-1, :-2] & valid[2:, 1:-1] & valid[:-2, 1:-1]
    A, B = zp - zm, zd - zu
    mj = _f32(max_jump, dt)
    if mj > 0:
        ok = ok & (np.maximum(np.abs(A), np.abs(B)) <= mj * z[c])
    S, T = (zp + zm) / fx, (zd + zu) / fy
    i, j = np.meshgrid(np.arange(1, W - 1), np.arange(1, H - 1))
    rx = ((i.astype(dt) + dt(0.5)) - cx) / fx
    ry = ((j.astype(dt) + dt(0.5)) - cy) / fy
    mx, my = A * T, B * S
    mz = -((mx * rx + my * ry) + S * T)
    ln = np.sqrt((mx * mx + my * my) + mz * mz)
    ok = ok & (ln > 0)
    safe = np.where(ok, ln, dt(1))
    for k, v in (("A", A), ("B", B), ("S", S), ("T", T), ("rx", rx), ("ry", ry), ("len", ln)):
        g[k][c] = np.where(ok, v, dt(0))
    g["n"][c] = np.where(ok[..., None], np.stack([mx / safe, my / safe, mz / safe], -1), dt(0))
    has[c] = ok
    return has, g, valid


def depth_normals(K, D, a, alpha_min=0.05, max_jump=0.0, dtype=np.float64):
    """-> (n [H, W, 3], the zero vector where there is no normal; has [H, W] bool)."""
    dt = np.dtype(dtype).type
    has, g, _ = _geometry(K, D, a, alpha_min, max_jump, dt)
    return g["n"], has


def _target(target, mask, shape, dt):
    """(Nt [H, W, 3] normalised, usable [H, W] bool)."""
    if target is None:
        return np.zeros(shape + (3,), dt), np.zeros(shape, bool)
    t = np.asarray(target, dt)
    s = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
    ok = s >= dt(0.25)
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    ln = np.sqrt(np.where(ok, s, dt(1)))
    return np.where(ok[..., None], t / ln[..., None], dt(0)), ok


def _weights(edge, gamma, shape, dt):
    """(wr [H, W-1] of the pairs (i, i+1), wd [H-1, W] of the pairs (j, j+1))."""
    H, W = shape
    gm = _f32(gamma, dt)
    if edge is None or not gm > 0:
        return np.ones((H, max(W - 1, 0)), dt), np.ones((max(H - 1, 0), W), dt)
    I = np.asarray(edge, dt)

    def w(p, q):
        d = np.abs(p - q)
        return np.exp(-gm * (((d[..., 0] + d[..., 1]) + d[..., 2]) / dt(3)))
    return w(I[:, :-1], I[:, 1:]), w(I[:-1], I[1:])


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def normal_loss(K, D, a, target=None, mask=None, edge=None, lam=(0.0, 0.0, 0.0), alpha_min=0.05, max_jump=0.0, gamma=0.0,
                dtype=np.float64):
    """-> dict(terms=(L_l1, L_cos, L_s) float64, total (their weighted sum, float64), cot_depth, cot_alpha [H, W] in dtype,
    n [H, W, 3], has, prior (Vp) [H, W] bool, valid [H, W] bool, counts=(#Vp, #pairs))."""
    dt = np.dtype(dtype).type
    l1w, cw, sw = (_f32(v, dt) for v in lam)
    fx, fy = _f32(K[0], dt), _f32(K[1], dt)
    D, a = np.asarray(D, dt), np.asarray(a, dt)
    H, W = D.shape
    has, g, valid = _geometry(K, D, a, alpha_min, max_jump, dt)
    n = g["n"]
    Nt, usable = _target(target, mask, (H, W), dt)
    prior = has & usable
    wr, wd = _weights(edge, gamma, (H, W), dt)
    pr, pd = has[:, :-1] & has[:, 1:], has[:-1] & has[1:]
    f8 = np.float64
    cP, cS = int(prior.sum()), int(pr.sum()) + int(pd.sum())
    nP, nS = max(float(cP), 1e-6), max(float(cS), 1e-6)
    diff = n - Nt
    l1 = (np.abs(diff[..., 0]) + np.abs(diff[..., 1])) + np.abs(diff[..., 2])
    L1 = float(np.where(prior, l1, dt(0)).sum(dtype=f8)) / nP
    Lc = float(np.where(prior, dt(1) - _dot(n, Nt), dt(0)).sum(dtype=f8)) / nP
    sr = np.where(pr, wr * (dt(1) - _dot(n[:, :-1], n[:, 1:])), dt(0))
    sd = np.where(pd, wd * (dt(1) - _dot(n[:-1], n[1:])), dt(0))
    Ls = (float(sr.sum(dtype=f8)) + float(sd.sum(dtype=f8))) / nS
    total = (float(l1w) * L1 + float(cw) * Lc) + float(sw) * Ls
    # g_n: the prior terms, then the pairs in the kernel's order (right, left, down, up)
    nPd, nSd = dt(np.float32(nP)) if dt is np.float32 else dt(nP), dt(np.float32(nS)) if dt is np.float32 else dt(nS)
    ka, kb = l1w / nPd, cw / nPd
    gn = np.where(prior[..., None], ka * np.sign(diff) - kb * Nt, dt(0)).astype(dt)
    ws = sw / nSd
    gn[:, :-1] = gn[:, :-1] - np.where(pr, ws * wr, dt(0))[..., None] * n[:, 1:]
    gn[:, 1:] = gn[:, 1:] - np.where(pr, ws * wr, dt(0))[..., None] * n[:, :-1]
    gn[:-1] = gn[:-1] - np.where(pd, ws * wd, dt(0))[..., None] * n[1:]
    gn[1:] = gn[1:] - np.where(pd, ws * wd, dt(0))[..., None] * n[:-1]
    dot = _dot(n, gn)
    ln = np.where(has, g["len"], dt(1))
    gm = (gn - n * dot[..., None]) / ln[..., None]
    mx, my, mz = gm[..., 0], gm[..., 1], gm[..., 2]
    A, B, S, T, rx, ry = (g[k] for k in ("A", "B", "S", "T", "rx", "ry"))
    gA = mx * T - mz * (T * rx)
    gT = mx * A - mz * (A * rx + S)
    gB = my * S - mz * (S * ry)
    gS = my * B - mz * (B * ry + T)
    sx, ty = gS / fx, gT / fy
    z0 = dt(0)
    qp, qm, qd, qu = (np.where(has, v, z0) for v in (gA + sx, -gA + sx, gB + ty, -gB + ty))
    gz = np.zeros((H, W), dt)
    gz[:, 1:] = gz[:, 1:] + qp[:, :-1]
    gz[:, :-1] = gz[:, :-1] + qm[:, 1:]
    gz[1:] = gz[1:] + qd[:-1]
    gz[:-1] = gz[:-1] + qu[1:]
    sa = np.where(valid, a, dt(1))
    cd = np.where(valid, gz / sa, z0)
    ca = np.where(valid, -gz * D / (sa * sa), z0)
    return dict(terms=(L1, Lc, Ls), total=total, cot_depth=cd, cot_alpha=ca, n=n, has=has, prior=prior, valid=valid,
                counts=(cP, cS), Nt=Nt)


def total(K, D, a, target=None, mask=None, edge=None, lam=(0.0, 0.0, 0.0), alpha_min=0.05, max_jump=0.0, gamma=0.0):
    """The weighted sum in float64: what the call adds to loss[0]."""
    return normal_loss(K, D, a, target, mask, edge, lam, alpha_min, max_jump, gamma)["total"]


def pick_max_jump(s, alpha_min=0.05, least=10):
    """A max_jump for scene s whose verdict no rounding changes: the scene's ratios max(|A|, |B|) / z are a continuum, so a
    threshold inside it has pixels within float32's reach of it (z carries 1.2e-7 of itself).  This one lies in the middle of
    the widest gap between two neighbouring ratios that still drops at least `least` pixels.  -> (max_jump as a float32 value,
    the gap, the number of pixels it drops)."""
    D, a = np.asarray(s["D"], np.float64), np.asarray(s["a"], np.float64)
    has, g, valid = _geometry(s["K"], D, a, alpha_min, 0.0, np.float64)
    z = np.where(valid, D / np.where(valid, a, 1.0), 1.0)
    rho = np.sort((np.maximum(np.abs(g["A"]), np.abs(g["B"])) / z)[has])
    gaps = np.diff(rho)[: len(rho) - least]
    lo = int(0.8 * len(rho))
    k = lo + int(np.argmax(gaps[lo:]))
    return float(np.float32(0.5 * (rho[k] + rho[k + 1]))), float(gaps[k]), len(rho) - 1 - k


def scene(H, W, seed=0):
    """The tests' images (float32): a tilted, wavy surface with sub-pixel roughness, an alpha in [0.55, 0.95) with a 4 x 5 block at
    0.01 (not depth-valid at alpha_min = 0.05), D = z a, random unit targets facing the camera, a random edge image, a random
    mask.  -> dict(K, D, a, target, edge, mask, z)."""
    rng = np.random.default_rng([seed, H, W])
    fx = fy = 0.9 * W
    cx, cy = W / 2 + 1.7, H / 2 - 2.3
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    rx, ry = ((i + 0.5) - cx) / fx, ((j + 0.5) - cy) / fy
    z = 4 + 0.8 * rx - 0.5 * ry + 0.15 * np.sin(9 * rx + 1) * np.cos(7 * ry) + (1.2 / fx) * rng.uniform(size=(H, W))
    a = 0.55 + 0.4 * rng.uniform(size=(H, W))
    if H > 8 and W > 9:
        a[H // 3: H // 3 + 4, W // 3: W // 3 + 5] = 0.01
    a = a.astype(np.float32)
    D = (z * a).astype(np.float32)
    t = rng.normal(size=(H, W, 3))
    t[..., 2] = -1.0 - np.abs(t[..., 2])
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    edge = rng.uniform(size=(H, W, 3)).astype(np.float32)
    mask = (rng.uniform(size=(H, W)) > 0.3).astype(np.uint8)
    return dict(K=(fx, fy, cx, cy), D=D, a=a, target=t.astype(np.float32), edge=edge, mask=mask, z=z)
