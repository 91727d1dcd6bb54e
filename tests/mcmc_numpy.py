"""A numpy restatement of the MCMC strategy's generator, per-step terms, event draws and whole events (include/gsplat.h
gs_set_mcmc, gs_mcmc_random, gs_mcmc_relocate, gs_mcmc_grow), for tests/test_mcmc_cpu.py, tests/test_gpu_mcmc.py and
tests/test_gpu_mcmc_events.py."""
from __future__ import annotations

import numpy as np

TAG0 = 0x6D636D63
TAGS = {0: 0x6E6F6973, 1: 0x72656C6F, 2: 0x67726F77}       # noise, relocation draws, growth draws
M32 = np.uint64(0xFFFFFFFF)


def philox(i, t: int, stream: int, seed: int):
    """Philox4x32-10 of counters (i, t, TAG0, tag) under key seed: uint32 [n, 4]."""
    i = np.asarray(i, np.uint64).reshape(-1)
    c0, c1 = i.copy(), np.full_like(i, t)
    c2, c3 = np.full_like(i, TAG0), np.full_like(i, TAGS[stream])
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def normals(words):
    """Box-Muller on the four words in float64 from float32 uniforms (the kernel forms u in float32): [n, 3]."""
    w = np.asarray(words, np.uint32)
    u = (np.float32(1.0 / 16777216.0) * ((w >> 8).astype(np.float32) + np.float32(0.5))).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a1, a3 = 2 * np.pi * u[:, 1], 2 * np.pi * u[:, 3]
    return np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3)], 1)


def uniforms(words):
    """((w0 >> 5) 2^26 + (w1 >> 6) + 1/2) 2^-53, float64 (the same IEEE operations as the kernel: bit for bit)."""
    w = np.asarray(words, np.uint32).astype(np.uint64)
    m = ((w[:, 0] >> np.uint64(5)) << np.uint64(26)) | (w[:, 1] >> np.uint64(6))
    return (m.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def regularizer_grads(scales_raw, opacity_raw, opacity_reg, scale_reg):
    """(d/d scales_raw, d/d opacity_raw) of opacity_reg mean(o) + scale_reg mean(s), float64."""
    s = np.exp(np.asarray(scales_raw, np.float64))
    o = sigmoid(opacity_raw)
    N = o.shape[0]
    return scale_reg * s / (3 * N), opacity_reg * o * (1 - o) / N


def rotmat(q):
    q = np.asarray(q, np.float64)
    q = q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-8)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def noise(scales_raw, rotation, opacity_raw, eps, noise_lr, lr_xyz):
    """Sigma eps noise_lr lr_xyz / (1 + exp(-100 ((1 - o) - 0.995))), float64 [N, 3]."""
    R = rotmat(rotation)
    s2 = np.exp(2.0 * np.asarray(scales_raw, np.float64))
    cov = np.einsum("nij,nj,nkj->nik", R, s2, R)
    o = sigmoid(opacity_raw)
    with np.errstate(over="ignore"):
        gate = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))
    return np.einsum("nij,nj->ni", cov, np.asarray(eps, np.float64)) * (noise_lr * lr_xyz * gate)[:, None]


def draw(opacity_raw, mode: int, min_opacity: float, n: int, seed: int, t: int):
    """The event's draws: mode 0 = relocation (candidates: finite, o > min_opacity), 1 = growth (finite, o > 0).
    Returns (sources [n], targets [n], cdf of the candidates, candidate rows, dead rows)."""
    raw = np.asarray(opacity_raw, np.float32)
    o = sigmoid(raw.astype(np.float64))
    fin = np.isfinite(raw)
    cand = fin & ((o > min_opacity) if mode == 0 else (o > 0))
    rows = np.nonzero(cand)[0]
    dead = np.nonzero(~cand)[0] if mode == 0 else np.zeros(0, np.int64)
    cdf = np.cumsum(o[rows])
    u = uniforms(philox(np.arange(n), t, 1 if mode == 0 else 2, seed))
    target = u * cdf[-1]
    k = np.minimum(np.searchsorted(cdf, target, side="right"), len(rows) - 1)
    return rows[k], target, cdf, rows, dead


def min_boundary_gap(cdf, target) -> float:
    """The smallest |cdf[q] - target[j]| / cdf[-1] over all draws j and prefix entries q.  The device builds its prefix in
    another summation order (a Hillis-Steele scan per block plus a serial carry), so its entries differ from numpy's cumsum by
    up to about N 2^-53 of the total: a draw whose target is farther than that from every entry has one possible source."""
    cdf, target = np.asarray(cdf, np.float64), np.asarray(target, np.float64).reshape(-1)
    if cdf.size == 0 or target.size == 0:
        return np.inf
    k = np.searchsorted(cdf, target)
    lo, hi = cdf[np.clip(k - 1, 0, cdf.size - 1)], cdf[np.clip(k, 0, cdf.size - 1)]
    return float(np.minimum(np.abs(target - lo), np.abs(hi - target)).min() / cdf[-1])


KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")


def event(p, m, v, mode: int, cfg, t: int, seed: int, n_add=None):
    """A whole event (include/gsplat.h gs_mcmc_relocate: mode 0, gs_mcmc_grow: mode 1) restated in float64 over the N rows of
    the six float32 tensors p and their moments m, v (dicts keyed like KEYS), with cfg's min_opacity, n_max, cap_max and
    grow_rate.  The destinations are the dead rows in index order (relocation) or the rows N + j (growth; n_add rows, by
    default grown_count(N, cap_max, grow_rate) - N).  A source drawn c times gets the formula's opacity and scale for n =
    min(c + 1, n_max), each rounded to float32 once; a destination is a copy of its source's modified row; the moments of
    sources and destinations are zero; every other float is the input's, bit for bit.

    Returns dict(p, m, v: the state after the event (N + n_add rows after a growth), N: its count, stats: dead / relocated /
    live / N as gs_mcmc_relocate reports them (relocation), sources: [draws] the source of every draw, dests: [draws] its
    destination, counts: [N] draws per row, cdf / target: the draws' prefix and targets (for min_boundary_gap))."""
    from gaussiansplattingmlx_amd.mcmc import grown_count, relocation_formula
    p = {k: np.array(p[k], np.float32, copy=True) for k in KEYS}
    m = {k: np.array(m[k], np.float32, copy=True) for k in KEYS}
    v = {k: np.array(v[k], np.float32, copy=True) for k in KEYS}
    N = p["opacity"].shape[0]
    raw = p["opacity"].reshape(N)
    o = sigmoid(raw.astype(np.float64))
    fin = np.isfinite(raw)
    cand = fin & ((o > cfg.min_opacity) if mode == 0 else (o > 0))
    n_dead, n_cand = (int((~cand).sum()) if mode == 0 else 0), int(cand.sum())
    if mode == 0:
        n_draw = n_dead
    else:
        n_draw = grown_count(N, cfg.cap_max, cfg.grow_rate) - N if n_add is None else int(n_add)
    out = dict(p=p, m=m, v=v, N=N, stats=dict(dead=n_dead, relocated=0, live=n_cand, N=N) if mode == 0 else None,
               sources=np.zeros(0, np.int64), dests=np.zeros(0, np.int64), counts=np.zeros(N, np.int64),
               cdf=np.zeros(0), target=np.zeros(0))
    if N == 0 or n_draw <= 0 or n_cand == 0:
        return out
    src, target, cdf, _, dead = draw(raw, mode, cfg.min_opacity, n_draw, seed, t)
    dst = dead if mode == 0 else N + np.arange(n_draw)
    cnt = np.bincount(src, minlength=N)
    s_rows = np.nonzero(cnt)[0]
    on, ratio = relocation_formula(o[s_rows], cnt[s_rows] + 1, cfg.min_opacity, cfg.n_max)
    p["opacity"].reshape(N)[s_rows] = np.log(on / (1.0 - on)).astype(np.float32)
    p["scales"][s_rows] = np.log(np.exp(p["scales"][s_rows].astype(np.float64)) * ratio[:, None]).astype(np.float32)
    for k in KEYS:
        m[k][s_rows] = 0
        v[k][s_rows] = 0
    if mode == 1:
        grow = lambda a, fill: np.concatenate([a, fill((n_draw,) + a.shape[1:], np.float32)])       # noqa: E731
        for k in KEYS:
            p[k], m[k], v[k] = grow(p[k], np.empty), grow(m[k], np.zeros), grow(v[k], np.zeros)
    for k in KEYS:
        p[k][dst] = p[k][src]
        m[k][dst] = 0
        v[k][dst] = 0
    out.update(N=N + (n_draw if mode == 1 else 0), sources=src, dests=np.asarray(dst, np.int64), counts=cnt, cdf=cdf, target=target)
    if mode == 0:
        out["stats"]["relocated"] = n_draw
    return out
