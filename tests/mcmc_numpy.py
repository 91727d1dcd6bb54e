"""A numpy restatement of the MCMC strategy's generator, per-step terms and event draws (include/gsplat.h gs_set_mcmc,
gs_mcmc_random, gs_mcmc_relocate, gs_mcmc_grow), for tests/test_mcmc_cpu.py and tests/test_gpu_mcmc.py."""
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
