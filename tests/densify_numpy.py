"""A numpy restatement of the densify / prune event's kernels (csrc/densify.hip: the scan, the plan, the two output maps, the
noise generator and the gather), integers exact and floats in float64, with the action mixes and sizes the tests share;
for tests/test_densify_numpy_cpu.py (which qualifies it without a device) and tests/test_gpu_densify_kernels.py."""
from __future__ import annotations

import numpy as np

KEEP, SPLIT, CLONE, PRUNE = 0, 1, 2, 3
SCAN_TILE = 1024                    # counts per scan tile (DN_SCAN_TILE)
SCAN_CHUNK = 256 * SCAN_TILE        # rows behind one 256-tile chunk of dn_tile_offsets_kernel's carry loop
NOISE_TAG = (0x64656E73, 0x69667921)
M32 = np.uint64(0xFFFFFFFF)
NOISE_BAR = 1e-5                    # test_gpu_mcmc.py::test_generator_matches_the_restatement holds the same arithmetic to it

# ------------------------------------------------------------------------------------------------ the cases the tests share
SCAN_NS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 262143, 262144, 262145, 524288, 524289, 786433)
MAP_NS = (1025, 262145)
MIXES = ("random", "all_keep", "all_prune", "all_split", "all_clone", "first_split", "first_prune", "last_split", "last_prune",
         "alternating_tiles", "chunk0_prune")
GATHER_KS = (1, 4, 9, 16, 25)
GATHER_NS = (1, 257, 1000)
GATHER_MIXES = ("random", "prune_only")
NOISE_ROWS = (1, 255, 256, 257, 4096)
NOISE_SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 20260313)


def actions_of(mix: str, N: int, seed: int = 5):
    """The action of every row (int32 [N]) of a named mix, generated as integers (no classification)."""
    rng = np.random.default_rng([seed, N])
    rand = rng.choice(4, size=N, p=[0.7, 0.1, 0.1, 0.1]).astype(np.int32)
    a = np.zeros(N, np.int32)
    if mix == "random":
        a = rand
    elif mix == "prune_only":                                  # what contribution pruning produces
        a = np.where(rng.random(N) < 0.15, PRUNE, KEEP).astype(np.int32)
    elif mix in ("all_keep", "all_prune", "all_split", "all_clone"):
        a[:] = dict(all_keep=KEEP, all_prune=PRUNE, all_split=SPLIT, all_clone=CLONE)[mix]
    elif mix in ("first_split", "first_prune"):
        a[0] = SPLIT if mix == "first_split" else PRUNE
    elif mix in ("last_split", "last_prune"):
        a[N - 1] = SPLIT if mix == "last_split" else PRUNE
    elif mix == "alternating_tiles":                           # whole tiles that sum to zero between tiles of 2048
        a = np.where((np.arange(N) // SCAN_TILE) % 2 == 0, PRUNE, SPLIT).astype(np.int32)
    elif mix == "chunk0_prune":                                # a whole 256-tile chunk that sums to zero
        a = rand
        a[:SCAN_CHUNK] = PRUNE
    else:
        raise ValueError(mix)
    return a


# ------------------------------------------------------------------------------------------------ scan, plan, maps
def counts_of(actions):
    """Output rows of every action: keep 1, split and clone 2, prune 0."""
    return np.array([1, 2, 2, 0], np.int32)[np.asarray(actions, np.int64)]


def offsets(actions):
    """(exclusive cumsum of the counts [N] int32, dict(total, keep, split, clone, prune))."""
    a = np.asarray(actions, np.int64)
    c = counts_of(a).astype(np.int64)
    incl = np.cumsum(c)
    h = np.bincount(a, minlength=4)
    st = dict(total=int(incl[-1]) if len(a) else 0, keep=int(h[0]), split=int(h[1]), clone=int(h[2]), prune=int(h[3]))
    return (incl - c).astype(np.int32), st


def output_map(actions, off, total: int):
    """build_map_kernel: (gather, mode), int32 [total].  A row whose slots do not all fit `total` writes nothing; modes are
    1 / 2 for a split's two rows, 0 / 3 for a clone's, 0 for a kept row; unwritten slots are 0."""
    a, o = np.asarray(actions, np.int64), np.asarray(off, np.int64)
    total = max(int(total), 0)
    gather, mode = np.zeros(total, np.int32), np.zeros(total, np.int32)
    rows = np.arange(len(a))
    fits = (a >= 0) & (a <= 2) & (o >= 0) & (o + np.where(a == 0, 1, 2) <= total)
    gather[o[fits]] = rows[fits]
    mode[o[fits]] = a[fits] == 1
    two = fits & (a != 0)
    gather[o[two] + 1] = rows[two]
    mode[o[two] + 1] = np.where(a[two] == 1, 2, 3)
    return gather, mode


PLAN_WORDS = ("N_new", "applies", "total", "keep", "split", "clone", "prune", "N")


def plan(actions, N: int):
    """dn_plan_kernel's eight words: new count, applies, total, keep, split, clone, prune, N.  Nothing applies when every row
    is pruned (total 0) or when no row splits, clones or is pruned."""
    _, st = offsets(actions)
    applies = int(st["total"] > 0 and (st["split"] or st["clone"] or st["prune"]) != 0)
    return [st["total"] if applies else int(N), applies, st["total"], st["keep"], st["split"], st["clone"], st["prune"], int(N)]


def planned_map(actions, off, plan_words, cap: int):
    """build_map_planned_kernel over `cap` zero-filled slots: output_map for min(total, cap) slots when the plan applies, the
    identity on the rows below min(N, cap) when it does not."""
    N, cap = len(actions), int(cap)
    gather, mode = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    if not plan_words[1]:
        n = min(N, cap)
        gather[:n] = np.arange(n)
        return gather, mode
    total = min(int(plan_words[2]), cap)
    gather[:total], mode[:total] = output_map(actions, off, total)
    return gather, mode


# ------------------------------------------------------------------------------------------------ the noise generator
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123): counter uint [n, 4], key (k0, k1) -> uint32 [n, 4]."""
    c = np.asarray(counter, np.uint64).reshape(-1, 4) & M32
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                     # 32 x 32 -> 64 bits: no wrap
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def noise_words(seed: int, rows):
    """The four words of densify_noise3's rows: counter (row, 0, 'dens', 'ify!'), key the seed's two halves."""
    rows = np.arange(rows) if np.isscalar(rows) else np.asarray(rows)
    c = np.zeros((len(rows), 4), np.uint64)
    c[:, 0], c[:, 2], c[:, 3] = rows, NOISE_TAG[0], NOISE_TAG[1]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32))


def noise_uniforms(words):
    """(u [n, 4] float32, the two angles 6.2831855f u1 and 6.2831855f u3 as float32): the kernel's own float32 operations,
    each a correctly rounded IEEE operation, so these are its bits.  (float32(w >> 8) is exact; + 0.5f rounds to even from
    w >> 8 = 2^23 on, i.e. w >= 2^31; u = 1 occurs and gives a radius of zero.)"""
    w = np.asarray(words, np.uint32)
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    ang = np.float32(6.283185307179586) * u[:, [1, 3]]
    assert u.dtype == np.float32 and ang.dtype == np.float32
    return u, ang


def densify_noise(seed: int, rows, dtype=np.float64):
    """[n, 3] standard normal of the output rows `rows` (a count or an array of row numbers): Box-Muller on the float32
    uniforms, sin / cos / log / sqrt in `dtype` (float64: the reference; float32: the walk the kernel takes)."""
    u, ang = noise_uniforms(noise_words(seed, rows))
    u, ang = u.astype(dtype), ang.astype(dtype)
    ra, rb = np.sqrt(dtype(-2.0) * np.log(u[:, 0])), np.sqrt(dtype(-2.0) * np.log(u[:, 2]))
    z = np.stack([ra * np.cos(ang[:, 0]), ra * np.sin(ang[:, 0]), rb * np.cos(ang[:, 1])], 1)
    assert z.dtype == dtype
    return z


# ------------------------------------------------------------------------------------------------ the gather
SCALE_REDUCTION = np.float32(-np.log(1.6))
PARAMS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")


def gather(params, gather_idx, mode, noise):
    """gather_small_kernel + the row gather in float64: out[j] = in[gather[j]]; with noise ([total, 3], or None: a plain copy)
    xyz += (+-1 for a split's two rows) mean(exp(scales)) 0.1f nz + (clone's second row) 0.01f nz and a split's scales +=
    float32(-log 1.6).  (The sum of two float32 values rounded to float64 and then to float32 is their float32 sum: scales
    come out with the kernel's bits.)"""
    g, m = np.asarray(gather_idx, np.int64), np.asarray(mode, np.int64)
    out = {k: np.asarray(params[k], np.float64)[g] for k in PARAMS}
    if noise is None:
        return out
    nz = np.asarray(noise, np.float64).reshape(len(g), 3)
    sc = out["scales"]
    mean = (np.exp(sc[:, 0]) + np.exp(sc[:, 1]) + np.exp(sc[:, 2])) * np.float64(np.float32(1.0 / 3.0))
    sign = (m == 1).astype(np.float64) - (m == 2)
    split_noise = (sign * mean * np.float64(np.float32(0.1)))[:, None] * nz
    clone_noise = ((m == 3) * np.float64(np.float32(0.01)))[:, None] * nz
    out["xyz"] = out["xyz"] + split_noise + clone_noise
    out["scales"] = sc + ((m == 1) | (m == 2))[:, None] * np.float64(SCALE_REDUCTION)
    return out


def gather_params(N: int, K: int, seed: int = 11):
    """Six float32 tensors of a test model; every value distinct enough that a wrong row or a wrong column shows."""
    rng = np.random.default_rng([seed, N, K])
    p = dict(xyz=rng.normal(size=(N, 3)), features_dc=rng.normal(size=(N, 1, 3)), features_rest=rng.normal(size=(N, K - 1, 3)),
             scales=rng.normal(np.log(0.01), 0.5, (N, 3)), rotation=rng.normal(size=(N, 4)), opacity=rng.normal(-3, 3, N))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ classify / accumulate
CLASSIFY_THRESHOLDS = (dict(gradThreshold=0.0002, maxScale=0.01, minOpacity=0.005),            # the defaults
                       dict(gradThreshold=0.00075, maxScale=0.02, minOpacity=0.02))
CLASSIFY_DENOMS = (0.0, -1.0, 8.0)


def classify_inputs(th: dict, N: int = 3000, seed: int = 3):
    """(gradAccum [N], scales [N, 4] with junk in column 3, opacity [N]) float32 for classify_kernel under the thresholds `th`
    and denom 8: random rows, then rows with the statistic exactly at and one ulp above threshold x 8 (the quotient by a power of
    two is exact: `avg > threshold` is false at, true above), raw scales of 89 (exp overflows to inf) and -104 (exp underflows to
    zero) and raw opacities of +-inf (sigmoid exactly 1 and 0).  No NaN."""
    rng = np.random.default_rng([seed, N])
    thr = np.float32(th["gradThreshold"])
    acc = (np.abs(rng.normal(0, 1.5, N)) * thr * np.float32(8.0)).astype(np.float32)
    scales = np.empty((N, 4), np.float32)
    scales[:, :3] = rng.normal(np.log(th["maxScale"]), 0.5, (N, 3))
    scales[:, 3] = rng.choice([80.0, -80.0, 1e30, -1e30], N)             # junk: would overflow the maximum if it were read
    opacity = rng.normal(np.log(th["minOpacity"] / (1 - th["minOpacity"])), 2.0, N).astype(np.float32)
    at = thr * np.float32(8.0)
    assert np.float32(at / np.float32(8.0)) == thr
    acc[0:8] = at
    acc[8:16] = np.nextafter(at, np.float32(np.inf))
    acc[16:24] = np.nextafter(at, np.float32(0.0))
    small, big = np.float32(np.log(th["maxScale"]) - 1.0), np.float32(np.log(th["maxScale"]) + 1.0)
    scales[0:24:2, :3], scales[1:24:2, :3] = small, big                   # each of the three statistics with a clone and a split
    opacity[0:24] = 2.0
    acc[24:40] = at * np.float32(4.0)
    scales[24:28, :3], scales[28:32, :3] = (small, 89.0, small), (-104.0, -104.0, -104.0)
    scales[32:36, :3], scales[36:40, :3] = (-104.0, small, 89.0), (small, small, -104.0)
    opacity[24:40:2], opacity[25:40:2] = np.inf, -np.inf
    opacity[40:44], opacity[44:48] = np.inf, -np.inf
    return acc, scales, opacity


def classify_near(th: dict, scales, opacity):
    """The existing test's exclusion rule: rows whose decision value lies within 4 ulp (4e-7 relative) of a threshold, where
    the device's exp and libm's may round differently."""
    with np.errstate(over="ignore"):
        ms = np.exp(np.asarray(scales, np.float64)[:, :3]).max(1)
        op = 1 / (1 + np.exp(-np.asarray(opacity, np.float64)))
    return (np.abs(ms - th["maxScale"]) < 4e-7 * th["maxScale"]) | (np.abs(op - th["minOpacity"]) < 4e-7 * th["minOpacity"])


ACCUM_NS = (1, 255, 256, 257)


def accum_inputs(N: int, seed: int = 17):
    """(xyz gradient [N, 3], accumulator [N]) float32: random rows and components of 1e-25 (the square underflows to zero)
    and 1e20 (the square overflows to inf)."""
    rng = np.random.default_rng([seed, N])
    g = rng.normal(0, 1e-3, (N, 3)).astype(np.float32)
    acc = np.abs(rng.normal(0, 1e-3, N)).astype(np.float32)
    g[0] = (1e-25, -1e-25, 1e-25)
    if N > 4:
        g[1], g[2], g[3], g[4] = (1e20, 0.0, 0.0), (1e-25, 3e-4, 0.0), (-1e20, 1e20, 1e-25), (0.0, 0.0, 0.0)
    return g, acc
