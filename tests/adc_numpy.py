"""A numpy restatement of the adaptive density control kernels (csrc/adc.hip: the step's statistic, the decision, the gather
with its split sampling and revised opacity, the moments' gather and the opacity reset), parameterised by dtype: float64 is the
reference, float32 the walk the kernels take (the same operations in the same order, each rounded to float32; only exp, log and
hypot may round differently from the device's).  For tests/test_adc_cpu.py (which qualifies it without a device) and
tests/test_gpu_adc.py, with the inputs and the distance rule the two share."""
from __future__ import annotations

import numpy as np

KEEP, SPLIT, CLONE, PRUNE = 0, 1, 2, 3
PARAMS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
SCALE_REDUCTION = np.float32(-np.log(1.6))
DEFAULTS = dict(grad_threshold=0.0002, percent_dense=0.01, min_opacity=0.005, max_screen_size=20.0, prune_world=0.1,
                scene_extent=4.0)


# ------------------------------------------------------------------------------------------------ the step's statistic
def accumulate(rows16, radii, use_abs, W, H, gradSum, count, maxRadius, dtype=np.float64):
    """adc_accum_kernel: (gradSum, count, maxRadius) after one step.  Rows of radius > 0 add hypot(W/2 gx, H/2 gy) of columns
    0, 1 (12, 13 with use_abs), one visit and the radius; the others keep their values."""
    rows = np.asarray(rows16, np.float32).reshape(-1, 16).astype(dtype)
    r = np.asarray(radii, np.float32).astype(dtype)
    col = 12 if use_abs else 0
    g, n, mr = (np.asarray(a, np.float32).astype(dtype).copy() for a in (gradSum, count, maxRadius))
    vis = r > 0
    x, y = dtype(0.5 * W) * rows[:, col], dtype(0.5 * H) * rows[:, col + 1]
    h = np.hypot(x, y)
    assert h.dtype == dtype
    g[vis] = g[vis] + h[vis]
    n[vis] = n[vis] + dtype(1.0)
    mr[vis] = np.maximum(mr[vis], r[vis])
    return g, n, mr


# ------------------------------------------------------------------------------------------------ the decision
def thresholds(prm: dict, dtype=np.float64):
    """The decision's six numbers as the kernel gets them: float32 values, the two products taken in float32 on the host."""
    f = {k: np.float32(v) for k, v in prm.items()}
    out = dict(grad=f["grad_threshold"], dense=f["percent_dense"] * f["scene_extent"], op=f["min_opacity"],
               screen=f["max_screen_size"], world=f["prune_world"] * f["scene_extent"])
    return {k: dtype(v) for k, v in out.items()}


def decision_values(gradSum, count, maxRadius, scales, opacity, dtype=np.float64):
    """(avg, smax, op, maxRadius) in `dtype`: the four numbers the decision compares with its thresholds."""
    g, n, mr = (np.asarray(a, np.float32).astype(dtype) for a in (gradSum, count, maxRadius))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        avg = np.where(n > 0, g / np.where(n > 0, n, dtype(1.0)), dtype(0.0)).astype(dtype)
        smax = np.exp(np.asarray(scales, np.float32)[:, :3].astype(dtype)).max(axis=1)
        op = dtype(1.0) / (dtype(1.0) + np.exp(-np.asarray(opacity, np.float32).reshape(-1).astype(dtype)))
    assert avg.dtype == smax.dtype == op.dtype == dtype
    return avg, smax, op, mr


def classify(gradSum, count, maxRadius, scales, opacity, prm: dict, allowDensify, sizePrune, dtype=np.float64):
    """adc_classify_kernel: (actions, counts) int32 [N]."""
    avg, smax, op, mr = decision_values(gradSum, count, maxRadius, scales, opacity, dtype)
    t = thresholds(prm, dtype)
    low = op < t["op"]
    grow = bool(allowDensify) & (avg >= t["grad"])
    big = bool(sizePrune) & (((t["screen"] > 0) & (mr > t["screen"])) | (smax > t["world"]))
    a = np.where(low, PRUNE, np.where(grow, np.where(smax <= t["dense"], CLONE, SPLIT), np.where(big, PRUNE, KEEP)))
    a = a.astype(np.int32)
    return a, np.array([1, 2, 2, 0], np.int32)[a]


def near_threshold(gradSum, count, maxRadius, scales, opacity, prm: dict, rel=1e-3):
    """Rows one of whose decision values lies within `rel` (relative) of its threshold in float64."""
    avg, smax, op, mr = decision_values(gradSum, count, maxRadius, scales, opacity, np.float64)
    t = thresholds(prm, np.float64)
    near = lambda v, th: np.abs(v - th) <= rel * abs(th)      # noqa: E731
    out = near(avg, t["grad"]) | near(smax, t["dense"]) | near(smax, t["world"]) | near(op, t["op"])
    if t["screen"] > 0:
        out |= near(mr, t["screen"])
    return out


# ------------------------------------------------------------------------------------------------ the gather
def rotation_matrices(q, dtype=np.float64):
    """R(q / max(|q|, 1e-8)) [n, 3, 3] as build_cov3d forms it (gs_math.h), sums left to right."""
    q = np.asarray(q, np.float32).astype(dtype)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    norm = np.sqrt(n2)
    safe = np.where(norm > dtype(1e-8), norm, dtype(np.float32(1e-8)))
    w, x, y, z = (q[:, i] / safe for i in range(4))
    one, two = dtype(1.0), dtype(2.0)
    R = np.empty((len(q), 3, 3), dtype)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - w * z)
    R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y)
    R[:, 2, 1] = two * (y * z + w * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def revised_opacity(o, dtype=np.float64):
    """Raw opacity of alpha' with 1 - (1 - alpha')^2 = sigmoid(o), in the kernel's form: t = 1 / (1 + e^o) = 1 - alpha,
    r = sqrt(t), alpha' = alpha / (1 + r), 1 - alpha' = r."""
    o = np.asarray(o, np.float32).astype(dtype)
    one = dtype(1.0)
    with np.errstate(over="ignore", divide="ignore"):
        a = one / (one + np.exp(-o))
        r = np.sqrt(one / (one + np.exp(o)))
        out = np.log(a / ((one + r) * r))
    assert out.dtype == dtype
    return out


def gather(params, gather_idx, mode, noise, revised=False, dtype=np.float64):
    """adc_gather_small_kernel + the row gather: out[j] = in[gather[j]]; a split's two rows (modes 1, 2) get
    xyz + R(q) (exp(scales) * noise[j]) and scales + float32(-log 1.6); a clone's rows (0 in front of its 3) are copies.
    revised: split rows and both rows of a clone get revised_opacity."""
    g, m = np.asarray(gather_idx, np.int64), np.asarray(mode, np.int64)
    out = {k: np.asarray(params[k], np.float32)[g].astype(dtype) for k in PARAMS}
    split = (m == 1) | (m == 2)
    nz = np.asarray(noise, np.float32).reshape(len(g), 3).astype(dtype)
    sc = out["scales"]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(sc) * nz
        R = rotation_matrices(np.asarray(params["rotation"], np.float32)[g], dtype)
        off = np.empty_like(e)
        for a in range(3):
            acc = R[:, a, 0] * e[:, 0]
            acc = acc + R[:, a, 1] * e[:, 1]
            acc = acc + R[:, a, 2] * e[:, 2]
            off[:, a] = acc
        out["xyz"] = np.where(split[:, None], out["xyz"] + off, out["xyz"])
    out["scales"] = np.where(split[:, None], sc + dtype(SCALE_REDUCTION), sc)
    if revised:
        first = np.zeros(len(g), bool)
        first[:-1] = (m[:-1] == 0) & (m[1:] == 3) & (g[1:] == g[:-1])
        rev = split | (m == 3) | first
        o = out["opacity"].reshape(-1)
        out["opacity"] = np.where(rev, revised_opacity(np.asarray(params["opacity"], np.float32).reshape(-1)[g], dtype),
                                  o).reshape(out["opacity"].shape)
    for k in PARAMS:
        assert out[k].dtype == dtype
    return out


def gather_moments(moments, gather_idx, mode, actions):
    """adc_gather_moments_kernel on a dict of six tensors: rows with mode 0 whose source is no split are copied (float32, bit
    for bit), every other row is zero."""
    g, m, a = np.asarray(gather_idx, np.int64), np.asarray(mode, np.int64), np.asarray(actions, np.int64)
    kept = (m == 0) & (a[g] != SPLIT)
    out = {}
    for k in PARAMS:
        src = np.asarray(moments[k], np.float32)[g]
        out[k] = np.where(kept.reshape((-1,) + (1,) * (src.ndim - 1)), src, np.float32(0.0)).astype(np.float32)
    return out


def reset_raw(reset_value) -> np.float32:
    """logit(reset_value) as gs_adc_reset_opacity forms it: the float32 value, the logit in double, rounded to float32."""
    rv = np.float64(np.float32(reset_value))
    return np.float32(np.log(rv / (1.0 - rv)))


def reset_opacity(opacity, m, v, reset_value=0.01):
    """adc_reset_opacity_kernel: (min(opacity, logit(reset_value)), zeros, zeros) float32."""
    o = np.asarray(opacity, np.float32)
    return np.minimum(o, reset_raw(reset_value)), np.zeros_like(np.asarray(m, np.float32)), np.zeros_like(np.asarray(v, np.float32))


# ------------------------------------------------------------------------------------------------ the distance rule
def ulp32(x):
    """One float32 ulp of |x| (of the smallest normal number below it)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), np.float64(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def yardstick(want32, want64, magnitude=None):
    """The float32-to-float64 distance of the restatements: the largest |want32 - want64| over the elements, each in float32
    ulps of the element's `magnitude` -- the float64 value itself where the result is a sum of like signs or a product (the
    statistic), the magnitude of what was added up where terms may cancel (gather_magnitudes): a rounding error is an ulp of an
    operand, not of a difference that came out small.  One number per tensor: the device and numpy round exp, log and hypot
    differently, so WHICH element is a last place off differs between them."""
    w64 = np.asarray(want64, np.float64)
    d = np.abs(np.asarray(want32, np.float64) - w64) / ulp32(w64 if magnitude is None else magnitude)
    return float(d.max()) if d.size else 0.0


def distance_check(got, want32, want64, magnitude=None, factor=4.0):
    """(worst distance of `got` from float64, the yardstick, the bar, all in ulps; the elements beyond the bar): no element may
    be further from float64 than `factor` x the yardstick, with a floor of one float32 ulp, in ulps of the element's magnitude."""
    w64 = np.asarray(want64, np.float64)
    mag = w64 if magnitude is None else np.maximum(np.abs(np.asarray(magnitude, np.float64)), np.abs(w64))
    yard = yardstick(want32, w64, mag)
    bar = max(factor * yard, 1.0)
    d = np.abs(np.asarray(got, np.float64) - w64) / ulp32(mag)
    return (float(d.max()) if d.size else 0.0), yard, bar, np.argwhere(d > bar)


def gather_magnitudes(params, gather_idx, mode, noise, revised=False):
    """Per element of the gather's float results, the magnitude its rounding errors scale with (float64): xyz |p_a| + sum_k
    |R_ak| e^s_k |z_k| (the child's offset may cancel the position), scales |s| + log 1.6, opacity max(|o'|, |o|, 1) (the
    revised opacity is a logarithm: a relative error of its argument is an absolute error of the result, so near o' = 0 the
    unit is an ulp of 1)."""
    g, m = np.asarray(gather_idx, np.int64), np.asarray(mode, np.int64)
    split = (m == 1) | (m == 2)
    p = np.abs(np.asarray(params["xyz"], np.float64)[g])
    sc = np.asarray(params["scales"], np.float64)[g]
    e = np.exp(sc) * np.abs(np.asarray(noise, np.float64).reshape(len(g), 3))
    R = np.abs(rotation_matrices(np.asarray(params["rotation"], np.float32)[g], np.float64))
    off = np.einsum("nak,nk->na", R, e)
    o = np.asarray(params["opacity"], np.float64).reshape(-1)[g]
    mag_o = np.maximum(np.abs(o), 1.0)
    if revised:
        mag_o = np.maximum(mag_o, np.abs(revised_opacity(np.asarray(params["opacity"], np.float32).reshape(-1)[g])))
    return dict(xyz=np.where(split[:, None], p + off, p), scales=np.abs(sc) + split[:, None] * np.log(1.6), opacity=mag_o)


# ------------------------------------------------------------------------------------------------ inputs the tests share
N_GPU = 2500          # crosses two boundaries of the 1024-item scan tile and leaves a partial 256-thread block


def accumulate_inputs(N=N_GPU, seed=23):
    """(rows16 [N, 16], radii [N], the three accumulators) float32 for the op-level accumulate: random rows with junk in the
    unread columns, zero radii among positive ones, a row whose sums are 1e-25 (squares underflow) and one of 1e20 (overflow)."""
    rng = np.random.default_rng([seed, N])
    rows = rng.normal(0, 1e-4, (N, 16)).astype(np.float32)
    rows[:, 12:14] = np.abs(rng.normal(0, 1e-3, (N, 2)))
    radii = (3.0 * rng.integers(1, 40, N)).astype(np.float32)
    radii[rng.random(N) < 0.3] = 0.0
    rows[5, 0:2], rows[5, 12:14], radii[5] = (1e-25, -1e-25), (1e-25, 1e-25), 6.0
    rows[6, 0:2], rows[6, 12:14], radii[6] = (1e20, -1e20), (1e20, 1e20), 9.0
    radii[7], radii[N - 1] = 0.0, 12.0            # a zero radius between positive ones; the last row of the partial block
    radii[4], radii[8] = 3.0, 3.0
    acc = np.stack([np.abs(rng.normal(0, 1e-2, N)), rng.integers(0, 50, N).astype(np.float64), 3.0 * rng.integers(0, 30, N)])
    return rows, radii, acc.astype(np.float32)


def classify_inputs(prm: dict, N=N_GPU, seed=29):
    """(gradSum, count, maxRadius, scales [N, 3], opacity [N]) float32: random rows spread about every threshold (with
    count == 0 rows), then every row whose avg, smax, op or maxRadius lies within 1e-3 relative of its threshold in float64 is
    pushed away from it by 1 % (the device's exp and division may round the last place differently from numpy's)."""
    rng = np.random.default_rng([seed, N])
    t = thresholds(prm)
    count = rng.integers(0, 40, N).astype(np.float32)
    count[rng.random(N) < 0.05] = 0.0
    gradSum = (np.abs(rng.normal(0, 1.2, N)) * t["grad"] * np.maximum(count, 1.0)).astype(np.float32)
    centre = np.log(np.where(rng.random(N) < 0.5, t["dense"], t["world"]))
    scales = (centre[:, None] + rng.normal(0, 0.7, (N, 3))).astype(np.float32)
    opacity = rng.normal(np.log(t["op"] / (1 - t["op"])), 2.0, N).astype(np.float32)
    opacity[rng.random(N) < 0.5] += np.float32(4.0)
    screen = t["screen"] if t["screen"] > 0 else 20.0
    maxRadius = (np.abs(rng.normal(0, 1.0, N)) * screen).astype(np.float32)
    for _ in range(4):
        avg, smax, op, mr = decision_values(gradSum, count, maxRadius, scales, opacity)
        near = lambda v, th: np.abs(v - th) <= 1e-3 * abs(th)      # noqa: E731
        gradSum = np.where(near(avg, t["grad"]), gradSum * np.float32(1.01), gradSum).astype(np.float32)
        scales = np.where((near(smax, t["dense"]) | near(smax, t["world"]))[:, None], scales + np.float32(0.01), scales)
        opacity = np.where(near(op, t["op"]), opacity + np.float32(0.01), opacity)
        if t["screen"] > 0:
            maxRadius = np.where(near(mr, t["screen"]), maxRadius * np.float32(1.01), maxRadius).astype(np.float32)
    return gradSum, count, maxRadius, np.ascontiguousarray(scales, np.float32), opacity.astype(np.float32)


def gather_params(N=N_GPU, K=16, seed=31):
    """Six float32 tensors of a test model: distinct values everywhere, quaternions far from unit length (row 3: length 7,
    row 4: 1e-3), moderate scales and opacities on both sides of 0."""
    rng = np.random.default_rng([seed, N, K])
    p = dict(xyz=rng.normal(size=(N, 3)), features_dc=rng.normal(size=(N, 1, 3)), features_rest=rng.normal(size=(N, K - 1, 3)),
             scales=rng.normal(np.log(0.05), 0.6, (N, 3)), rotation=rng.normal(size=(N, 4)), opacity=rng.normal(0, 3, N))
    p["rotation"][3] *= 7.0 / np.linalg.norm(p["rotation"][3])
    p["rotation"][4] *= 1e-3 / np.linalg.norm(p["rotation"][4])
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


def gather_actions(N=N_GPU, seed=37):
    """The action of every row: a random mix with rows 3 and 4 (the unnormalised quaternions) split."""
    rng = np.random.default_rng([seed, N])
    a = rng.choice(4, size=N, p=[0.55, 0.15, 0.15, 0.15]).astype(np.int32)
    a[3] = a[4] = SPLIT
    a[5], a[6], a[7] = CLONE, KEEP, PRUNE
    return a
