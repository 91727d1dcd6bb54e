"""gs_depth_loss / gs_depth_normalize (include/gsplat.h, csrc/depth_loss.hip) restated in numpy, in
float64 or float32.

    D render depth, a render alpha, t = scale * target + offset
    accumulated  x = D      valid iff mask
    expected     x = D / a  valid iff mask, a >= alpha_min, a > 0
    disparity    x = a / D  valid iff mask, a >= alpha_min, a > 0, D > 0
    n = max(#valid, 1e-6),  Ld = sum_valid |x - t| / n,  g = lambda sign(x - t) / n on valid pixels, 0 elsewhere
    cotangents (depth, alpha):  (g, 0)   (g / a, -g D / a^2)   (-g a / D^2, g / D)

The inputs are taken as they are given (float32 images stay the float32 values they are) and every operation runs in `dtype`;
lambda, alpha_min, scale and offset are first rounded to float32, as the C ABI takes them."""
import numpy as np

ACCUMULATED, EXPECTED, DISPARITY = 0, 1, 2
MODES = ("accumulated", "expected", "disparity")


def _f32(x, dtype):
    return dtype(np.float32(x))


def valid_and_x(mode, D, a, mask, alpha_min, dtype=np.float64):
    """(valid [bool], x [dtype], 0 where invalid)."""
    D, a = np.asarray(D, dtype), np.asarray(a, dtype)
    valid = np.ones(D.shape, bool) if mask is None else np.asarray(mask) != 0
    x = np.zeros(D.shape, dtype)
    if mode == ACCUMULATED:
        x[valid] = D[valid]
        return valid, x
    valid = valid & (a >= _f32(alpha_min, dtype)) & (a > 0)
    if mode == EXPECTED:
        x[valid] = D[valid] / a[valid]
        return valid, x
    valid = valid & (D > 0)
    x[valid] = a[valid] / D[valid]
    return valid, x


def depth_loss(mode, D, a, target, mask, lam, alpha_min=0.05, scale=1.0, offset=0.0, dtype=np.float64):
    """-> (Ld, cot_depth, cot_alpha, valid), all in dtype."""
    dt = np.dtype(dtype).type
    D, a, target = np.asarray(D, dt), np.asarray(a, dt), np.asarray(target, dt)
    valid, x = valid_and_x(mode, D, a, mask, alpha_min, dt)
    t = _f32(scale, dt) * target + _f32(offset, dt)
    n = dt(max(float(valid.sum()), 1e-6))
    d = np.where(valid, x - t, dt(0))
    Ld = dt(np.abs(d).sum(dtype=np.float64) / np.float64(n)) if dt is np.float32 else np.abs(d).sum() / n
    g = _f32(lam, dt) * np.sign(d).astype(dt) / n
    cd, ca = np.zeros(D.shape, dt), np.zeros(D.shape, dt)
    v = valid
    if mode == ACCUMULATED:
        cd[v] = g[v]
    elif mode == EXPECTED:
        cd[v] = g[v] / a[v]
        ca[v] = -g[v] * D[v] / (a[v] * a[v])
    else:
        cd[v] = -g[v] * a[v] / (D[v] * D[v])
        ca[v] = g[v] / D[v]
    return Ld, cd, ca, valid


def total(mode, D, a, target, mask, lam, alpha_min=0.05, scale=1.0, offset=0.0, base=0.0):
    """base + lambda Ld in float64: what loss[0] holds after the call."""
    return base + float(np.float32(lam)) * float(depth_loss(mode, D, a, target, mask, lam, alpha_min, scale, offset)[0])


def expected_depth(D, a, alpha_min, dtype=np.float32):
    dt = np.dtype(dtype).type
    return valid_and_x(EXPECTED, D, a, None, alpha_min, dt)[1]


def inputs(H, W, mode, alpha_min=0.05, seed=0):
    """The GPU tests' images (float32): D in [0.5, 20]; a in [0, 1] with a block of exact zeros, a block exactly alpha_min (valid)
    and every other value at least 1e-3 from the threshold; target = x (1 +- delta), delta in [0.05, 0.3], so that no sign is
    ambiguous between float32 and float64; in the accumulated mode a block of exact ties target == D; a random mask."""
    rng = np.random.default_rng([seed, H, W, mode])
    D = rng.uniform(0.5, 20.0, (H, W)).astype(np.float32)
    a = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    am = np.float32(alpha_min)
    near = np.abs(a - am) < np.float32(1e-3)
    a[near] = am + np.float32(2e-3)
    a[: H // 5, : W // 4] = 0.0
    a[H // 5: 2 * (H // 5), : W // 4] = am
    mask = (rng.uniform(size=(H, W)) > 0.3).astype(np.uint8)
    _, x = valid_and_x(mode, D, a, None, alpha_min, np.float64)
    if mode != ACCUMULATED:      # (where a pixel is invalid any target does: keep it finite and ordinary)
        x = np.where(x == 0, 1.0, x)
    delta = rng.uniform(0.05, 0.3, (H, W)) * rng.choice([-1.0, 1.0], (H, W))
    target = (x * (1.0 + delta)).astype(np.float32)
    if mode == ACCUMULATED:
        target[-(H // 5):, -(W // 4):] = D[-(H // 5):, -(W // 4):]
    return D, a, target, mask
