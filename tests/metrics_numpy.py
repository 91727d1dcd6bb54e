"""gs_image_metrics / gs_colour_moments (include/gsplat.h, csrc/metrics.hip) restated in numpy.

dtype = np.float64 is the truth the tests hold the kernels to.  dtype = np.float32 evaluates what the kernel evaluates,
operation for operation: the clamp, the weights, the five planes a, b, a a, b b, a b, the separable window (rows, then columns,
taps ascending, acc = acc + g[k] x) and the SSIM quotient, every step rounded to float32.  The sums are float64 in both, as the
kernel's are double.  ssim_map_bruteforce is the 121-tap form in float64: the mirror checks itself against it."""
import numpy as np

K, PAD, SIGMA = 11, 5, 1.5
C1, C2 = 1e-4, 9e-4


def taps(dtype=np.float64):
    """The eleven normalised taps exp(-(i - 5)^2 / (2 sigma^2)), summed in order, every step in dtype."""
    dt = np.dtype(dtype).type
    d = (np.arange(K) - PAD).astype(dtype)
    g = np.exp(-(d * d) / dt(2.0 * SIGMA * SIGMA)).astype(dtype)
    s = dt(0)
    for x in g:
        s = dt(s + x)
    return (g / s).astype(dtype)


def weights(mask, shape, dtype=np.float64):
    """Pixel weights: (float)v / 255.0f, the float32 quotient, in dtype; ones without a mask."""
    if mask is None:
        return np.ones(shape, dtype)
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8) * np.uint8(255)
    assert m.dtype == np.uint8 and m.shape == tuple(shape)
    return (m.astype(np.float32) / np.float32(255.0)).astype(dtype)


def clamp(img, dtype=np.float64):
    return np.clip(np.asarray(img, np.float32), np.float32(0), np.float32(1)).astype(dtype)


def _window(plane, g):
    """The zero-padded "same" separable filter of one [H, W] plane: rows, then columns, taps ascending."""
    dtype = plane.dtype
    H, W = plane.shape
    p = np.zeros((H, W + 2 * PAD), dtype)
    p[:, PAD:PAD + W] = plane
    acc = np.zeros((H, W), dtype)
    for k in range(K):
        acc = acc + g[k] * p[:, k:k + W]
    p = np.zeros((H + 2 * PAD, W), dtype)
    p[PAD:PAD + H] = acc
    out = np.zeros((H, W), dtype)
    for k in range(K):
        out = out + g[k] * p[k:k + H]
    return out


def _ssim_from_stats(m1, m2, E11, E22, E12, dtype):
    dt = np.dtype(dtype).type
    m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
    s1, s2, s12 = E11 - m11, E22 - m22, E12 - m12
    num = (dt(2) * m12 + dt(C1)) * (dt(2) * s12 + dt(C2))
    den = (m11 + m22 + dt(C1)) * (s1 + s2 + dt(C2))
    return num / den


def ssim_map(a, b, dtype=np.float64):
    """Inria's ssim_map of two [H, W, C] images already clamped (and weighted), per channel, in dtype."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    g = taps(dtype)
    out = np.empty(a.shape, dtype)
    for c in range(a.shape[2]):
        x, y = a[..., c], b[..., c]
        st = [_window(p, g) for p in (x, y, x * x, y * y, x * y)]
        out[..., c] = _ssim_from_stats(*st, dtype)
    return out


def ssim_map_bruteforce(a, b):
    """The same map with the 121-tap window g (x) g, float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = taps(np.float64)
    win = np.outer(g, g)
    H, W, C = a.shape
    out = np.empty(a.shape)
    for c in range(C):
        st = []
        for plane in (a[..., c], b[..., c], a[..., c] ** 2, b[..., c] ** 2, a[..., c] * b[..., c]):
            p = np.zeros((H + 2 * PAD, W + 2 * PAD))
            p[PAD:PAD + H, PAD:PAD + W] = plane
            acc = np.zeros((H, W))
            for i in range(K):
                for j in range(K):
                    acc += win[i, j] * p[i:i + H, j:j + W]
            st.append(acc)
        out[..., c] = _ssim_from_stats(*st, np.float64)
    return out


def image_metrics(render, target, mask=None, dtype=np.float64):
    """dict(sums = {sse, ssim_sum, wsum, 3 wsum} float64 [4], psnr, ssim, map = the per-pixel ssim values [H, W, 3], w [H, W])."""
    r, g = clamp(render, dtype), clamp(target, dtype)
    w = weights(mask, r.shape[:2], dtype)
    d = r - g
    sse = (w[..., None] * (d * d)).astype(np.float64).sum()
    smap = ssim_map(w[..., None] * r, w[..., None] * g, dtype)
    ssim_sum = (w[..., None] * smap).astype(np.float64).sum()
    wsum = w.astype(np.float64).sum()
    sums = np.array([sse, ssim_sum, wsum, 3.0 * wsum])
    psnr, ssim = from_sums(sums)
    return dict(sums=sums, psnr=psnr, ssim=ssim, map=smap, w=w)


def from_sums(sums):
    """(psnr, ssim): inf where the error is zero, nan where wsum is."""
    s = np.asarray(sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(-10.0 * np.log10(s[0] / s[3])), float(s[1] / s[3])


TRIU = [(i, j) for i in range(4) for j in range(i, 4)]


def colour_moments(render, target, mask=None):
    """The 22 moments, float64: S[i][j] = sum w p_i p_j (upper triangle by rows), then T[i][c] = sum w p_i t_c."""
    r, t = clamp(render).reshape(-1, 3), clamp(target).reshape(-1, 3)
    w = weights(mask, np.shape(render)[:2]).reshape(-1)
    p = np.concatenate([r, np.ones((r.shape[0], 1))], 1)
    S = (w[:, None] * p).T @ p
    T = (w[:, None] * p).T @ t
    return np.concatenate([[S[i, j] for i, j in TRIU], T.reshape(-1)])


def pixel_matrix_fit(render, target, mask=None):
    """M [3, 4] by least squares on the pixels themselves: sqrt(w) p M^T = sqrt(w) t."""
    r, t = clamp(render).reshape(-1, 3), clamp(target).reshape(-1, 3)
    sw = np.sqrt(weights(mask, np.shape(render)[:2]).reshape(-1))[:, None]
    p = np.concatenate([r, np.ones((r.shape[0], 1))], 1)
    return np.linalg.lstsq(sw * p, sw * t, rcond=None)[0].T


def apply_affine(M, img, dtype=np.float64):
    """M p of the CLAMPED image, computed in float64 and rounded to dtype."""
    M = np.asarray(M, np.float64).reshape(3, 4)
    return (clamp(img) @ M[:, :3].T + M[:, 3]).astype(dtype)


# ---- the test images ---------------------------------------------------------------------------------------------------
def noise_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((H, W, 3), dtype=np.float32), rng.random((H, W, 3), dtype=np.float32)


def ramp_pair(H, W, seed):
    """A ramp from -0.3 to 1.3 across the image (each channel another direction) plus 0.05 noise: both clamps at work."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    base = np.stack([u, v, 0.5 * (u + v)], -1) * 1.6 - 0.3
    a = base + 0.05 * rng.standard_normal((H, W, 3))
    b = base + 0.05 * rng.standard_normal((H, W, 3))
    return a.astype(np.float32), b.astype(np.float32)


def close_pair(H, W, seed):
    a = np.random.default_rng(seed).random((H, W, 3), dtype=np.float32) * np.float32(0.9)
    return a, a + np.float32(0.002)


IMAGES = dict(noise=noise_pair, ramp=ramp_pair, close=close_pair)


def make_mask(kind, H, W, seed):
    rng = np.random.default_rng(seed + 77)
    if kind == "none":
        return None
    if kind == "ones":
        return np.full((H, W), 255, np.uint8)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "binary":
        return (rng.random((H, W)) < 0.6).astype(np.uint8) * np.uint8(255)
    if kind == "soft":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    raise ValueError(kind)


MASKS = ("none", "ones", "zeros", "binary", "soft")
