"""The bilateral grid restated in numpy (include/gsplat.h gs_set_bilateral_grid), composed with the oracle's loss.

A grid G of shape (grid_w, grid_h, grid_l) is an array [grid_h, grid_w, grid_l, 12]: G[y][x][z] is a 3 x 4 M = [A | b] in
exposure's convention.  Pixel (x, y) slices it at (u, v, w) -- its position and the clamped luminance of the render -- with
nested lerps (x, then y, then z), and the loss is taken of a r + b.  Everything is computed in `dtype` in the header's order of
operations; in float32 each fmaf is a float64 product and sum rounded once to float32 (its double rounding is ~1 ulp away
from the device's fmaf at worst, well inside every bar that compares the two).  The grid gradient's pixel sums run in
float64."""
import numpy as np

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)
LUM = (0.299, 0.587, 0.114)


def identity(shape):
    gw, gh, gl = shape
    return np.tile(IDENTITY, (gh, gw, gl, 1))


def constant(M, shape):
    gw, gh, gl = shape
    return np.tile(np.asarray(M, np.float32).reshape(12), (gh, gw, gl, 1))


def random_grid(rng, shape, amp=0.15):
    """Identity plus a smooth random field: per coefficient a low-order polynomial in (x, y, z) of size ~amp."""
    gw, gh, gl = shape
    y, x, z = np.meshgrid(np.linspace(-1, 1, gh), np.linspace(-1, 1, gw), np.linspace(-1, 1, gl), indexing="ij")
    G = identity(shape).astype(np.float64)
    for k in range(12):
        c = rng.uniform(-1, 1, 7) * amp / 3
        G[..., k] += c[0] + c[1] * x + c[2] * y + c[3] * z + c[4] * x * y + c[5] * z * z + c[6] * x * z
    return G.astype(np.float32)


def _fma(a, b, c, dt):
    if dt == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(dt)


def _lerp(a, b, t, dt):
    return _fma(t, (b - a).astype(dt), a, dt)


def _axis(n_px, n_nodes, dt):
    """u per pixel (one correctly rounded division of two exact integers), its cell and fraction."""
    i = np.arange(n_px)
    u = (np.asarray((2 * i + 1) * (n_nodes - 1), dt) / dt(2 * n_px)).astype(dt)
    c = np.minimum(u.astype(np.int64), n_nodes - 2)
    return c, (u - c.astype(dt)).astype(dt)


def place(render, shape, dtype=np.float32):
    """Per pixel: x0 [W], fu [W], y0 [H], fv [H], z0 [H, W], fw [H, W], gray [H, W] (unclamped)."""
    dt = np.dtype(dtype).type
    gw, gh, gl = shape
    r = np.asarray(render, dt)
    H, W, _ = r.shape
    x0, fu = _axis(W, gw, dt)
    y0, fv = _axis(H, gh, dt)
    gray = _fma(dt(LUM[0]), r[..., 0], _fma(dt(LUM[1]), r[..., 1], (dt(LUM[2]) * r[..., 2]).astype(dt), dt), dt)
    w = (np.minimum(np.maximum(gray, dt(0)), dt(1)) * dt(gl - 1)).astype(dt)
    z0 = np.minimum(w.astype(np.int64), gl - 2)
    fw = (w - z0.astype(dt)).astype(dt)
    return x0, fu, y0, fv, z0, fw, gray


def slice_grid(G, render, shape, dtype=np.float32):
    """(a [H, W, 12], P_hi - P_lo [H, W, 12], place(...)): the sliced coefficients and the z-difference the VJP needs."""
    dt = np.dtype(dtype).type
    G = np.asarray(G, dt).reshape(shape[1], shape[0], shape[2], 12)
    pl = place(render, shape, dtype)
    x0, fu, y0, fv, z0, fw, _ = pl
    Y, X = y0[:, None], x0[None, :]
    FU, FV, FW = fu[None, :, None], fv[:, None, None], fw[..., None]

    def bil(z):
        c0 = _lerp(G[Y, X, z], G[Y, X + 1, z], FU, dt)
        c1 = _lerp(G[Y + 1, X, z], G[Y + 1, X + 1, z], FU, dt)
        return _lerp(c0, c1, FV, dt)
    plo, phi = bil(z0), bil(z0 + 1)
    return _lerp(plo, phi, FW, dt), (phi - plo).astype(dt), pl


def _affine(a, r, dt):
    out = np.empty(r.shape, dt)
    for c in range(3):
        out[..., c] = _fma(a[..., 4 * c], r[..., 0], _fma(a[..., 4 * c + 1], r[..., 1],
                                                          _fma(a[..., 4 * c + 2], r[..., 2], a[..., 4 * c + 3], dt), dt), dt)
    return out


def apply(G, img, shape, dtype=np.float32):
    """The image under the grid, in `dtype`."""
    dt = np.dtype(dtype).type
    a, _, _ = slice_grid(G, img, shape, dtype)
    return _affine(a, np.asarray(img, dt), dt)


def tv(G, shape):
    """TV(G) = sum over the axes of (1 / n_axis) sum (G_next - G)^2 (float64)."""
    G = np.asarray(G, np.float64).reshape(shape[1], shape[0], shape[2], 12)
    return sum(float((np.diff(G, axis=ax) ** 2).sum()) / np.diff(G, axis=ax).size for ax in (0, 1, 2))


def tv_grad(G, shape):
    """dTV/dG (float64), the grid's shape."""
    G = np.asarray(G, np.float64).reshape(shape[1], shape[0], shape[2], 12)
    out = np.zeros_like(G)
    for ax in (0, 1, 2):
        d = np.diff(G, axis=ax)
        s = 2.0 / d.size
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        out[tuple(lo)] -= s * d
        out[tuple(hi)] += s * d
    return out


def vjp(G, g, render, shape, tv_weight=0.0, dtype=np.float32):
    """(dL/dr [H, W, 3] in `dtype`, dL/dG [grid_h, grid_w, grid_l, 12] float64) from g = dL/d(corrected image)."""
    dt = np.dtype(dtype).type
    gw, gh, gl = shape
    r = np.asarray(render, dt)
    g = np.asarray(g, dt)
    a, dP, (x0, fu, y0, fv, z0, fw, gray) = slice_grid(G, r, shape, dtype)
    H, W, _ = r.shape
    base = np.empty(r.shape, dt)
    for j in range(3):
        base[..., j] = _fma(a[..., j], g[..., 0], _fma(a[..., 4 + j], g[..., 1], (a[..., 8 + j] * g[..., 2]).astype(dt), dt), dt)
    da = np.empty((H, W, 12), dt)
    for c in range(3):
        for j in range(3):
            da[..., 4 * c + j] = g[..., c] * r[..., j]
        da[..., 4 * c + 3] = g[..., c]
    s = (dP[..., 0] * da[..., 0]).astype(dt)
    for k in range(1, 12):
        s = _fma(dP[..., k], da[..., k], s, dt)
    dgray = np.where((gray > 0) & (gray < 1), (s * dt(gl - 1)).astype(dt), dt(0))
    dr = np.empty(r.shape, dt)
    for j in range(3):
        dr[..., j] = _fma(dgray, dt(LUM[j]), base[..., j], dt)
    # dL/dG: every pixel scatters wt(p, node) da_p into its eight nodes, wt = (wx wy) wz
    dG = np.zeros((gh, gw, gl, 12))
    Y = np.broadcast_to(y0[:, None], (H, W))
    X = np.broadcast_to(x0[None, :], (H, W))
    FU = np.broadcast_to(fu[None, :], (H, W))
    FV = np.broadcast_to(fv[:, None], (H, W))
    da64 = da.astype(np.float64)
    for dy in (0, 1):
        wy = FV if dy else (dt(1) - FV).astype(dt)
        for dx in (0, 1):
            wx = FU if dx else (dt(1) - FU).astype(dt)
            wxy = (wx * wy).astype(dt)
            for dz in (0, 1):
                wz = fw if dz else (dt(1) - fw).astype(dt)
                wt = (wxy * wz).astype(dt).astype(np.float64)
                np.add.at(dG, (Y + dy, X + dx, z0 + dz), wt[..., None] * da64)
    if tv_weight:
        dG += tv_weight * tv_grad(G, shape)
    return dr, dG


def composed(o, render, target, G, shape, tv_weight=0.0, lam=0.2, **depth):
    """The oracle `o`'s loss of the render under G at the oracle's precision: (loss, dL/dr, dL/dG, g).  The loss is the data
    term alone (the library's loss[4]); dL/dG includes tv_weight dTV/dG."""
    c = apply(G, render, shape, o.dtype)
    loss, g, _, _, _ = o.loss_forward_backward(c, target, lam, **depth)
    dr, dG = vjp(G, g, render, shape, tv_weight, o.dtype)
    return loss, dr, dG, g
