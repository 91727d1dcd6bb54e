"""The 3-D smoothing filter in float64 (include/gsplat.h gs_set_filter3d): Mip-Splatting's second filter.

    width        f_i = sqrt(0.2) min over the cameras n that SEE x_i of z / focal_x,n,   p = [x_i, 1] . view_n, z = p.z,
                 seen iff z >= 0.2, |p.x / z + ox| <= 1.3 tan(fov_x / 2), |p.y / z + oy| <= 1.3 tan(fov_y / 2), with
                 (ox, oy) = (proj[8] / proj[0], proj[9] / proj[5]) the camera's off-centre principal point (0 when centred);
                 a Gaussian no camera sees gets the largest f among the seen ones; nothing seen: all 0
    activations  s_eff = sqrt(s^2 + f^2),  kappa = prod_a s_a / s_eff_a,  opacity = sigma kappa (rho)
    VJP          dL/dscales_raw_a = g_a s_a^2 / s_eff_a + c sigma rho kappa f^2 / s_eff_a^2,  dL/dopacity_raw = c kappa rho sigma (1 - sigma)
    bake         scales_raw' = log s_eff,  opacity_raw' = logit(sigma kappa)

These are the host-side statements of what csrc/filter3d.hip and csrc/gs_math.h filter3d_activate compute in float32, for tests
and tools that compose the mode from the reference's ops (as antialias.py is for the anti-aliased mode's rho).
"""
from __future__ import annotations

import numpy as np

Z_NEAR = 0.2                # the projection's visibility rule
MARGIN = 1.3                # the EWA clamp's constant: Mip-Splatting's 15 % screen margin, 0.65 W / focal = 1.3 tan(fov / 2)
RATE = float(np.sqrt(0.2))  # Mip-Splatting's filter variance 0.2, as a width


def _cam(c):
    """(view [4, 4] float64, fovX, fovY, focalX) of a Camera or of a Camera.as_dict()."""
    if isinstance(c, dict):
        return np.asarray(c["view"], np.float64).reshape(4, 4), float(c["fovX"]), float(c["fovY"]), float(c["focalX"])
    return np.asarray(c.worldViewTransform, np.float64).reshape(4, 4), float(c.FoVx), float(c.FoVy), float(c.focalX)


def _offsets(c, fold: bool = True):
    """(ox, oy) = (proj[8] / proj[0], proj[9] / proj[5]) of a Camera or of a Camera.as_dict(): the off-centre principal point in
    units of x / z.  (0, 0) for a centred camera, for one without a projection matrix, and with
    fold=False (the table gs_set_filter3d_cameras builds for a centred camera)."""
    P = c.get("proj") if isinstance(c, dict) else getattr(c, "projectionMatrix", None)
    if P is None or not fold:
        return 0.0, 0.0
    P = np.asarray(P, np.float64).reshape(16)
    return (float(P[8] / P[0]) if P[8] != 0.0 and P[0] != 0.0 else 0.0,
            float(P[9] / P[5]) if P[9] != 0.0 and P[5] != 0.0 else 0.0)


def camera_terms(xyz, cam, fold: bool = True):
    """One camera's share per point: (seen [N] bool, T = z / focal_x [N], p [N, 3] the view-space point, (limX, limY)).  For an
    off-centre camera p.x and p.y carry the offset, p.x + ox z and p.y + oy z (the fold of gs_set_filter3d_cameras), so that
    seen is |p.x / z| <= limX, |p.y / z| <= limY for every camera; fold=False ignores the offset."""
    view, fx, fy, focal = _cam(cam)
    ox, oy = _offsets(cam, fold)
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    p = x @ view[:3, :3] + view[3, :3]
    z = p[:, 2]
    if ox != 0.0:
        p[:, 0] += ox * z
    if oy != 0.0:
        p[:, 1] += oy * z
    lim = (MARGIN * np.tan(fx / 2.0), MARGIN * np.tan(fy / 2.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        seen = (z >= Z_NEAR) & (np.abs(p[:, 0] / z) <= lim[0]) & (np.abs(p[:, 1] / z) <= lim[1])
    return seen, z / focal, p, lim


def filter_width(xyz, cameras, details: bool = False, fold: bool = True):
    """f [N] float64.  details=True: also (seen_any [N], argmin camera [N] (-1 where unseen)).  fold=False: the cameras'
    principal points are ignored (every frustum centred)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    best = np.full(x.shape[0], np.inf)
    arg = np.full(x.shape[0], -1, np.int64)
    for n, c in enumerate(cameras):
        seen, T, _, _ = camera_terms(x, c, fold)
        take = seen & (T < best)
        best[take] = T[take]
        arg[take] = n
    any_seen = arg >= 0
    f = np.zeros(x.shape[0])
    if any_seen.any():
        f[any_seen] = RATE * best[any_seen]
        f[~any_seen] = f[any_seen].max()
    return (f, any_seen, arg) if details else f


def threshold_distance(xyz, cameras):
    """The smallest relative distance of any (point, camera) pair to one of the three thresholds of `seen`: |z - 0.2| / 0.2,
    ||p.x / z| - limX| / limX, ||p.y / z| - limY| / limY, over every pair (in front of the camera plane or behind it).  A float32
    evaluation sees the same set when this is well above its rounding."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    d = np.inf
    for c in cameras:
        _, _, p, lim = camera_terms(x, c)
        z = p[:, 2]
        d = min(d, float(np.abs(z - Z_NEAR).min() / Z_NEAR))
        front = z != 0
        if front.any():
            d = min(d, float((np.abs(np.abs(p[front, 0] / z[front]) - lim[0]) / lim[0]).min()),
                    float((np.abs(np.abs(p[front, 1] / z[front]) - lim[1]) / lim[1]).min()))
    return d


def width_bar(xyz, cameras, ulps: float = 8.0):
    """Per element, the float32 error bound of the width kernel's arithmetic: ulps 2^-23 (|x v02| + |y v12| + |z v22| + |v32|)
    / focal sqrt(0.2) at the camera that sets the width (three products, three sums, a division, a product: below 8 roundings
    of a quantity bounded by the sum of the terms' magnitudes); the never-seen take the largest bar among the elements they
    may copy."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    f, any_seen, arg = filter_width(x, cameras, details=True)
    bar = np.zeros(x.shape[0])
    for n, c in enumerate(cameras):
        view, _, _, focal = _cam(c)
        m = arg == n
        if m.any():
            mag = np.abs(x[m] * view[:3, 2]).sum(axis=1) + abs(view[3, 2])
            bar[m] = ulps * 2.0 ** -23 * mag / focal * RATE
    if any_seen.any() and (~any_seen).any():
        # the copied element is the float32 maximum: any seen element whose interval reaches the float64 maximum's
        fs, bs = f[any_seen], bar[any_seen]
        top = np.argmax(fs)
        bar[~any_seen] = bs[fs + bs >= fs[top] - bs[top]].max()
    return bar


def filter_scales(s, f, dtype=np.float64):
    """(s_eff [N, 3], kappa [N]) from ACTIVATED scales s = exp(scales_raw) [N, 3] and widths [N], in `dtype` and in the kernels'
    order of operations (gs_math.h filter3d_activate: s s + f f, its square root, the three ratios, (r0 r1) r2).  float64 is the
    statement the kernels are held to; float32 is their own arithmetic, for a float32 oracle loop."""
    s = np.asarray(s, dtype).reshape(-1, 3)
    f = np.asarray(f, dtype).reshape(-1, 1)
    se = np.sqrt(s * s + f * f)
    r = s / se
    return se, r[:, 0] * r[:, 1] * r[:, 2]


def activations(scales_raw, f):
    """(s_eff [N, 3], kappa [N]) from raw scales [N, 3] and widths [N]; kappa as the product of the three ratios."""
    return filter_scales(np.exp(np.asarray(scales_raw, np.float64).reshape(-1, 3)), f)


def filter_vjp(s, sigma, f, g_seff, c, rho=1.0):
    """activations_vjp from the ACTIVATED values s = exp(scales_raw) [N, 3] and sigma = sigmoid(opacity_raw) [N] (what an
    oracle's activations_forward returned), in float64."""
    s = np.asarray(s, np.float64).reshape(-1, 3)
    f = np.asarray(f, np.float64).reshape(-1, 1)
    se, kappa = filter_scales(s, f)
    sg = np.asarray(sigma, np.float64).reshape(-1)
    c = np.asarray(c, np.float64).reshape(-1)
    rho = np.broadcast_to(np.asarray(rho, np.float64).reshape(-1), c.shape)
    ds = np.asarray(g_seff, np.float64).reshape(-1, 3) * s * s / se + (c * sg * rho * kappa)[:, None] * (f * f) / (se * se)
    return ds, c * kappa * rho * sg * (1.0 - sg)


def activations_vjp(scales_raw, opacity_raw, f, g_seff, c, rho=1.0):
    """(dL/dscales_raw [N, 3], dL/dopacity_raw [N]) from g_seff = dL/ds_eff [N, 3] and c = dL/d(packed opacity) [N]."""
    s = np.exp(np.asarray(scales_raw, np.float64).reshape(-1, 3))
    f = np.asarray(f, np.float64).reshape(-1, 1)
    se, kappa = activations(scales_raw, f)
    sg = 1.0 / (1.0 + np.exp(-np.asarray(opacity_raw, np.float64).reshape(-1)))
    c = np.asarray(c, np.float64).reshape(-1)
    rho = np.broadcast_to(np.asarray(rho, np.float64).reshape(-1), c.shape)
    ds = np.asarray(g_seff, np.float64).reshape(-1, 3) * s * s / se + (c * sg * rho * kappa)[:, None] * (f * f) / (se * se)
    return ds, c * kappa * rho * sg * (1.0 - sg)


def bake(scales_raw, opacity_raw, f):
    """Mip-Splatting's fused export: (log s_eff [N, 3], logit(sigma kappa) [N]).  logit(sigma kappa) = log kappa -
    log((1 - kappa) + exp(-o)), with 1 - kappa summed from the ratios' complements so that nothing cancels where kappa -> 1."""
    s = np.exp(np.asarray(scales_raw, np.float64).reshape(-1, 3))
    o = np.asarray(opacity_raw, np.float64).reshape(-1)
    f = np.asarray(f, np.float64).reshape(-1, 1)
    se, kappa = activations(scales_raw, f)
    d = f * f / (se * (se + s))
    r = s / se
    omk = d[:, 0] + r[:, 0] * d[:, 1] + r[:, 0] * r[:, 1] * d[:, 2]
    return np.log(se), np.log(kappa) - np.log(omk + np.exp(-o))
