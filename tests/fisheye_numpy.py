"""The equidistant fisheye projection (include/gsplat.h gs_set_camera_model; csrc/gs_math.h fisheye_map,
build_cov2d / project_geometry / project_geometry_bwd with FISHEYE) restated in numpy: the mean, the Jacobian, the covariance and
the full VJP of the geometry, in float32 and in float64.

float32 mirrors the kernel's form operation for operation -- the polynomial atan ratio, the series below GS_FISHEYE_SERIES_W, the
order of every sum -- with mul, add, div and sqrt only, so that means, radii and rects are the bits the device produces
(projection.hip is compiled without FMA contraction).  float64 is the textbook form: atan2 from libm, the quotients' series below
w = 1e-3 (ten terms; the closed forms lose eps / w to cancellation, 2e-13 there) -- the reference the float32 form is measured against.

Conventions as the kernels': view is the row-major 4 x 4 with p_view = [p, 1] @ view, proj[2, 0] / proj[2, 1] carry the principal
point (camera.py), a cotangent of cov2d / conic has four independent entries.
"""
from __future__ import annotations

import numpy as np

SERIES_W = 0.04                      # GS_FISHEYE_SERIES_W
SERIES_W64 = 1e-3
# atan(sqrt w) / sqrt w on [0, 1], highest power first (fisheye_atan_ratio)
ATAN_RATIO = (0.0028340641874819994, -0.016005029901862144, 0.042587608098983765, -0.07495445758104324, 0.10636754333972931,
              -0.14202570915222168, 0.19992484152317047, -0.3333306610584259, 1.0)


def _series_coeffs(terms):
    """g z^3 = sum_{k >= 1} (-1)^k 2 k / (2 k + 1) w^(k - 1) and its derivative in w, lowest power first."""
    G = [(-1.0) ** k * 2.0 * k / (2.0 * k + 1.0) for k in range(1, terms + 1)]
    D = [(-1.0) ** k * 2.0 * k * (k - 1.0) / (2.0 * k + 1.0) for k in range(2, terms + 2)]
    return G, D


def _horner(coeffs_high_first, w, dt):
    a = np.full_like(w, dt(coeffs_high_first[0]))
    for c in coeffs_high_first[1:]:
        a = a * w + dt(c)
    return a


def _kernel_series32(w):
    f = np.float32
    G = [f(12.0) / f(13.0), f(-10.0) / f(11.0), f(8.0) / f(9.0), f(-6.0) / f(7.0), f(4.0) / f(5.0), f(-2.0) / f(3.0)]
    D = [f(-84.0) / f(15.0), f(60.0) / f(13.0), f(-40.0) / f(11.0), f(24.0) / f(9.0), f(-12.0) / f(7.0), f(4.0) / f(5.0)]
    return _horner(G, w, f), _horner(D, w, f)


def fisheye_map(x, y, z, dtype=np.float64):
    """s = theta / r, g = 2 ds/drho, h = 1 / (rho + z^2), grho = dg/drho of the view-space points (x, y, z)."""
    dt = np.dtype(dtype).type
    x, y, z = (np.asarray(v, dtype) for v in (x, y, z))
    with np.errstate(all="ignore"):
        rho = x * x + y * y
        z2 = z * z
        h = dt(1.0) / (rho + z2)
        w = rho / z2
        if dt is np.float32:
            near = (z > 0) & (w <= dt(1.0))
            s_near = _horner(ATAN_RATIO, np.where(near, w, dt(0.0)), dt) / z
            r = np.sqrt(rho)
            az = np.abs(z)
            steep = az < r
            lo, hi = np.where(steep, az, r), np.where(steep, r, az)
            a = lo / hi
            th = a * _horner(ATAN_RATIO, a * a, dt)
            th = np.where(steep, dt(1.5707963267948966) - th, th)
            th = np.where(z < 0, dt(3.141592653589793) - th, th)
            s = np.where(near, s_near, th / r)
            ser = (z > 0) & (w < dt(SERIES_W))
            G, D = _kernel_series32(np.where(ser, w, dt(0.0)))
            iz = dt(1.0) / z
            iz3 = iz * iz * iz
            g_far = (z * h - s) / rho
            grho_far = -(z * h * h + dt(1.5) * g_far) / rho
            g = np.where(ser, G * iz3, g_far)
            grho = np.where(ser, D * iz3 * iz * iz, grho_far)
        else:
            r = np.sqrt(rho)
            s = np.where(r > 0, np.arctan2(r, z) / np.where(r > 0, r, 1.0), 1.0 / z)
            ser = (z > 0) & (w < SERIES_W64)
            Gc, Dc = _series_coeffs(10)
            ws = np.where(ser, w, 0.0)
            iz = 1.0 / z
            g_far = (z * h - s) / rho
            grho_far = -(z * h * h + 1.5 * g_far) / rho
            g = np.where(ser, _horner(Gc[::-1], ws, dt) * iz ** 3, g_far)
            grho = np.where(ser, _horner(Dc[::-1], ws, dt) * iz ** 5, grho_far)
    return s.astype(dtype), g.astype(dtype), h.astype(dtype), grho.astype(dtype)


def jacobian(x, y, z, fx, fy, dtype=np.float64):
    """[..., 2, 3]: d(fx x s, fy y s) / d(x, y, z), and the map's (s, g, h, grho)."""
    dt = np.dtype(dtype).type
    x, y, z = (np.asarray(v, dtype) for v in (x, y, z))
    fx, fy = dt(fx), dt(fy)
    s, g, h, grho = fisheye_map(x, y, z, dtype)
    with np.errstate(all="ignore"):
        xy = x * y * g
        J = np.stack([np.stack([fx * (s + x * x * g), fx * xy, -(fx * x * h)], -1),
                      np.stack([fy * xy, fy * (s + y * y * g), -(fy * y * h)], -1)], -2)
    return J.astype(dtype), (s, g, h, grho)


def jacobian_vjp(x, y, z, fx, fy, dj, fm=None, dtype=np.float64):
    """(dx, dy, dz) = sum_ra dj[3 r + a] dJ[r][a] / d(x, y, z): the second derivatives of the map under the cotangent of J
    (dj: six arrays, rows (x, y, z) of the two screen coordinates)."""
    dt = np.dtype(dtype).type
    x, y, z = (np.asarray(v, dtype) for v in (x, y, z))
    fx, fy, two = dt(fx), dt(fy), dt(2.0)
    sm, g, h, grho = fm if fm is not None else fisheye_map(x, y, z, dtype)
    with np.errstate(all="ignore"):
        a00, a01, a02 = fx * dj[0], fx * dj[1], fx * dj[2]
        a10, a11, a12 = fy * dj[3], fy * dj[4], fy * dj[5]
        A, ax = a00 + a11, a01 + a10
        B = a00 * x * x + ax * x * y + a11 * y * y
        Cc = a02 * x + a12 * y
        h2 = h * h
        common = A * g + two * B * grho + two * Cc * h2
        dt0 = x * common + g * (two * a00 * x + ax * y) - a02 * h
        dt1 = y * common + g * (two * a11 * y + ax * x) - a12 * h
        dt2 = -(A * h) + two * B * h2 + two * Cc * z * h2
    return dt0, dt1, dt2


def principal_offset(proj, W, H, dtype):
    """(cx - 0.5, cy - 0.5) as the kernel forms them from proj[8], proj[9]."""
    dt = np.dtype(dtype).type
    P = np.asarray(proj, dtype).reshape(16)
    return ((P[8] + dt(1.0)) * dt(W) - dt(1.0)) * dt(0.5), ((P[9] + dt(1.0)) * dt(H) - dt(1.0)) * dt(0.5)


def view_points(means3d, view, dtype):
    V = np.asarray(view, dtype).reshape(16)
    m = np.asarray(means3d, dtype)
    return [m[:, 0] * V[a] + m[:, 1] * V[4 + a] + m[:, 2] * V[8 + a] + V[12 + a] for a in range(3)]


def _cov3d(scales, rot, dtype):
    dt = np.dtype(dtype).type
    s = np.asarray(scales, dtype)
    rq = np.asarray(rot, dtype)
    n2 = rq[:, 0] * rq[:, 0] + rq[:, 1] * rq[:, 1] + rq[:, 2] * rq[:, 2] + rq[:, 3] * rq[:, 3]
    norm = np.sqrt(n2)
    safe = np.where(norm > dt(1e-8), norm, dt(1e-8))
    qw, qx, qy, qz = (rq[:, i] / safe for i in range(4))
    one, two = dt(1.0), dt(2.0)
    R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy)],
         [two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx)],
         [two * (qx * qz - qw * qy), two * (qy * qz + qw * qx), one - two * (qx * qx + qy * qy)]]
    A = [[R[i][k] * s[:, k] for k in range(3)] for i in range(3)]
    c = [[A[i][0] * A[j][0] + A[i][1] * A[j][1] + A[i][2] * A[j][2] for j in range(3)] for i in range(3)]
    return c, R, dict(q=(qw, qx, qy, qz), safe=safe, norm=norm, n2=n2)


def project(scales, rot, means3d, cam, W, H, dtype=np.float64):
    """The geometry of the projection forward under the fisheye model: dict(means2d [N, 2], depths [N], cov2d [N, 2, 2],
    conic [N, 2, 2], radii [N], rectMin [N, 2], rectMax [N, 2], lambdaMax [N]) plus the intermediates the VJP reads."""
    dt = np.dtype(dtype).type
    V = np.asarray(cam["view"], dtype).reshape(16)
    fx, fy = dt(cam["focalX"]), dt(cam["focalY"])
    with np.errstate(all="ignore"):
        pv = view_points(means3d, V, dtype)
        c3, R, rc = _cov3d(scales, rot, dtype)
        J, fm = jacobian(pv[0], pv[1], pv[2], fx, fy, dtype)
        JW = [[J[:, r, 0] * V[4 * k] + J[:, r, 1] * V[4 * k + 1] + J[:, r, 2] * V[4 * k + 2] for k in range(3)] for r in range(2)]
        M = [[JW[r][0] * c3[0][k] + JW[r][1] * c3[1][k] + JW[r][2] * c3[2][k] for k in range(3)] for r in range(2)]
        raw = [[M[r][0] * JW[q][0] + M[r][1] * JW[q][1] + M[r][2] * JW[q][2] for q in range(2)] for r in range(2)]
        cov = [[raw[r][q] + dt(0.3) if r == q else raw[r][q] for q in range(2)] for r in range(2)]
        ox, oy = principal_offset(cam["proj"], W, H, dtype)
        sx = fx * pv[0] * fm[0] + ox
        sy = fy * pv[1] * fm[0] + oy
        det = cov[0][0] * cov[1][1] - cov[0][1] * cov[1][0]
        conic = np.stack([np.stack([cov[1][1] / det, -cov[0][1] / det], -1), np.stack([-cov[1][0] / det, cov[0][0] / det], -1)], -2)
        mid = dt(0.5) * (cov[0][0] + cov[1][1])
        delta = mid * mid - det
        delta = np.where(delta > dt(1e-5), delta, dt(1e-5))
        lam = mid + np.sqrt(delta)
        vis = np.where(pv[2] >= dt(0.2), dt(1.0), dt(0.0))
        radius = dt(3.0) * np.ceil(np.sqrt(lam)) * vis
        maxX, maxY = dt(W) - dt(1.0), dt(H) - dt(1.0)
        rmin = np.stack([np.maximum(sx - radius, dt(0.0)), np.maximum(sy - radius, dt(0.0))], -1)
        rmax = np.stack([np.minimum(sx + radius, maxX), np.minimum(sy + radius, maxY)], -1)
    cov2d = np.stack([np.stack([cov[0][0], cov[0][1]], -1), np.stack([cov[1][0], cov[1][1]], -1)], -2)
    return dict(means2d=np.stack([sx, sy], -1).astype(dtype), depths=pv[2].astype(dtype), cov2d=cov2d.astype(dtype),
                conic=conic.astype(dtype), radii=radius.astype(dtype), rectMin=rmin.astype(dtype), rectMax=rmax.astype(dtype),
                lambdaMax=lam.astype(dtype), _pv=pv, _c3=c3, _R=R, _rc=rc, _J=J, _fm=fm, _JW=JW, _M=M)


def project_vjp(scales, rot, means3d, cam, W, H, cotMeans2d, cotDepths, cotCov2d, cotConic, dtype=np.float64, fwd=None):
    """Cotangents of means2d [N, 2], depths [N], cov2d [N, 2, 2], conic [N, 2, 2] -> dict(gradMeans3d, gradScales, gradRot): the
    geometry's share of the projection backward (the colour path's view-direction term of the means is not part of it)."""
    dt = np.dtype(dtype).type
    f = fwd if fwd is not None else project(scales, rot, means3d, cam, W, H, dtype)
    V = np.asarray(cam["view"], dtype).reshape(16)
    fx, fy = dt(cam["focalX"]), dt(cam["focalY"])
    s = np.asarray(scales, dtype)
    rq = np.asarray(rot, dtype)
    cm = np.asarray(cotMeans2d, dtype).reshape(-1, 2)
    cd = np.asarray(cotDepths, dtype).reshape(-1)
    ccov = np.asarray(cotCov2d, dtype).reshape(-1, 4)
    ccon = np.asarray(cotConic, dtype).reshape(-1, 4)
    two = dt(2.0)
    with np.errstate(all="ignore"):
        c2 = f["cov2d"].reshape(-1, 4)
        c2 = [c2[:, k] for k in range(4)]
        det = c2[0] * c2[3] - c2[1] * c2[2]
        det2 = det * det
        S29, S30, S31, S32 = ccon[:, 3] / det2, ccon[:, 2] / det2, ccon[:, 1] / det2, ccon[:, 0] / det2
        S33 = c2[0] * -S29 + -c2[2] * -S30 + -c2[1] * -S31 + c2[3] * -S32
        S34 = -S33
        dC = [det * S29 + c2[3] * S33, -(det * S31) + c2[2] * S34, -(det * S30) + c2[1] * S34, det * S32 + c2[0] * S33]
        dC = [dC[k] + ccov[:, k] for k in range(4)]
        b = [f["_JW"][0][k] for k in range(3)] + [f["_JW"][1][k] for k in range(3)]
        t = [f["_M"][0][k] for k in range(3)] + [f["_M"][1][k] for k in range(3)]
        c3 = f["_c3"]
        dtt, db = [None] * 6, [None] * 6
        for k in range(3):
            dtt[k] = dC[0] * b[k] + dC[1] * b[3 + k]
            dtt[3 + k] = dC[2] * b[k] + dC[3] * b[3 + k]
            db[k] = dC[0] * t[k] + dC[2] * t[3 + k]
            db[3 + k] = dC[1] * t[k] + dC[3] * t[3 + k]
        dS = [[None] * 3 for _ in range(3)]
        for l in range(3):
            for k in range(3):
                dS[l][k] = b[l] * dtt[k] + b[3 + l] * dtt[3 + k]
            db[l] = db[l] + (dtt[0] * c3[l][0] + dtt[1] * c3[l][1] + dtt[2] * c3[l][2])
            db[3 + l] = db[3 + l] + (dtt[3] * c3[l][0] + dtt[4] * c3[l][1] + dtt[5] * c3[l][2])
        dj = [db[3 * r] * V[a] + db[3 * r + 1] * V[4 + a] + db[3 * r + 2] * V[8 + a] for r in range(2) for a in range(3)]
        x, y, z = f["_pv"]
        dt0, dt1, dt2 = jacobian_vjp(x, y, z, fx, fy, dj, f["_fm"], dtype)
        J = f["_J"]
        dt0 = dt0 + (J[:, 0, 0] * cm[:, 0] + J[:, 1, 0] * cm[:, 1])
        dt1 = dt1 + (J[:, 0, 1] * cm[:, 0] + J[:, 1, 1] * cm[:, 1])
        dt2 = dt2 + (J[:, 0, 2] * cm[:, 0] + J[:, 1, 2] * cm[:, 1] + cd)
        dm = np.stack([V[4 * a] * dt0 + V[4 * a + 1] * dt1 + V[4 * a + 2] * dt2 for a in range(3)], -1)
        # Sigma = L L^T, L = R diag(s)
        R = f["_R"]
        L = [[R[i][j] * s[:, j] for j in range(3)] for i in range(3)]
        dL = [[sum((dS[i][k] + dS[k][i]) * L[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        ds = np.stack([sum(dL[i][j] * R[i][j] for i in range(3)) for j in range(3)], -1)
        dr = [dL[i][j] * s[:, j] for i in range(3) for j in range(3)]
        qw, qx, qy, qz = f["_rc"]["q"]
        four = dt(4.0)
        dqw = two * (-qz * dr[1] + qy * dr[2] + qz * dr[3] - qx * dr[5] - qy * dr[6] + qx * dr[7])
        dqx = two * (qy * dr[1] + qz * dr[2] + qy * dr[3] - qw * dr[5] + qz * dr[6] + qw * dr[7]) - four * qx * (dr[4] + dr[8])
        dqy = two * (qx * dr[1] + qw * dr[2] + qx * dr[3] + qz * dr[5] - qw * dr[6] + qz * dr[7]) - four * qy * (dr[0] + dr[8])
        dqz = two * (-qw * dr[1] + qx * dr[2] + qw * dr[3] + qy * dr[5] + qx * dr[6] + qy * dr[7]) - four * qz * (dr[0] + dr[4])
        sn, norm, n2 = f["_rc"]["safe"], f["_rc"]["norm"], f["_rc"]["n2"]
        dsafe = -(dqw * rq[:, 0] + dqx * rq[:, 1] + dqy * rq[:, 2] + dqz * rq[:, 3]) / (sn * sn)
        tiny = dt(1e-8)
        dnorm = np.where(norm > tiny, dsafe, np.where(norm < tiny, dt(0.0), dt(0.5) * dsafe))
        mx = np.where(n2 > dt(1e-7), n2, dt(1e-7))
        dn2 = dt(0.5) / np.sqrt(mx) * dnorm
        dq = np.stack([d / sn + two * rq[:, i] * dn2 for i, d in enumerate((dqw, dqx, dqy, dqz))], -1)
    return dict(gradMeans3d=dm.astype(dtype), gradScales=ds.astype(dtype), gradRot=dq.astype(dtype))


def lens_theta_d(theta, k):
    """OPENCV_FISHEYE's distorted angle theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)."""
    t2 = theta * theta
    return theta * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


# ---- the scene of tests/test_gpu_fisheye.py (here, so that the CPU suite can check what the GPU tests assume about it) ----------
SCENE_W, SCENE_H, SCENE_N, SCENE_K, SCENE_DEGREE, SCENE_SEED = 64, 48, 300, 16, 3, 5
SCENE_FOCAL, SCENE_PRINCIPAL = (22.0, 21.0), (30.5, 25.25)
HAND_ROWS = dict(on_axis=0, below_series=1, above_series=2, z_below_near=3, z_at_near=4, behind=5, steep=6)


def scene_c2w():
    """The camera at the origin looking along world +x with world z up: a signed permutation, so that view-space coordinates
    are the world's bits and the hand-placed rows sit exactly where they are put."""
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2] = (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)
    return c2w


def scene(seed=SCENE_SEED, N=SCENE_N, K=SCENE_K):
    """Raw parameters (float32) of a cloud around the camera's axis out to about 80 degrees, distances 0.6 .. 3, splats of one
    to a few pixels, with the hand-placed rows HAND_ROWS in front."""
    rng = np.random.default_rng(seed)
    theta = np.deg2rad(rng.uniform(0.0, 80.0, N))
    phi = rng.uniform(0.0, 2.0 * np.pi, N)
    dist = rng.uniform(0.6, 3.0, N)
    pv = np.stack([dist * np.sin(theta) * np.cos(phi), dist * np.sin(theta) * np.sin(phi), dist * np.cos(theta)], -1)
    near = float(np.float32(0.2))
    hand = [(0.0, 0.0, 1.5), (0.3998, 0.0, 2.0), (0.0, 0.4002, 2.0), (0.05, 0.02, float(np.nextafter(np.float32(0.2), np.float32(0.0)))),
            (0.03, -0.04, near), (0.3, -0.2, -1.0), (1.1, 0.3, 0.21)]
    pv[:len(hand)] = hand
    pv = pv.astype(np.float32)
    R = scene_c2w()[:3, :3].astype(np.float32)
    xyz = (pv @ R.T).astype(np.float32)                       # (one non-zero term per sum: exact)
    p = dict(xyz=xyz,
             features_dc=rng.uniform(-0.5, 1.5, (N, 1, 3)),
             features_rest=0.15 * rng.standard_normal((N, K - 1, 3)),
             scales=np.log(rng.uniform(0.02, 0.12, (N, 3)) * dist[:, None]),
             rotation=rng.standard_normal((N, 4)),
             opacity=rng.uniform(-1.0, 2.5, (N, 1)))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, pv


def activated(p, dtype):
    """(scales, rotations) as the renderer activates them: exp, q / (|q| + 1e-8)."""
    dt = np.dtype(dtype).type
    s = np.exp(np.asarray(p["scales"], dtype))
    q = np.asarray(p["rotation"], dtype)
    q = q / (np.sqrt(np.sum(q * q, axis=1, keepdims=True)) + dt(1e-8))
    return s.astype(dtype), q.astype(dtype)
