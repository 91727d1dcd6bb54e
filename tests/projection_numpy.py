"""The edge-case cloud and the row-wise measure that tests/test_projection_numpy_cpu.py and tests/test_gpu_projection_rows.py
hold the pinhole projection (project_geometry, project_geometry_bwd, color_backward) to.  Pure numpy plus oracle.oracle.

The cloud is built in VIEW space, group by group, and mapped back through the inverse view matrix (row vectors: pv = [m, 1] @ V),
so that every group sits where the arithmetic changes: on either side of the EWA clamp (build_cov2d clamps the DEPTH against
limX = 1.3 tan(fovX / 2) and limY, the reference's quirk), around the z >= 0.2 visibility plane, behind the camera, within 1e-4
of the camera plane, off the screen, needle-shaped, isotropic, with a tiny or a huge raw quaternion, and below a pixel.  The
groups are contiguous and their sizes are no multiples of 64, so they straddle waves; N = 631 is no multiple of 64 or 128.

The measure is per Gaussian: row_error = max|got - want| / max|want| over one row of a tensor.  Nothing is taken from the
tensor's largest entry, which in a cloud that mixes close-ups with distant splats is a hundred times a typical row's.

BARS holds the bar of every (tensor, group): 2e-4 (the project's rtol for these tensors) wherever the float32 oracle stays
within half of it against the float64 oracle, else four times the float32 oracle's worst row error of that group, never above
1e-3.  tests/test_projection_numpy_cpu.py asserts that qualification; the GPU file holds the kernels to the same numbers.
"""
import numpy as np

W, H = 200, 152
SEED = 7
GROUPS = (("far", 97), ("inside_clamp", 97), ("between_lims", 33), ("near_plane", 64), ("behind", 33), ("plane_zero", 16),
          ("offscreen", 64), ("needle", 64), ("isotropic", 33), ("tiny_q", 33), ("big_q", 33), ("subpixel", 64))
N_TOTAL = sum(n for _, n in GROUPS)
CASES = ((25, 4), (25, 2), (16, 3), (9, 2), (4, 1), (1, 0))          # (K, degree) of the op-level and the CPU walks
FORWARD_ROWWISE = ("color", "cov2d", "conic")
BACKWARD = ("gradScales", "gradRot", "gradMeans3d", "gradShs", "gradCamCenterPoint")
RTOL = 2e-4              # test_projection_forward_backward's rtol for the five gradients
CAP = 1e-3

# (tensor, group) -> bar, where 2e-4 does not hold: 4 x the float32 oracle's worst row error over CASES.  Nothing here may
# exceed CAP.  Fed the same activated bits, the float32 oracle's worst row error against the float64 one is 2.7e-5 (colour,
# far) over every tensor, group and case (the table in tests/test_gpu_projection_rows.py), so 2e-4 holds everywhere and the
# table of exceptions is empty.
BARS = {}
# isotropic gradRot is zero but for rounding (Sigma = s^2 I whatever the rotation): held absolutely, to four times the float32
# oracle's largest |gradRot| in the group (2^-11 = 4.9e-4, where the other groups' rows are of the order of 100).
ISOTROPIC_GRADROT_ABS = 4 * 2.0 ** -11


def bar(tensor, group):
    return BARS.get((tensor, group), RTOL)


def camera():
    """test_gpu_parity._scene's camera."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    focal = 0.9 * W
    return Camera(W, H, focal, focal * 1.02, look_at_c2w([2.2, -2.6, 1.7]))


def limits(cam):
    """(limX, limY) as make_cam forms them: tanf(fov / 2) * 1.3f."""
    f = np.float32
    return (float(np.tan(f(cam.FoVx) * f(0.5), dtype=f) * f(1.3)), float(np.tan(f(cam.FoVy) * f(0.5), dtype=f) * f(1.3)))


def group_rows(groups, name):
    return np.flatnonzero(groups == name)


def edge_cloud(seed=SEED, K=25):
    """(raw parameters, group name per row, camera, cotangents).  The geometry does not depend on K: every K sees the same
    rows, and features_rest of a smaller K is the leading part of a larger one's."""
    cam = camera()
    limX, limY = limits(cam)
    lo = min(limX, limY)
    rng = np.random.default_rng(seed)
    V = np.asarray(cam.worldViewTransform, np.float64)
    view, scales, rot, names = [], [], [], []
    for name, n in GROUPS:
        zr = dict(inside_clamp=(0.21, 0.98 * lo), between_lims=(1.01 * limY, 0.99 * limX), near_plane=(0.15, 0.25),
                  behind=(-3.0, -0.05), plane_zero=(-1e-4, 1e-4), far=(2.0, 6.0)).get(name, (2.0, 5.0))
        z = rng.uniform(zr[0], zr[1], n)
        u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
        if name == "offscreen":
            u = rng.choice([-1.0, 1.0], n) * rng.uniform(0.8, 1.6, n)
        # plane_zero: x = u z would put the whole point on the camera centre; it is spread over the plane instead
        zz = np.ones(n) if name == "plane_zero" else z
        view.append(np.stack([u * zz, v * zz * H / W, z], 1))
        mu, sd = dict(inside_clamp=(0.01, 0.5), needle=(0.05, 1.2), subpixel=(1e-4, 0.3)).get(name, (0.05, 0.5))
        s = rng.normal(np.log(mu), sd, (n, 3))
        if name == "isotropic":
            s = np.repeat(s[:, :1], 3, 1)
        scales.append(s)
        rot.append(rng.normal(0, 1, (n, 4)) * dict(tiny_q=1e-3, big_q=1e3).get(name, 1.0))
        names += [name] * n
    pv = np.concatenate(view)
    N = pv.shape[0]
    xyz = (pv - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    rest = rng.normal(0, 0.3, (N, 24, 3))[:, :K - 1]
    p = dict(xyz=xyz, features_dc=rng.normal(0, 1, (N, 1, 3)), features_rest=rest, scales=np.concatenate(scales),
             rotation=np.concatenate(rot), opacity=rng.normal(0.3, 1.5, N))
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    cots = dict(means2d=rng.normal(size=(N, 2)), depths=rng.normal(size=N), color=rng.normal(size=(N, 3)),
                cov2d=rng.normal(size=(N, 2, 2)), conic=rng.normal(size=(N, 2, 2)) * 100)
    cots = {k: np.ascontiguousarray(v, np.float32) for k, v in cots.items()}
    assert all(np.abs(v).min() > 0 for v in cots.values())
    assert N == N_TOTAL and N % 64 and all(n % 64 or n == 64 for _, n in GROUPS)
    return p, np.array(names), cam, cots


def shs_of(p):
    return np.concatenate([p["features_dc"], p["features_rest"]], 1)


def walk(o, sc, rt, p, cam, cots, degree, rows=None):
    """(projection_forward, projection_backward) of oracle `o` from the given ACTIVATED scales and rotations (cast to the
    oracle's precision: both precisions then see the same bits) on the first `rows` rows."""
    c = cam.as_dict()
    s = slice(0, rows)
    args = (sc[s], rt[s], p["xyz"][s], shs_of(p)[s], c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"], c["focalX"],
            c["focalY"], W, H, degree)
    with np.errstate(all="ignore"):
        fw = o.projection_forward(*args)
        bw = o.projection_backward(*args, cots["depths"][s], cots["means2d"][s], cots["cov2d"][s], cots["color"][s],
                                   cots["conic"][s])
    return fw, bw


def row_error(got, want64):
    """Per row of a tensor max|got - want| / max|want| over that row.  A row the reference leaves all zero: 0 where `got` is
    all zero too, inf otherwise."""
    want = np.asarray(want64, np.float64)
    want = want.reshape(want.shape[0], -1)
    got = np.asarray(got, np.float64).reshape(want.shape)
    with np.errstate(all="ignore"):
        err, size = np.abs(got - want).max(1), np.abs(want).max(1)
        return np.where(size > 0, err / size, np.where(err > 0, np.inf, 0.0))


def worst_by_group(got, want64, groups):
    """{group: (worst row error, its row)} over the rows of `got` (the leading rows of the cloud)."""
    e = row_error(got, want64)
    g = groups[:e.shape[0]]
    out = {}
    for name in dict.fromkeys(g):
        rows = np.flatnonzero(g == name)
        bad = ~np.isfinite(e[rows])
        i = rows[np.argmax(bad)] if bad.any() else rows[np.argmax(e[rows])]
        out[name] = (float(e[i]), int(i))
    return out


def near_integer_sqrt_lambda(fw64):
    """Rows whose float64 sqrt(lambdaMax) lies within 1e-4 of an integer: the only rows whose radius 3 ceil(sqrt(lambdaMax))
    two correct float32 evaluations may disagree on."""
    c = np.asarray(fw64["cov2d"], np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        det = c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2]
        mid = 0.5 * (c[:, 0] + c[:, 3])
        root = np.sqrt(mid + np.sqrt(np.maximum(mid * mid - det, 1e-5)))
        return np.abs(root - np.round(root)) < 1e-4


def delta_of(fw):
    c = np.asarray(fw["cov2d"], np.float64).reshape(-1, 4)
    mid = 0.5 * (c[:, 0] + c[:, 3])
    return mid * mid - (c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2])


def assert_cloud_does_its_job(p, groups, cam, fw64, sc, degree):
    """Every group's intended condition holds on at least 80 % of its rows in the float64 forward `fw64` (sc: the activated
    scales it ran on); near_plane has at least 8 rows on each side of the plane; between a tenth and six tenths of the colour
    channels sit on the zero side of max(c + 0.5, 0) wherever a band above the constant one is on (degree 0 alone puts
    c = 0.282 N(0, 1) + 0.5 below zero 3.8 % of the time: there both sides must merely be present)."""
    limX, limY = limits(cam)
    lo, hi = min(limX, limY), max(limX, limY)
    z, rad = np.asarray(fw64["depths"]), np.asarray(fw64["radii"])
    sx = np.asarray(fw64["means2d"])[:, 0]
    rmin, rmax = np.asarray(fw64["rectMin"]), np.asarray(fw64["rectMax"])
    qn = np.linalg.norm(p["rotation"].astype(np.float64), axis=1)
    ratio = sc.max(1).astype(np.float64) / sc.min(1)
    delta = delta_of(fw64)
    cond = dict(far=(z > hi) & (rad > 0), inside_clamp=(z >= 0.2) & (z <= lo) & (rad > 0),
                between_lims=(z > limY) & (z < limX) & (rad > 0), near_plane=(z > 0.14) & (z < 0.26), behind=(z < 0) & (rad == 0),
                plane_zero=(np.abs(z) < 2e-4) & (rad == 0), offscreen=(rad > 0) & ((sx < 0) | (sx > W - 1)) & (z > hi),
                needle=(ratio >= 2) & (rad > 0), isotropic=(ratio == 1) & (rad > 0), tiny_q=(qn < 1e-2) & (rad > 0),
                big_q=(qn > 1e2) & (rad > 0), subpixel=(delta <= 1e-5) & (rad == 3))
    assert limY < limX
    for name, n in GROUPS:
        rows = group_rows(groups, name)
        assert rows.size == n and cond[name][rows].mean() >= 0.8, (name, float(cond[name][rows].mean()))
    near = group_rows(groups, "near_plane")
    assert (z[near] >= 0.2).sum() >= 8 and (z[near] < 0.2).sum() >= 8
    assert np.array_equal(rad[near] > 0, z[near] >= 0.2)
    off = group_rows(groups, "offscreen")
    empty = (rmin[off, 0] > rmax[off, 0]) & (rad[off] > 0)
    assert empty.sum() >= 8, int(empty.sum())
    needle = group_rows(groups, "needle")
    assert np.median(ratio[needle]) >= 5
    for k in ("means2d", "depths", "color", "cov2d", "conic", "radii"):
        assert np.isfinite(np.asarray(fw64[k])[groups != "plane_zero"]).all(), k
    zero = float((np.asarray(fw64["color"]) == 0).mean())
    if degree > 0:
        assert 0.1 <= zero <= 0.6, zero
    else:
        assert 0 < zero < 1, zero
    return dict(colour_channels_at_zero=zero, offscreen_empty_rects=int(empty.sum()))


def bar_shares(got, want64, groups, tensors, skip=("plane_zero",)):
    """{(tensor, group): (worst row error / bar, row)} over the tensors; isotropic gradRot absolutely."""
    out = {}
    for t in tensors:
        for g, (e, i) in worst_by_group(got[t], want64[t], groups).items():
            if g in skip:
                continue
            if t == "gradRot" and g == "isotropic":
                rows = np.flatnonzero(groups[:np.asarray(got[t]).shape[0]] == g)
                a = np.abs(np.asarray(got[t], np.float64)[rows] - np.asarray(want64[t], np.float64)[rows]).max(1)
                out[(t, g)] = (float(a.max() / ISOTROPIC_GRADROT_ABS), int(rows[np.argmax(a)]))
            else:
                out[(t, g)] = (e / bar(t, g), i)
    return out
