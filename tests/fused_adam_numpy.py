"""Numpy helpers of tests/test_gpu_fused_adam_elementwise.py and tests/test_fused_adam_numpy_cpu.py: the project's Adam in
float64, the per-element bars an Adam kernel is held to, small scenes whose unfused gradient is bit-reproducible, and a
hand-laid arena whose features_rest segment starts off a 16-byte boundary.  numpy only; nothing here touches a device.

The step (csrc/optim.hip adam_kernel, csrc/projection.hip adam_step; no bias correction):

    gr = g * scale,   m = b1 m0 + (1 - b1) gr,   v = b2 v0 + ((1 - b2) gr) gr,   p = p0 - (lr m) / (sqrt(v) + eps)

b1, b2, 1 - b1, 1 - b2, lr, eps and scale are float32 numbers on the device and are taken at those values here.

The bars are rounding alone, u = 2^-24, F = 2^-125 (a floor: whether the device's float32 multiply-adds keep subnormals is for
the device test to print, not for a bar to assume):

    m   |m - m64| <= 4u (|b1 m0| + |(1 - b1) gr|) + F       gr, two products, the sum
    v   |v - v64| <= 5u v64 + F                             gr twice, two products, the sum; every term is >= 0
    p   from the kernel's OWN stored m and v (the moments are pinned above, so their error does not compound here):
        d64 = lr m / (sqrt(v) + eps) in float64,  |p - (p0 - d64)| <= 8u |d64| + u |p0 - d64| + F
        8u = 4 x 2^-23: gs_adam_delta (csrc/gs_ctx.h) takes the hardware's 1-ulp square root and 1-ulp reciprocal; with the
        add and the two multiplies its worst case is 3.5 x 2^-23, and the subtraction rounds once more at the size of p.
        Where the stored v is subnormal the hardware square root may flush it: the step then lies between the d64 taken with
        sqrt(v) and the d64 taken with 0, each end widened by its own terms.
"""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -125
TINY = 2.0 ** -126                     # the smallest normal float32
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")       # the learning rates' order
DEGREE = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}
SIZES = ((32, 16), (29, 13))           # at most two 16 x 16 blocks: at most two addends per gradAcc16 entry
ADAM = dict(b1=0.9, b2=0.999, eps=1e-15)


def row_floats(K):
    return dict(xyz=3, features_dc=3, features_rest=3 * (K - 1), scales=3, rotation=4, opacity=1)


def row_shape(K):
    return dict(xyz=(3,), features_dc=(1, 3), features_rest=(K - 1, 3), scales=(3,), rotation=(4,), opacity=())


def active_columns(d):
    """The features_rest columns an active degree d moves: 3 ((d + 1)^2 - 1)."""
    return 3 * ((d + 1) ** 2 - 1)


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _consts(lr, b1, b2, eps, scale):
    one = np.float32(1)
    b1, b2 = np.float32(b1), np.float32(b2)
    return (np.asarray(lr, np.float32).astype(np.float64), float(b1), float(b2), float(one - b1), float(one - b2),
            float(np.float32(eps)), float(np.float32(scale)))


def adam64(p0, m0, v0, g, lr, b1, b2, eps, scale):
    """(m64, v64): the moments of the step in float64, on float32 inputs."""
    _, b1, b2, c1, c2, _, scale = _consts(lr, b1, b2, eps, scale)
    gr = _f64(g) * scale
    return b1 * _f64(m0) + c1 * gr, b2 * _f64(v0) + (c2 * gr) * gr


def restate32(p0, m0, v0, g, lr, b1, b2, eps, scale):
    """(p, m, v): the step in IEEE float32, every operation rounded once, correctly rounded sqrt and division."""
    f = np.float32
    p0, m0, v0, g = (np.asarray(a, f) for a in (p0, m0, v0, g))
    lr, b1, b2, eps, scale = np.asarray(lr, f), f(b1), f(b2), f(eps), f(scale)
    with np.errstate(under="ignore"):
        gr = g * scale
        m = b1 * m0 + (f(1) - b1) * gr
        v = b2 * v0 + ((f(1) - b2) * gr) * gr
        p = p0 - (lr * m) / (np.sqrt(v) + eps)
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def bars(p0, m0, v0, g, p, m, v, lr, b1, b2, eps, scale):
    """The bars of the module docstring for a step that left (p, m, v), element by element (arrays of one shape; lr a scalar or
    one rate per element).  Returns m64, v64, bar_m, bar_v, the interval [p_lo, p_hi] and the three ratios error / bar
    (ratio_p: the distance from the interval's middle over its half width); a step passes where every ratio is <= 1."""
    lr64, b1_, b2_, c1, c2, eps_, scale_ = _consts(lr, b1, b2, eps, scale)
    m64, v64 = adam64(p0, m0, v0, g, lr, b1, b2, eps, scale)
    gr = _f64(g) * scale_
    bar_m = 4 * U * (np.abs(b1_ * _f64(m0)) + np.abs(c1 * gr)) + FLOOR
    bar_v = 5 * U * v64 + FLOOR
    P0, P, M, V = _f64(p0), _f64(p), _f64(m), _f64(v)

    def ends(root):
        d = lr64 * M / (root + eps_)
        c = P0 - d
        w = 8 * U * np.abs(d) + U * np.abs(c) + FLOOR
        return c - w, c + w
    with np.errstate(invalid="ignore"):
        lo, hi = ends(np.sqrt(V))
        sub = (V > 0) & (V < TINY)
        if sub.any():
            lo0, hi0 = ends(np.where(sub, 0.0, np.sqrt(V)))
            lo, hi = np.minimum(lo, lo0), np.maximum(hi, hi0)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        out = dict(m64=m64, v64=v64, bar_m=bar_m, bar_v=bar_v, p_lo=lo, p_hi=hi, ratio_m=np.abs(M - m64) / bar_m,
                   ratio_v=np.abs(V - v64) / bar_v, ratio_p=np.abs(P - mid) / half)
    for k in ("ratio_m", "ratio_v", "ratio_p"):          # a NaN or an infinity the step left is beyond every bar
        out[k] = np.where(np.isfinite(out[k]), out[k], np.inf)
    return out


def value_table(lrs=None):
    """Ordinary gradients at which a kernel's arithmetic can go wrong, as float32 arrays p0, m0, v0, g, lr: g = 0 with zero and
    with non-zero moments, |g| = 1e-25 (the square underflows), v0 = 0 with |g| = 1e-20 (a subnormal v), mixed signs with
    b1 m0 close to -(1 - b1) g, a few plain ones -- each at every learning rate (default: the trainer's six at step 0)."""
    if lrs is None:
        lrs = [0.00016, 0.0025, 0.0025 / 20, 0.005, 0.001, 0.025]
    f = np.float32
    c1_b1 = float(f(1) - f(0.9)) / float(f(0.9))
    rows = []                                   # (p0, m0, v0, g)
    for p0 in (0.0, 0.37, -1.9):
        rows += [(p0, 0.0, 0.0, 0.0), (p0, 3e-4, 1e-7, 0.0), (p0, -3e-4, 1e-7, 0.0), (p0, 0.0, 1e-7, 0.0)]
        for s in (1.0, -1.0):
            rows += [(p0, 0.0, 0.0, s * 1e-25), (p0, s * 2e-5, 3e-9, s * 1e-25), (p0, -s * 2e-5, 3e-9, s * 1e-25),
                     (p0, 0.0, 0.0, s * 1e-20), (p0, s * 1e-21, 0.0, s * 1e-20), (p0, 0.0, 0.0, s * 1e-3),
                     (p0, s * 0.2, 0.5, -s * 0.7), (p0, s * 1e-3, 1e-6, s * 1e-3)]
            for g in (1e-3, 0.25, 3e-6):
                for delta in (0.0, 1e-7, -1e-7, 1e-3, -1e-3):
                    rows.append((p0, -s * g * c1_b1 * (1.0 + delta), g * g, s * g))
    t = np.asarray(rows, np.float64)
    n, k = t.shape[0], len(lrs)
    t = np.tile(t, (k, 1)).astype(f)
    lr = np.repeat(np.asarray(lrs, f), n)
    return dict(p0=t[:, 0].copy(), m0=t[:, 1].copy(), v0=t[:, 2].copy(), g=t[:, 3].copy(), lr=lr)


# ------------------------------------------------------------------------------------------------------------------ the scenes
def invisible_set(N, kind, seed=0):
    """Which rows a scene puts behind the camera.  "scattered": about a third, at random (every full wave mixed).  "blocked":
    rows 0 .. 127 (a whole workgroup of the fused backward), 192 .. 255 (a whole wave beside a visible one) and 256 .. 300 (a
    mixed wave), clipped to N."""
    inv = np.zeros(N, bool)
    if kind == "scattered":
        inv = np.random.default_rng(100 + seed).random(N) < 0.35
        inv[:1] = False
    elif kind == "blocked":
        inv[0:128] = True
        inv[192:256] = True
        inv[256:301] = True
    elif kind is not None:
        raise ValueError(kind)
    return inv


def scene(W, H, N, K, seed, invisible=None):
    """(params, [camera A, camera B], invisible): N Gaussians of a few pixels' size in the plane in front of both cameras, spread
    over the W x H image and overlapping several deep, translucent enough for the deep ones to be reached; features_rest adding
    of order 0.05 per band to the colour and a DC term that keeps the colours above the max(., 0) gate.  The rows of `invisible` (invisible_set) stand
    behind both cameras: the projection gives them radius 0 and nothing else does."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    assert (W, H) in SIZES and K in DEGREE
    rng = np.random.default_rng(seed)
    f, dist = 40.0, 4.0
    cams = [Camera(W, H, f, f, look_at_c2w([0.0, -dist, 0.0])), Camera(W, H, f, f * 1.02, look_at_c2w([0.5, -3.9, 0.3]))]
    hx, hz = 0.5 * W / f * dist, 0.5 * H / f * dist
    xyz = np.stack([rng.uniform(-0.85 * hx, 0.85 * hx, N), rng.uniform(-0.3, 0.3, N), rng.uniform(-0.8 * hz, 0.8 * hz, N)], 1)
    inv = invisible_set(N, invisible, seed)
    xyz[inv, 1] -= 2.0 * dist
    # (the SH direction xyz - camera is not normalised: band l's basis is of order dist^l, so its coefficients are 0.05 / dist^l
    # and every band adds of order 0.05 to the colour)
    band = np.floor(np.sqrt(np.arange(1, K))).astype(np.int64)
    rest = rng.normal(0, 0.05, (N, K - 1, 3)) / (dist ** band)[None, :, None]
    p = dict(xyz=xyz, features_dc=rng.normal(0.6, 0.6, (N, 1, 3)), features_rest=rest,
             scales=rng.normal(np.log(0.2), 0.3, (N, 3)), rotation=rng.normal(0, 1, (N, 4)), opacity=rng.normal(-2.0, 0.5, N))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, cams, inv


def cotangent(W, H, seed=3):
    """A dense random colour cotangent [H, W, 3], of the size a mean loss gives."""
    return (np.random.default_rng(seed).standard_normal((H, W, 3)) / (W * H)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the arenas
def carve(buf, starts, N, K):
    """The six tensors as views of a flat buffer (numpy array or torch tensor), tensor k from float starts[k]."""
    per, shape = row_floats(K), row_shape(K)
    return {k: buf[starts[k]:starts[k] + N * per[k]].reshape((N,) + shape[k]) for k in KEYS}


def tensor_ids(numel, starts, N, K):
    """Per arena element the index into KEYS of the tensor it belongs to, -1 for an element of none."""
    ids = np.full(numel, -1, np.int8)
    per = row_floats(K)
    for i, k in enumerate(KEYS):
        assert (ids[starts[k]:starts[k] + N * per[k]] == -1).all() and starts[k] + N * per[k] <= numel, k
        ids[starts[k]:starts[k] + N * per[k]] = i
    return ids


def hand_arena(p, N, K, offsets, seed=9):
    """Parameter, m and v buffers laid out by hand.  offsets: the residue 1, 2 or 3 of the features_rest segment's float offset
    modulo 4 (the other five tensors are strewn around it, gaps between them), or a dict of all six float offsets.  The
    parameters are p's; the moments are zero and every element of no tensor holds a random value, in all three buffers.
    Returns dict(arena, m, v, views, starts, mask, numel): views[name][k] alias the buffers, mask is True on the elements
    that belong to a tensor."""
    per = row_floats(K)
    if isinstance(offsets, dict):
        starts = {k: int(offsets[k]) for k in KEYS}
    else:
        res = int(offsets)
        assert res in (1, 2, 3)
        starts, off = {}, 5
        for k in ("opacity", "rotation", "features_rest", "xyz", "features_dc", "scales"):
            if k == "features_rest":
                off += (res - off) % 4
            starts[k] = off
            off += N * per[k] + {"opacity": 3, "rotation": 1, "features_rest": 2, "xyz": 0, "features_dc": 5, "scales": 7}[k]
    numel = max(starts[k] + N * per[k] for k in KEYS) + 7
    numel += -numel % 4
    ids = tensor_ids(numel, starts, N, K)
    mask = ids >= 0
    rng = np.random.default_rng(seed)
    out = dict(starts=starts, mask=mask, numel=numel, ids=ids, views={})
    for name in ("arena", "m", "v"):
        buf = np.zeros(numel, np.float32)
        buf[~mask] = rng.normal(0, 1, int((~mask).sum())).astype(np.float32)
        out[name] = buf
        out["views"][name] = carve(buf, starts, N, K)
    for k in KEYS:
        out["views"]["arena"][k][...] = np.asarray(p[k], np.float32).reshape(out["views"]["arena"][k].shape)
    return out


def scatter(tensors, numel, starts, N, K, fill=0.0):
    """A flat float32 buffer of the layout `starts` holding the six tensors (gradients, say), `fill` elsewhere."""
    buf = np.full(numel, fill, np.float32)
    views = carve(buf, starts, N, K)
    for k in KEYS:
        views[k][...] = np.asarray(tensors[k], np.float32).reshape(views[k].shape)
    return buf


def rest_columns(ids, starts, N, K):
    """Per arena element its features_rest column, -1 outside features_rest."""
    col = np.full(ids.shape[0], -1, np.int32)
    L = 3 * (K - 1)
    if L:
        col[starts["features_rest"]:starts["features_rest"] + N * L] = np.tile(np.arange(L, dtype=np.int32), N)
    return col


def element_rows(ids, starts, N, K):
    """Per arena element the Gaussian it belongs to, -1 for an element of no tensor."""
    row = np.full(ids.shape[0], -1, np.int64)
    per = row_floats(K)
    for k in KEYS:
        row[starts[k]:starts[k] + N * per[k]] = np.repeat(np.arange(N, dtype=np.int64), per[k])
    return row


def start_moments(g_flat, ids, seed):
    """Random non-zero moments at the size of the gradient, per tensor: m signed, v in [0.01, 1] times the square of the
    tensor's largest |g|; elsewhere random values of order one (a stray load or store shows)."""
    rng = np.random.default_rng(seed)
    n = g_flat.shape[0]
    m, v = rng.normal(0, 1, n), rng.uniform(0.01, 1.0, n)
    for i in range(len(KEYS)):
        sel = ids == i
        if sel.any():
            s = float(np.abs(g_flat[sel]).max()) or 1.0          # (degree 0 gives features_rest no gradient at all)
            m[sel] *= 0.5 * s
            v[sel] *= s * s
    return m.astype(np.float32), v.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
