"""The training loss (csrc/ssim.hip loss_fused_kernel, launch_loss) stated in float64 numpy, the images
the loss kernels are held to it on, and the bars.

The statement: the eleven taps as gs_ssim_window and launch_loss build them (float32: centre 5.5, exp(-d^2 / 4.5), summed in
order, divided by the sum; the 2-D window their float32 outer product), the 121-tap zero-padded window sums of R, G, R R,
G G, R G, the SSIM quotient, loss = (1 - lambda) mean|R - G| + lambda (1 - mean ssim), and the cotangent of that with
respect to R with sign(0) = 0.  Everything after the taps is float64.  It agrees with Oracle(np.float64) to 1e-12
(tests/test_loss_numpy_cpu.py), so it says nothing the oracle does not; what it adds is MISTAKES: six deliberate errors of
the kind a tiled kernel makes, each behind a switch, with which the CPU test shows that the images and the bars reject them.

The bars (`bars`): a quantity q of the kernel is held to the float64 oracle's q64 with what float32 arithmetic is allowed to
cost taken from the float32 oracle ON THE SAME PAIR, err32 = |q32 - q64|:
    colour cotangent   max|q - q64| <= FACTOR err32 + GRAD_RTOL u,    u = (1 - lambda) / (3 P)
    loss, L1, ssim     |q - q64|    <= FACTOR err32 + ABS_FLOOR
FACTOR = 1.5 is _elementwise_gradient_bar's and test_gpu_trajectory's "no worse than float32 arithmetic allows"; ABS_FLOOR =
2e-6 is test_loss_forward_backward's absolute bar; GRAD_RTOL = 1e-3 is test_gpu_parity's, and times u -- the size of the L1
term at a pixel -- it is a thousandth of the smallest non-zero cotangent the L1 term hands any pixel."""
import numpy as np

K, PAD = 11, 5
C1, C2 = 1e-4, 9e-4
LAMBDA = 0.2
TILE = 32                       # loss_fused_kernel's TX = TY
FACTOR, ABS_FLOOR, GRAD_RTOL = 1.5, 2e-6, 1e-3
SEED = 11

MISTAKES = ("border_clamped", "taps_centred", "sign_zero_negative", "target_stats_shifted", "ssim_mean_padded",
            "backward_unflipped")


# ---- the float64 statement ---------------------------------------------------------------------------------------------
def taps(centre=5.5):
    """The eleven float32 taps of gs_ssim_window / launch_loss.  (expf is taken as the float32 rounding of the float64
    exponential: the CPU test compares the window with the oracle's, bit for bit.)"""
    f = np.float32
    g = np.empty(K, f)
    s = f(0)
    for x in range(K):
        d = f(x) - f(centre)
        g[x] = f(np.exp(np.float64(-(d * d) / f(4.5))))
        s = f(s + g[x])
    return (g / s).astype(f)


def window(centre=5.5):
    """[11, 11] float64: the float32 outer product of the taps, widened."""
    g = taps(centre)
    return (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)


def _window_sums(plane, win, clamp_border=False):
    """sum_ij win[i, j] plane[h + i - 5, w + j - 5]; outside the image the plane is zero (or, the mistake, its nearest pixel)."""
    H, W = plane.shape
    p = np.pad(plane, PAD, mode="edge" if clamp_border else "constant")
    out = np.zeros((H, W))
    for i in range(K):
        for j in range(K):
            out += win[i, j] * p[i:i + H, j:j + W]
    return out


def _gather(d, win, unflipped=False):
    """The adjoint of _window_sums: pixel (h, w) gathers centre (h - i + 5, w - j + 5) with weight win[i, j] (the mistake: the
    forward's own (h + i - 5, w + j - 5)); centres outside the image give nothing."""
    H, W = d.shape
    p = np.pad(d, PAD, mode="constant")
    out = np.zeros((H, W))
    for i in range(K):
        for j in range(K):
            a, b = (i, j) if unflipped else (2 * PAD - i, 2 * PAD - j)
            out += win[i, j] * p[a:a + H, b:b + W]
    return out


def loss_statement(render, target, lam=LAMBDA, mistake=None):
    """dict(loss, l1, ssim, cot [H, W, 3]) in float64; mistake: None or one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES, mistake
    r, t = np.asarray(render, np.float64), np.asarray(target, np.float64)
    H, W, C = r.shape
    n3 = float(H * W * C)
    win = window(5.0 if mistake == "taps_centred" else 5.5)
    up, l1w = -lam / n3, (1.0 - lam) / n3
    cot = np.empty_like(r)
    ssim_sum = 0.0
    for c in range(C):
        x, y = r[..., c], t[..., c]
        m1, m2, e11, e22, e12 = (_window_sums(p, win, mistake == "border_clamped") for p in (x, y, x * x, y * y, x * y))
        if mistake == "target_stats_shifted":           # the target's mean and mean of squares read at (h, w + 1)
            col = np.minimum(np.arange(W) + 1, W - 1)
            m2, e22 = m2[:, col], e22[:, col]
        s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
        a, b = 2.0 * m1 * m2 + C1, 2.0 * s12 + C2
        cc, d = m1 * m1 + m2 * m2 + C1, s1 + s2 + C2
        num, den = a * b, cc * d
        ssim_sum += float((num / den).sum())
        dnum, dden = up / den, -up * num / (den * den)
        da, db, dc, dd = dnum * b, dnum * a, dden * d, dden * cc
        de11, de12 = dd, 2.0 * db
        dm1 = da * 2.0 * m2 + dc * 2.0 * m1 - dd * 2.0 * m1 - de12 * m2
        A, B, Cq = (_gather(p, win, mistake == "backward_unflipped") for p in (dm1, de11, de12))
        diff = x - y
        sign = np.sign(diff)
        if mistake == "sign_zero_negative":
            sign = np.where(diff > 0, 1.0, -1.0)
        cot[..., c] = A + 2.0 * x * B + y * Cq + l1w * sign
    if mistake == "ssim_mean_padded":                    # every centre of every TILE x TILE tile counted: those beyond the
        hp, wp = -(-H // TILE) * TILE, -(-W // TILE) * TILE     # image have zero statistics, ssim = C1 C2 / (C1 C2) = 1
        ssim_sum += float((hp * wp - H * W) * C)
    l1, ssim = float(np.abs(r - t).sum()) / n3, ssim_sum / n3
    return dict(loss=(1.0 - lam) * l1 + lam * (1.0 - ssim), l1=l1, ssim=ssim, cot=cot)


def mistake_can_act(mistake, H, W, render, target):
    """Whether a mistake changes anything at this shape / on this pair at all (the issue's list)."""
    if mistake == "ssim_mean_padded":
        return H % TILE != 0 or W % TILE != 0
    if mistake == "sign_zero_negative":
        return bool((np.asarray(render) == np.asarray(target)).any())
    return True


# ---- the bars ------------------------------------------------------------------------------------------------------------
def unit(shape, lam=LAMBDA):
    """u = (1 - lambda) / (3 P): the size of the L1 term of the cotangent at a pixel."""
    return (1.0 - lam) / float(np.prod(shape))


def oracle_result(oracle, render, target, lam=LAMBDA):
    loss, cot, _, l1, ssim = oracle.loss_forward_backward(np.asarray(render, oracle.dtype), np.asarray(target, oracle.dtype), lam)
    return dict(loss=loss, l1=l1, ssim=ssim, cot=np.asarray(cot, np.float64))


def bars(got, ref64, ref32, lam=LAMBDA, factor=FACTOR):
    """{quantity: (error of `got` against ref64, err32 = the float32 oracle's, the allowance)} for loss, l1, ssim, cot.
    got / ref64 / ref32: dict(loss, l1, ssim, cot)."""
    out = {}
    for k in ("loss", "l1", "ssim"):
        e32 = abs(float(ref32[k]) - float(ref64[k]))
        out[k] = (abs(float(got[k]) - float(ref64[k])), e32, factor * e32 + ABS_FLOOR)
    c64 = np.asarray(ref64["cot"], np.float64)
    e32 = float(np.abs(np.asarray(ref32["cot"], np.float64) - c64).max())
    err = float(np.abs(np.asarray(got["cot"], np.float64) - c64).max())
    out["cot"] = (err, e32, factor * e32 + GRAD_RTOL * unit(c64.shape, lam))
    return out


def map_bar(got, want64, want32, floor, factor=FACTOR):
    """(error, err32, allowance) of one array against the float64 one: max|q - q64| <= factor err32 + floor."""
    w64 = np.asarray(want64, np.float64)
    e32 = float(np.abs(np.asarray(want32, np.float64) - w64).max())
    return float(np.abs(np.asarray(got, np.float64) - w64).max()), e32, factor * e32 + floor


def misses(b):
    """The quantities beyond their allowance (a NaN is beyond any)."""
    return [k for k, (err, _, allow) in b.items() if not err <= allow]


# ---- the images ------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def blobs(H, W, seed):
    """A dozen isotropic Gaussians of width 2-12 px and random colour, summed and clipped to [0, 1]: float64 [H, W, 3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3))
    for _ in range(12):
        cx, cy, s = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 12)
        img += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))[..., None] * rng.uniform(0, 1, 3)
    return np.clip(img, 0, 1)


def _near(img, seed, sd=0.02):
    """img + sd noise, clipped."""
    return np.clip(img + np.random.default_rng(seed + 1000).normal(0, sd, img.shape), 0, 1)


def noise(H, W, seed):
    """The control: what the suite had.  Every window has variance near 0.08."""
    a = np.random.default_rng(seed).uniform(0, 1, (H, W, 3))
    return _f32(a), _f32(_near(a, seed))


def flat_equal(H, W, seed):
    """A converged flat background: sigma = E[x^2] - mu^2 cancels to nothing, d == 0 everywhere, the cotangent is zero."""
    return _f32(np.full((H, W, 3), 0.5)), _f32(np.full((H, W, 3), 0.5))


def white_equal(H, W, seed):
    """The same at exact 1.0 (a white background rendered exactly)."""
    return _f32(np.ones((H, W, 3))), _f32(np.ones((H, W, 3)))


def flat_vs_flat(H, W, seed):
    """Zero variance in both, different means: the quotient is all C2 / C2, and float32's 121-tap sums are 6e-5 off in the loss."""
    return _f32(np.full((H, W, 3), 0.5)), _f32(np.full((H, W, 3), 0.7))


def zeros_vs_blobs(H, W, seed):
    """Iteration 0: a black render against a real target."""
    return _f32(np.zeros((H, W, 3))), _f32(blobs(H, W, seed))


def white_bg(H, W, seed):
    """Dark blobs on an exactly white background (the lower half of the blob values is cut to nothing: half the image is exact
    1.0), against the same plus 0.02 noise (clipped: half the background equal)."""
    b = blobs(H, W, seed)
    a = 1.0 - np.where(b < np.median(b), 0.0, b)
    return _f32(a), _f32(_near(a, seed))


def blobs_near(H, W, seed):
    """Late in training: a smooth render within 0.02 of its target; black where no blob reaches."""
    a = blobs(H, W, seed)
    return _f32(a), _f32(_near(a, seed))


def blobs_vs_blobs(H, W, seed):
    """Early in training: two unrelated smooth images."""
    return _f32(blobs(H, W, seed)), _f32(blobs(H, W, seed + 1))


def ramp(H, W, seed):
    """Gradients along x, y and the diagonal, against the same plus 0.02 noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([xx / W, yy / H, (xx + yy) / (W + H)], -1)
    return _f32(a), _f32(_near(a, seed))


def step_column(W):
    """The column the step edge stands on: 32, the first tile seam, wherever the image is wider than a tile."""
    return TILE if W > TILE else W // 2


def step_edge(H, W, seed):
    """0 left of step_column(W), 1 from it on; the target's step one pixel further right.  All pixels but one column equal."""
    a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    a[:, step_column(W):] = 1.0
    b[:, step_column(W) + 1:] = 1.0
    return _f32(a), _f32(b)


def saturated(H, W, seed):
    """Blobs scaled until half their values clip at 1, against the same + 0.01 clipped: equal where both clip, 0.01 apart below."""
    a = blobs(H, W, seed)
    a = np.clip(a / np.median(a), 0, 1)
    return _f32(a), _f32(np.clip(a + 0.01, 0, 1))


def out_of_range(H, W, seed):
    """Exposure output beyond [0, 1]: metrics_numpy.ramp_pair's ramp from -0.3 to 1.3 plus 0.05 noise (the loss does not clamp)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    base = np.stack([u, v, 0.5 * (u + v)], -1) * 1.6 - 0.3
    return _f32(base + 0.05 * rng.standard_normal((H, W, 3))), _f32(base + 0.05 * rng.standard_normal((H, W, 3)))


ZERO_BAND = (27, 38)            # columns 27 ... 37: across the tile seam at 32


def zero_band(H, W, seed):
    """blobs_near with exact zeros in both images over columns 27 ... 37: what a zero mask makes of the inputs, across a seam."""
    a, b = blobs_near(H, W, seed)
    a[:, ZERO_BAND[0]:ZERO_BAND[1]] = 0
    b[:, ZERO_BAND[0]:ZERO_BAND[1]] = 0
    return a, b


PAIRS = dict(noise=noise, flat_equal=flat_equal, white_equal=white_equal, flat_vs_flat=flat_vs_flat,
             zeros_vs_blobs=zeros_vs_blobs, white_bg=white_bg, blobs_near=blobs_near, blobs_vs_blobs=blobs_vs_blobs, ramp=ramp,
             step_edge=step_edge, saturated=saturated, out_of_range=out_of_range, zero_band=zero_band)
EQUAL_PAIRS = ("flat_equal", "white_equal")

# (H, W): what it exercises of loss_fused_kernel (TX = TY = 32, halo 20, grid 8 * 3 * ceil(tiles / 8))
SHAPES_ALL_PAIRS = [(45, 70), (33, 65), (97, 161)]        # generic partial tiles; one-pixel partial tiles; 24 tiles, perXcd = 3 exact
SHAPES_FEW_PAIRS = [(7, 9),                                # smaller than the window
                    (5, 200), (200, 5),                    # thinner than the window, seven tiles long
                    (32, 32),                              # one exact tile; 21 of 24 workgroups idle
                    (64, 96),                              # exact 2 x 3
                    (96, 96),                              # nine tiles; perXcd = 2, seven empty slots
                    (129, 161)]                            # 30 tiles; two empty slots
FEW_PAIRS = ("noise", "blobs_near", "white_bg", "flat_equal")
CASES = [(H, W, n) for (H, W) in SHAPES_ALL_PAIRS for n in PAIRS] + [(H, W, n) for (H, W) in SHAPES_FEW_PAIRS for n in FEW_PAIRS]

_refs = {}


def reference(oracle32, oracle64, name, H, W, seed=SEED, images_only=False):
    """dict(render, target, ref32, ref64) of one pair at one shape: computed once, shared, read-only.  images_only: (render, target)."""
    key = (name, H, W, seed)
    if key not in _refs:
        render, target = PAIRS[name](H, W, seed)
        ref = dict(render=render, target=target, ref32=oracle_result(oracle32, render, target),
                   ref64=oracle_result(oracle64, render, target))
        for a in (render, target, ref["ref32"]["cot"], ref["ref64"]["cot"]):
            a.setflags(write=False)
        _refs[key] = ref
    return (_refs[key]["render"], _refs[key]["target"]) if images_only else _refs[key]


# ---- the op-level ssim / ssimVJP -------------------------------------------------------------------------------------------
SHAPES_SSIM_OP = [(45, 70), (33, 65)]
SSIM_MAPS = ("ssim", "mu1", "mu2", "sigma1", "sigma2", "sigma12")


def ssim_upstream(H, W):
    """The random upstream of the ssimVJP test, float32 [H, W, 3]."""
    return np.random.default_rng(H * 1000 + W).normal(size=(H, W, 3)).astype(np.float32)


def ssim_maps(oracle, a, b):
    """The six forward maps in the oracle's precision."""
    return oracle.ssim_forward(np.asarray(a, oracle.dtype), np.asarray(b, oracle.dtype))


def ssim_gradients(oracle, a, b, up):
    """(g1, g2) of the op-level ssim under `up` in the oracle's precision, from that oracle's own saved maps: float64 arrays."""
    a, b, up = (np.asarray(x, oracle.dtype) for x in (a, b, up))
    g1, g2 = oracle.ssim_backward(up, a, b, oracle.ssim_forward(a, b)[1:])
    return np.asarray(g1, np.float64), np.asarray(g2, np.float64)
