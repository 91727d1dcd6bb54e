"""Lens undistortion in float64 (include/gsplat.h gs_undistort): a view taken through OpenCV's / COLMAP's
radial-tangential lens, resampled into a pinhole camera once when a dataset is loaded.

    model        r2 = x^2 + y^2,  radial = 1 + k1 r2 + k2 r2^2,
                 xd = x radial + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y radial + p1 (r2 + 2 y^2) + 2 p2 x y
    sample       destination pixel (i, j) of the pinhole (nfx, nfy, ncx, ncy): x = (i + 0.5 - ncx) / nfx, y = (j + 0.5 - ncy) / nfy,
                 distort, u = fx xd + cx, v = fy yd + cy, sample position (su, sv) = (u - 0.5, v - 0.5): pixel i covers
                 [i, i + 1), its centre is at i + 0.5 (COLMAP's and nerfstudio's convention)
    taps         x0 = floor(su), x0 + 1, y0 = floor(sv), y0 + 1;  a = su - x0, b = sv - y0
    valid        all four taps inside the source, and the radial map has not folded back: 1 + 3 k1 r2 + 5 k2 r2^2 > 0
                 (d(r radial)/dr; a strong barrel lens otherwise maps far points back into the image);
                 invalid pixels get value 0 and valid 0, valid ones valid 255
    color        (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b per channel
    mask         the same blend of the uint8 levels, then floor(v + 0.5)
    depth        sum w_i d_i / sum w_i over the taps with d_i > 0 (0 = hole), 0 when the weights' sum is 0

FisheyeLensModel / undistort_fisheye_image (gs_undistort_fisheye) are the same resampling for OpenCV's
fisheye lens (k1 .. k4) into the ideal equidistant camera: taps, modes and validity as above, the lens map stated in the class.

These are the host-side statements of what csrc/lens.hip computes in float32, for tests, and the loaders' own undistorter on a
machine without a GPU (data.py).  dtype=np.float32 evaluates the kernel's own arithmetic, operation for operation, as
filter3d.filter_scales(dtype=) does.  The principal point is kept, not recentred: the camera renders it (camera.py)."""
from __future__ import annotations

import numpy as np

MODES = {"color": 0, "mask": 1, "depth": 2}
U32 = 2.0 ** -24                # float32's unit roundoff: the largest relative error of one rounding
COORD_ROUNDINGS = 23            # roundings on the longest path to su / sv (coord_delta)
FOLD_ROUNDINGS = 16             # roundings on the path to the fold-back expression
BLEND_ROUNDINGS = 4             # the blend's own share of remap_bar
DEPTH_ROUNDINGS = 12            # the normalised depth average's


class LensModel:
    """fx, fy, cx, cy in pixels (pixel i covers [i, i + 1)); k1, k2 radial and p1, p2 tangential coefficients in normalised
    coordinates (they do not change when the image is resized)."""

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.p1, self.p2 = (float(v or 0.0) for v in (k1, k2, p1, p2))
        if not (self.fx > 0.0 and self.fy > 0.0):
            raise ValueError("LensModel: focal lengths are > 0")

    @property
    def K(self):
        return self.fx, self.fy, self.cx, self.cy

    @property
    def coefficients(self):
        return self.k1, self.k2, self.p1, self.p2

    @property
    def is_pinhole(self) -> bool:
        return not any(self.coefficients)

    def as_float32(self) -> "LensModel":
        """The lens with every parameter rounded to float32: what the kernel is handed (gs_lens holds floats)."""
        return LensModel(*(float(np.float32(v)) for v in (*self.K, *self.coefficients)))

    def distort(self, x, y, dtype=np.float64):
        """(xd, yd) of normalised coordinates (x, y), in `dtype` and in the kernel's order of operations."""
        T = np.dtype(dtype).type
        x, y = np.asarray(x, dtype), np.asarray(y, dtype)
        k1, k2, p1, p2 = (T(v) for v in self.coefficients)
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        r4 = r2 * r2
        radial = (T(1) + k1 * r2) + k2 * r4
        xd = (x * radial + (T(2) * p1) * xy) + p2 * (r2 + T(2) * xx)
        yd = (y * radial + p1 * (r2 + T(2) * yy)) + (T(2) * p2) * xy
        return xd, yd


FISHEYE_COORD_ROUNDINGS = 38    # FisheyeLensModel: roundings on the longest path to su / sv (coord_delta)
FISHEYE_FOLD_ROUNDINGS = 33     # ... and to the derivative d theta_d / d theta


class FisheyeLensModel:
    """OpenCV's / COLMAP's fisheye lens (OPENCV_FISHEYE; SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE with k3 = k4 = 0; include/gsplat.h
    gs_undistort_fisheye): a ray at angle theta off the axis lands at
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) focal lengths from the principal point.  The
    destination of its resampling is the IDEAL EQUIDISTANT camera (theta_d = theta) that Camera(model="fisheye") renders, not a
    pinhole: a destination pixel's normalised (x, y) is theta (cos phi, sin phi), so the lens is the radial polynomial in
    t2 = x^2 + y^2 = theta^2 and needs no inversion.  Valid: the four taps inside the source, d theta_d / d theta > 0, and theta
    below the first root of that derivative (beyond it the derivative may turn positive again)."""

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.k3, self.k4 = (float(v or 0.0) for v in (k1, k2, k3, k4))
        if not (self.fx > 0.0 and self.fy > 0.0):
            raise ValueError("FisheyeLensModel: focal lengths are > 0")

    @property
    def K(self):
        return self.fx, self.fy, self.cx, self.cy

    @property
    def coefficients(self):
        return self.k1, self.k2, self.k3, self.k4

    @property
    def is_equidistant(self) -> bool:
        return not any(self.coefficients)

    def as_float32(self) -> "FisheyeLensModel":
        return FisheyeLensModel(*(float(np.float32(v)) for v in (*self.K, *self.coefficients)))

    def distort(self, x, y, dtype=np.float64):
        """(xd, yd) = (x, y) theta_d / theta, in `dtype` and in the kernel's order of operations."""
        T = np.dtype(dtype).type
        x, y = np.asarray(x, dtype), np.asarray(y, dtype)
        k1, k2, k3, k4 = (T(v) for v in self.coefficients)
        t2 = x * x + y * y
        radial = (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2 + T(1)
        return x * radial, y * radial

    def first_fold(self, tMax=None) -> float:
        """theta^2 at the first root of D(t) = d theta_d / d theta = 1 + 3 k1 t + 5 k2 t^2 + 7 k3 t^3 + 9 k4 t^4, inf without one.
        tMax=None: over all t > 0, the smallest positive real root numpy.roots finds.  tMax given (the largest t of a destination
        image, dst_t_max): csrc/lens.hip's own search, step for step in float64 -- [0, tMax] in 4096 steps for the first sign
        change, then 100 bisections -- which is what the resampling uses on both sides, so that host and kernel cut at the same
        limit.  The scan steps over a root D only touches and over a pair of roots closer than a step; `D > 0` still decides
        every pixel there, on both sides alike."""
        if tMax is not None:
            k1, k2, k3, k4 = self.coefficients
            D = lambda t: (((9.0 * k4 * t + 7.0 * k3) * t + 5.0 * k2) * t + 3.0 * k1) * t + 1.0      # noqa: E731
            lo = 0.0
            for step in range(1, 4097):
                hi = tMax * step / 4096
                if not D(hi) > 0.0:
                    a, b = lo, hi
                    for _ in range(100):
                        m = 0.5 * (a + b)
                        if D(m) > 0.0:
                            a = m
                        else:
                            b = m
                    return b
                lo = hi
            return float("inf")
        c = [9.0 * self.k4, 7.0 * self.k3, 5.0 * self.k2, 3.0 * self.k1, 1.0]
        while len(c) > 1 and c[0] == 0.0:
            c = c[1:]
        if len(c) == 1:
            return float("inf")
        roots = np.roots(c)
        real = roots[np.abs(roots.imag) <= 1e-12 * np.maximum(1.0, np.abs(roots.real))].real
        real = real[real > 0.0]
        return float(real.min()) if real.size else float("inf")

    def fold(self, x, y, dtype=np.float64, tMax=None):
        """The derivative d theta_d / d theta at (x, y), negated in magnitude beyond the first fold (first_fold(tMax)): valid iff > 0."""
        T = np.dtype(dtype).type
        x, y = np.asarray(x, dtype), np.asarray(y, dtype)
        k1, k2, k3, k4 = (T(v) for v in self.coefficients)
        t2 = x * x + y * y
        d = ((((T(9) * k4) * t2 + T(7) * k3) * t2 + T(5) * k2) * t2 + T(3) * k1) * t2 + T(1)
        lim = self.first_fold(tMax)
        limit = T(min(lim, float(np.finfo(np.float32).max))) if T is np.float32 else T(lim)
        return np.where(t2 < limit, d, -np.abs(d)).astype(dtype)


def dst_t_max(dstK, dstW, dstH) -> float:
    """The largest t = x^2 + y^2 over the destination image's corners (pixel edges 0 .. W, 0 .. H), as csrc/lens.hip forms it
    from the float32 destination intrinsics."""
    nfx, nfy, ncx, ncy = (float(np.float32(v)) for v in dstK)
    return max(((cx - ncx) / nfx) ** 2 + ((cy - ncy) / nfy) ** 2 for cx in (0.0, float(dstW)) for cy in (0.0, float(dstH)))


def undistort_fisheye_image(img, lens: FisheyeLensModel, dstK=None, dstSize=None, mode: str = "color", dtype=np.float64):
    """undistort_image for a FisheyeLensModel: (out, valid uint8 [H, W]), the view resampled into the ideal equidistant camera
    dstK = (fx, fy, cx, cy) of size dstSize (None: the lens's own intrinsics and the source's size).  float64 states it, float32
    evaluates csrc/lens.hip's arithmetic operation for operation."""
    if not isinstance(lens, FisheyeLensModel):
        raise ValueError("undistort_fisheye_image takes a FisheyeLensModel")
    return undistort_image(img, lens, dstK, dstSize, mode, dtype)


def _dst(lens, dstK, dstSize, srcShape):
    nfx, nfy, ncx, ncy = (float(v) for v in (lens.K if dstK is None else dstK))
    if not (nfx > 0.0 and nfy > 0.0):
        raise ValueError("dstK = (fx, fy, cx, cy) with focal lengths > 0")
    W, H = (int(srcShape[1]), int(srcShape[0])) if dstSize is None else (int(dstSize[0]), int(dstSize[1]))
    if W < 1 or H < 1:
        raise ValueError("dstSize = (width, height), both positive")
    return (nfx, nfy, ncx, ncy), W, H


def _normalised(dstK, dstW, dstH, dtype):
    T = np.dtype(dtype).type
    nfx, nfy, ncx, ncy = (T(v) for v in dstK)
    i = np.arange(dstW, dtype=dtype)[None, :]
    j = np.arange(dstH, dtype=dtype)[:, None]
    x = np.broadcast_to(((i + T(0.5)) - ncx) / nfx, (dstH, dstW))
    y = np.broadcast_to(((j + T(0.5)) - ncy) / nfy, (dstH, dstW))
    return x, y


def source_coords(lens, dstK, dstW, dstH, dtype=np.float64):
    """(su, sv, fold) [dstH, dstW] in `dtype`: the sample position in the source of every destination pixel of the pinhole
    dstK = (nfx, nfy, ncx, ncy), and the fold-back expression 1 + 3 k1 r2 + 5 k2 r2^2."""
    T = np.dtype(dtype).type
    x, y = _normalised(dstK, dstW, dstH, dtype)
    xd, yd = lens.distort(x, y, dtype)
    fx, fy, cx, cy = (T(v) for v in lens.K)
    su = (fx * xd + cx) - T(0.5)
    sv = (fy * yd + cy) - T(0.5)
    if isinstance(lens, FisheyeLensModel):
        return su, sv, lens.fold(x, y, dtype, dst_t_max(dstK, dstW, dstH))
    r2 = x * x + y * y
    fold = (T(1) + (T(3) * T(lens.k1)) * r2) + (T(5) * T(lens.k2)) * (r2 * r2)
    return su, sv, fold


def _taps(su, sv, fold, srcW, srcH):
    """(valid [H, W] bool, x0, y0 int64 (0 where invalid), a, b) of sample positions: NaN or out-of-range positions are invalid."""
    with np.errstate(invalid="ignore"):
        fx0, fy0 = np.floor(su), np.floor(sv)
        valid = (fold > 0) & (fx0 >= 0) & (fx0 <= srcW - 2) & (fy0 >= 0) & (fy0 <= srcH - 2)
    x0 = np.where(valid, fx0, 0).astype(np.int64)
    y0 = np.where(valid, fy0, 0).astype(np.int64)
    a = np.where(valid, su - fx0, 0).astype(su.dtype)
    b = np.where(valid, sv - fy0, 0).astype(su.dtype)
    return valid, x0, y0, a, b


def remap_values(img, lens, dstK=None, dstSize=None, mode: str = "color", dtype=np.float64):
    """(value, valid bool [H, W]) in `dtype`, before the result's own cast: the blend per channel ([H, W, C] for a colour image
    given as [H, W, C], else [H, W]); for a mask the value BEFORE floor(v + 0.5); for a depth the normalised average."""
    if mode not in MODES:
        raise ValueError(f"mode is one of {sorted(MODES)}")
    img = np.asarray(img)
    if mode == "color":
        if img.ndim not in (2, 3) or (img.ndim == 3 and not 1 <= img.shape[2] <= 4):
            raise ValueError("a colour image is float32 [H, W, C] with C in 1 .. 4")
    elif img.ndim != 2 or (mode == "mask" and img.dtype != np.uint8):
        raise ValueError("a mask is uint8 [H, W], a depth float32 [H, W]")
    T = np.dtype(dtype).type
    dstK, W, H = _dst(lens, dstK, dstSize, img.shape)
    srcH, srcW = img.shape[:2]
    su, sv, fold = source_coords(lens, dstK, W, H, dtype)
    valid, x0, y0, a, b = _taps(su, sv, fold, srcW, srcH)
    x1, y1 = np.where(valid, x0 + 1, 0), np.where(valid, y0 + 1, 0)
    S = img.astype(dtype)
    t00, t10, t01, t11 = S[y0, x0], S[y0, x1], S[y1, x0], S[y1, x1]
    a1, b1 = T(1) - a, T(1) - b
    if mode == "depth":
        num, den = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
        for w, d in ((a1 * b1, t00), (a * b1, t10), (a1 * b, t01), (a * b, t11)):
            live = d > 0
            num = np.where(live, num + w * d, num)
            den = np.where(live, den + w, den)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(den > 0, num / den, T(0))
    else:
        if S.ndim == 3:
            a, b, a1, b1 = (v[..., None] for v in (a, b, a1, b1))
        out = (t00 * a1 + t10 * a) * b1 + (t01 * a1 + t11 * a) * b
    out = np.where(valid if out.ndim == 2 else valid[..., None], out, T(0)).astype(dtype)
    return out, valid


def undistort_image(img, lens, dstK=None, dstSize=None, mode: str = "color", dtype=np.float64):
    """(out, valid uint8 [H, W]): the image seen through `lens` resampled into the pinhole dstK = (fx, fy, cx, cy) of size
    dstSize = (W, H); None: the lens's own fx, fy, cx, cy and the source's size.  out is float32 for "color" and "depth", uint8
    for "mask".  Evaluated in `dtype` (float64: the statement; float32: the kernel's own arithmetic)."""
    value, valid = remap_values(img, lens, dstK, dstSize, mode, dtype)
    if mode == "mask":
        out = np.minimum(np.floor(value + np.dtype(dtype).type(0.5)), 255).astype(np.uint8)
    else:
        out = value.astype(np.float32)
    return out, np.where(valid, 255, 0).astype(np.uint8)


def coord_delta(lens, dstK, dstW, dstH):
    """(delta [H, W], fold_delta [H, W]): float32 error bounds of the kernel's sample position, in source pixels, and of its
    fold-back expression, for float32 lens parameters (LensModel.as_float32).  Counting roundings along the longest path
    (each rounding at most 2^-24 relative, relative errors add through products and, over magnitudes, through sums):
    x: 2 (i + 0.5 is exact; a subtraction of exact operands, a division); x x: 5; r2: 6; r4: 13; k2 r4: 14; k1 r2: 7;
    radial: 15; x radial: 18; (2 p1)(x y): 6; their sum: 19; p2 (r2 + 2 x x): 8; xd: 20; fx xd: 21; + cx: 22; - 0.5: 23
    roundings of a quantity bounded by the sum of the terms' magnitudes,
        M_u = fx (|x| (1 + |k1| r2 + |k2| r4) + 2 |p1| |x y| + |p2| (r2 + 2 x^2)) + |cx| + 0.5,
    and the same for v; delta is the larger of the two.  The fold-back expression: r2 6, r4 13, its products and two sums
    16 roundings of 1 + 3 |k1| r2 + 5 |k2| r4."""
    x, y = _normalised(dstK, dstW, dstH, np.float64)
    ax, ay = np.abs(x), np.abs(y)
    r2 = x * x + y * y
    if isinstance(lens, FisheyeLensModel):
        # x: 2; x x: 5; t2: 6; k4 t2: 7; + k3: 8; t2: 15; + k2: 16; t2: 23; + k1: 24; t2: 31; + 1: 32; x radial: 35; fx: 36;
        # + cx: 37; - 0.5: 38 roundings of M = f |x| (1 + |k1| t2 + .. + |k4| t2^4) + |c| + 0.5.  The derivative: 9 k4: 1; t2: 8;
        # + 7 k3: 9 (its own product inside); t2: 16; 17; 24; 25; 32; + 1: 33 roundings of 1 + 3 |k1| t2 + .. + 9 |k4| t2^4
        k1, k2, k3, k4 = (abs(v) for v in lens.coefficients)
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        Mu, Mv = lens.fx * ax * rad + abs(lens.cx) + 0.5, lens.fy * ay * rad + abs(lens.cy) + 0.5
        der = 1.0 + r2 * (3.0 * k1 + r2 * (5.0 * k2 + r2 * (7.0 * k3 + r2 * 9.0 * k4)))
        return FISHEYE_COORD_ROUNDINGS * U32 * np.maximum(Mu, Mv), FISHEYE_FOLD_ROUNDINGS * U32 * der
    r4 = r2 * r2
    k1, k2, p1, p2 = (abs(v) for v in lens.coefficients)
    rad = 1.0 + k1 * r2 + k2 * r4
    Mu = lens.fx * (ax * rad + 2.0 * p1 * ax * ay + p2 * (r2 + 2.0 * x * x)) + abs(lens.cx) + 0.5
    Mv = lens.fy * (ay * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * ax * ay) + abs(lens.cy) + 0.5
    return COORD_ROUNDINGS * U32 * np.maximum(Mu, Mv), FOLD_ROUNDINGS * U32 * (1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r4)


def remap_bar(img, lens, dstK=None, dstSize=None, mode: str = "color"):
    """Per output element, the float32 error bound of the kernel against remap_values(dtype=float64), 0 where the float64
    statement is invalid.  With delta = coord_delta (the sample position's error in pixels):

        color, mask   bar = delta (max |tap differences| along x + along y) + 4 2^-24 max |tap|
                      Bilinear interpolation is continuous across cell borders, so a floor that flips costs no more than delta
                      times the slope of the cell it lands in: where a position is within delta of a border, the slopes and the
                      maximum are taken over the cells on both sides.  4 roundings: a tap's path through the blend.
        depth         v = N / D over the live taps, D their weights' sum: |dv/da| = |sum_i dw_i/da (d_i - v)| / D <= 2 range / D
                      (sum_i |dw_i/da| = 2, |d_i - v| <= range = max - min of the live taps), the same along b, so
                      bar = delta 4 range / D + 12 2^-24 max |tap| (weights 2 roundings, products 1, sums 3, for N and for D,
                      the division 1).  The average is NOT continuous across a border whose shared taps are all holes, so
                      within delta of a border the bar is the largest tap of the cells on both sides (a result lies between 0
                      and its taps' maximum).

    For a mask the bar is on the value before rounding, in levels.  No constant here is fitted to the kernel's output."""
    img = np.asarray(img)
    dstK, W, H = _dst(lens, dstK, dstSize, img.shape)
    srcH, srcW = img.shape[:2]
    su, sv, fold = source_coords(lens, dstK, W, H)
    valid, x0, y0, a, b = _taps(su, sv, fold, srcW, srcH)
    delta, _ = coord_delta(lens, dstK, W, H)
    S = img.astype(np.float64).reshape(srcH, srcW, -1)
    C = S.shape[2]
    bar = np.zeros((H, W, C))
    if srcW < 2 or srcH < 2 or not valid.any():
        return bar.reshape((H, W) + img.shape[2:])
    A = np.abs(S)
    cellMax = np.maximum(np.maximum(A[:-1, :-1], A[:-1, 1:]), np.maximum(A[1:, :-1], A[1:, 1:]))
    if mode == "depth":
        t = [S[y0, x0, 0], S[y0, x0 + valid, 0], S[y0 + valid, x0, 0], S[y0 + valid, x0 + valid, 0]]
        w = [(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b]
        live = [d > 0 for d in t]
        D = sum(np.where(l, wi, 0.0) for l, wi in zip(live, w))
        hi = np.max([np.where(l, d, -np.inf) for l, d in zip(live, t)], axis=0)
        lo = np.min([np.where(l, d, np.inf) for l, d in zip(live, t)], axis=0)
        rng = np.where(np.isfinite(hi), hi - lo, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            slope = np.where(D > 0, 4.0 * rng / D, 0.0)
        bar[..., 0] = delta * slope + DEPTH_ROUNDINGS * U32 * cellMax[y0, x0, 0]
    else:
        cellDx = np.maximum(np.abs(S[:-1, 1:] - S[:-1, :-1]), np.abs(S[1:, 1:] - S[1:, :-1]))
        cellDy = np.maximum(np.abs(S[1:, :-1] - S[:-1, :-1]), np.abs(S[1:, 1:] - S[:-1, 1:]))
    slopeSum, tapMax = np.zeros((H, W, C)), np.zeros((H, W, C))
    near = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = valid.copy()
            if dx:
                m &= (a < delta) if dx < 0 else (1.0 - a < delta)
            if dy:
                m &= (b < delta) if dy < 0 else (1.0 - b < delta)
            cx_, cy_ = x0 + dx, y0 + dy
            m &= (cx_ >= 0) & (cx_ <= srcW - 2) & (cy_ >= 0) & (cy_ <= srcH - 2)
            if not m.any():
                continue
            if dx or dy:
                near |= m
            yy, xx = cy_[m], cx_[m]
            tapMax[m] = np.maximum(tapMax[m], cellMax[yy, xx])
            if mode != "depth":
                slopeSum[m] = np.maximum(slopeSum[m], cellDx[yy, xx] + cellDy[yy, xx])
    if mode == "depth":
        bar[near] = np.maximum(bar[near], tapMax[near])
    else:
        bar = delta[..., None] * slopeSum + BLEND_ROUNDINGS * U32 * tapMax
    bar[~valid] = 0.0
    return bar.reshape((H, W) + img.shape[2:])
