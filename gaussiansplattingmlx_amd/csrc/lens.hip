// lens.hip -- lens undistortion (include/gsplat.h gs_undistort): resamples a view taken through OpenCV's
// radial-tangential lens into a pinhole camera, once per view at load time.  Compiled with -ffp-contract=off: every product
// and sum below rounds where it is written, the order lens.py's float32 evaluation restates, so a sample position does not
// depend on the build.
//
//   undistort_kernel<MODE, T>   one lane per destination pixel, 256-thread blocks laid out 64 x 4 over the image: a wave is a
//                               64-pixel row segment, so its stores coalesce and its four-tap gathers stay in neighbouring cache
//                               lines (the map is smooth).  The channel loop is inside the lane.  No LDS, no atomics.
//   LENS = gs_lens              the radial-tangential lens into a pinhole (gs_undistort);
//   LENS = FisheyeLensArgs      OpenCV's fisheye lens into the ideal equidistant camera of the destination intrinsics
//                               (gs_undistort_fisheye): a destination pixel's normalised (x, y) is theta (cos phi, sin phi), and
//                               theta_d / theta is a polynomial in t2 = theta^2 -- no square root, no inversion.
#include <type_traits>

#include "gs_ctx.h"

namespace gs {

constexpr int LENS_BX = 64, LENS_BY = 4;
constexpr int LENS_COLOR = 0, LENS_MASK = 1, LENS_DEPTH = 2;

struct FisheyeLensArgs {
    gs_fisheye_lens L;
    float t2Limit;      // theta^2 at the first root of d theta_d / d theta (the largest float without one), found on the host
};

template <int MODE, typename T, typename LENS>
__global__ __launch_bounds__(LENS_BX * LENS_BY) void undistort_kernel(LENS lens, int srcW, int srcH, int dstW, int dstH, int C,
                                                                      const T* __restrict__ src, T* __restrict__ dst,
                                                                      unsigned char* __restrict__ valid)
{
    const int i = blockIdx.x * LENS_BX + threadIdx.x, j = blockIdx.y * LENS_BY + threadIdx.y;
    if (i >= dstW || j >= dstH) return;
    float su, sv, fold;
    if constexpr (std::is_same<LENS, FisheyeLensArgs>::value) {
        const gs_fisheye_lens& L = lens.L;
        const float x = (((float)i + 0.5f) - L.dst_cx) / L.dst_fx;
        const float y = (((float)j + 0.5f) - L.dst_cy) / L.dst_fy;
        const float t2 = x * x + y * y;
        const float radial = (((L.k4 * t2 + L.k3) * t2 + L.k2) * t2 + L.k1) * t2 + 1.0f;
        const float xd = x * radial, yd = y * radial;
        su = (L.fx * xd + L.cx) - 0.5f; sv = (L.fy * yd + L.cy) - 0.5f;
        fold = ((((9.0f * L.k4) * t2 + 7.0f * L.k3) * t2 + 5.0f * L.k2) * t2 + 3.0f * L.k1) * t2 + 1.0f;
        if (!(t2 < lens.t2Limit)) fold = -fabsf(fold);      // (beyond the first fold the derivative may turn positive again)
    } else {
    const gs_lens& L = lens;
    const float x = (((float)i + 0.5f) - L.dst_cx) / L.dst_fx;
    const float y = (((float)j + 0.5f) - L.dst_cy) / L.dst_fy;
    const float xx = x * x, yy = y * y, xy = x * y;
    const float r2 = xx + yy, r4 = r2 * r2;
    const float radial = (1.0f + L.k1 * r2) + L.k2 * r4;
    const float xd = (x * radial + (2.0f * L.p1) * xy) + L.p2 * (r2 + 2.0f * xx);
    const float yd = (y * radial + L.p1 * (r2 + 2.0f * yy)) + (2.0f * L.p2) * xy;
    su = (L.fx * xd + L.cx) - 0.5f; sv = (L.fy * yd + L.cy) - 0.5f;
    fold = (1.0f + (3.0f * L.k1) * r2) + (5.0f * L.k2) * r4;
    }
    const float fx0 = floorf(su), fy0 = floorf(sv);
    // (compared as floats, before any conversion: a NaN or an out-of-range position fails every test and reads nothing)
    const bool ok = fold > 0.0f && fx0 >= 0.0f && fx0 <= (float)(srcW - 2) && fy0 >= 0.0f && fy0 <= (float)(srcH - 2);
    const size_t o = (size_t)j * dstW + i;
    if (valid) valid[o] = ok ? 255 : 0;
    if (!ok) {
        for (int c = 0; c < C; c++) dst[o * C + c] = (T)0;
        return;
    }
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float a = su - fx0, b = sv - fy0;
    const float a1 = 1.0f - a, b1 = 1.0f - b;
    const T* p00 = src + ((size_t)y0 * srcW + x0) * C;
    const T* p01 = p00 + (size_t)srcW * C;
    if (MODE == LENS_DEPTH) {
        const float d[4] = {(float)p00[0], (float)p00[1], (float)p01[0], (float)p01[1]};
        const float w[4] = {a1 * b1, a * b1, a1 * b, a * b};
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (d[k] > 0.0f) { num = num + w[k] * d[k]; den = den + w[k]; }
        dst[o] = (T)(den > 0.0f ? num / den : 0.0f);
        return;
    }
    for (int c = 0; c < C; c++) {
        const float t00 = (float)p00[c], t10 = (float)p00[C + c], t01 = (float)p01[c], t11 = (float)p01[C + c];
        const float v = (t00 * a1 + t10 * a) * b1 + (t01 * a1 + t11 * a) * b;
        dst[o * C + c] = MODE == LENS_MASK ? (T)fminf(floorf(v + 0.5f), 255.0f) : (T)v;
    }
}

template <typename LENS>
static int launch_undistort_as(gs_ctx* c, const LENS& lens, int srcW, int srcH, int dstW, int dstH, int channels, int mode,
                               const void* src, void* dst, unsigned char* valid)
{
    const dim3 grid(gs_div_up(dstW, LENS_BX), gs_div_up(dstH, LENS_BY)), block(LENS_BX, LENS_BY);
    if (mode == LENS_COLOR)
        hipLaunchKernelGGL((undistort_kernel<LENS_COLOR, float, LENS>), grid, block, 0, c->stream, lens, srcW, srcH, dstW, dstH,
                           channels, (const float*)src, (float*)dst, valid);
    else if (mode == LENS_MASK)
        hipLaunchKernelGGL((undistort_kernel<LENS_MASK, unsigned char, LENS>), grid, block, 0, c->stream, lens, srcW, srcH, dstW, dstH,
                           channels, (const unsigned char*)src, (unsigned char*)dst, valid);
    else
        hipLaunchKernelGGL((undistort_kernel<LENS_DEPTH, float, LENS>), grid, block, 0, c->stream, lens, srcW, srcH, dstW, dstH,
                           channels, (const float*)src, (float*)dst, valid);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_undistort(gs_ctx* c, const gs_lens& lens, int srcW, int srcH, int dstW, int dstH, int channels, int mode, const void* src,
                     void* dst, unsigned char* valid)
{
    return launch_undistort_as(c, lens, srcW, srcH, dstW, dstH, channels, mode, src, dst, valid);
}

// theta^2 at the first root of d theta_d / d theta = 1 + 3 k1 t + 5 k2 t^2 + 7 k3 t^3 + 9 k4 t^4 (t = theta^2) inside the
// destination image, in float64: a scan of [0, tMax] in 4096 steps for the first sign change, then bisection.  No root there: the
// largest float.  (A pixel at the root itself fails the derivative test whichever side of this limit rounding puts it.)
static float fisheye_first_fold(const gs_fisheye_lens& L, int dstW, int dstH)
{
    auto D = [&](double t) { return (((9.0 * L.k4 * t + 7.0 * L.k3) * t + 5.0 * L.k2) * t + 3.0 * L.k1) * t + 1.0; };
    double tMax = 0.0;
    for (int cy = 0; cy < 2; cy++)
        for (int cx = 0; cx < 2; cx++) {
            const double x = ((cx ? dstW : 0) - (double)L.dst_cx) / L.dst_fx, y = ((cy ? dstH : 0) - (double)L.dst_cy) / L.dst_fy;
            tMax = fmax(tMax, x * x + y * y);
        }
    constexpr int STEPS = 4096;
    double lo = 0.0;
    for (int s = 1; s <= STEPS; s++) {
        const double hi = tMax * s / STEPS;
        if (!(D(hi) > 0.0)) {
            double a = lo, b = hi;
            for (int it = 0; it < 100; it++) {
                const double m = 0.5 * (a + b);
                if (D(m) > 0.0) a = m; else b = m;
            }
            return (float)b;
        }
        lo = hi;
    }
    return 3.402823466e38f;
}

int launch_undistort_fisheye(gs_ctx* c, const gs_fisheye_lens& lens, int srcW, int srcH, int dstW, int dstH, int channels, int mode,
                             const void* src, void* dst, unsigned char* valid)
{
    FisheyeLensArgs a;
    a.L = lens;
    a.t2Limit = fisheye_first_fold(lens, dstW, dstH);
    return launch_undistort_as(c, a, srcW, srcH, dstW, dstH, channels, mode, src, dst, valid);
}

}  // namespace gs
