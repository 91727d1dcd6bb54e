// background.hip -- the training target of an RGBA view over a background colour (include/gsplat.h gs_composite_target;
// DESIGN.md section 18).
//
//   out_c = fma(a, rgb_c, (1 - a) b_c)      rgb straight (un-premultiplied), b by value
//
// Three roundings per value (1 - a, its product with b_c, the fma); the file is built with -ffp-contract=off, so the
// expression is the one written here on every compiler.  One pixel per thread over a grid-stride loop: 28 B of traffic per
// pixel (16 read, 12 written), memory-bound.  out may be rgb itself: a thread reads its pixel's three values before it writes
// them and no thread touches another's pixel.
#include "gs_ctx.h"

namespace gs {

constexpr int COMPOSITE_THREADS = 256;

__global__ __launch_bounds__(COMPOSITE_THREADS) void composite_target_kernel(long long n, const float* rgb,
                                                                             const float* __restrict__ alpha, float b0, float b1,
                                                                             float b2, float* out)
{
    const long long stride = (long long)gridDim.x * COMPOSITE_THREADS;
    for (long long p = (long long)blockIdx.x * COMPOSITE_THREADS + threadIdx.x; p < n; p += stride) {
        const float a = alpha[p];
        const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
        const float t = 1.0f - a;
        out[3 * p] = fmaf(a, r, t * b0);
        out[3 * p + 1] = fmaf(a, g, t * b1);
        out[3 * p + 2] = fmaf(a, b, t * b2);
    }
}

int launch_composite_target(gs_ctx* c, long long n, const float* rgb, const float* alpha, const float bg[3], float* out)
{
    if (n <= 0) return GS_OK;
    long long nb = (n + COMPOSITE_THREADS - 1) / COMPOSITE_THREADS;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(composite_target_kernel, dim3((unsigned)nb), dim3(COMPOSITE_THREADS), 0, c->stream, n, rgb, alpha, bg[0],
                       bg[1], bg[2], out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
