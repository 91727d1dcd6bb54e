// gs_expo.h -- the affine colour transform M = [A | b] shared by exposure compensation (exposure.hip) and the bilateral
// grid (bilateral_grid.hip), whose sliced coefficients are such an M per pixel.  Both files are compiled with
// -ffp-contract=off, so the nesting below is the one executed: with A = I, b = 0 every fmaf adds exact zeros.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

// M row-major 3 x 4: m[4c + j] = A[c][j] (j < 3), m[4c + 3] = b[c]
__device__ __forceinline__ void expo_apply(const float* m, float r0, float r1, float r2, float o[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++)
        o[c] = fmaf(m[4 * c], r0, fmaf(m[4 * c + 1], r1, fmaf(m[4 * c + 2], r2, m[4 * c + 3])));
}

// A^T g: dL/dr[j] = A[0][j] g0 + A[1][j] g1 + A[2][j] g2, in that nesting
__device__ __forceinline__ void expo_vjp(const float* m, float g0, float g1, float g2, float o[3])
{
#pragma unroll
    for (int j = 0; j < 3; j++) o[j] = fmaf(m[j], g0, fmaf(m[4 + j], g1, m[8 + j] * g2));
}

}  // namespace gs
