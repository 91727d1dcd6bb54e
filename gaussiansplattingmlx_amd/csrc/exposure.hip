// exposure.hip -- per-view exposure compensation (include/gsplat.h gs_set_exposure): an affine colour
// transform c = A r + b of the render, applied before the loss and trained with it.  Compiled with -ffp-contract=off: every
// product and sum below is written out (fmaf where the specification has one), so the identity exposure gives back the
// render and the loss's cotangent exactly, and the gradient's sums round the same way on every build.
//
// Three passes, one launch each, around the unchanged loss kernel:
//   exposure_apply_kernel  c = A r + b into the ctx's scratch image (never in place: the fused blend backward reads the
//                          forward's own colour image);
//   exposure_bwd_kernel    cot <- A^T g in place, and per workgroup the 12 sums g[c] r[j], g[c] in float64 (fixed grid,
//                          fixed order, no atomics);
//   exposure_final_kernel  one workgroup: the workgroups' partials in float64, in block order -> grad[12] as float32.
#include "gs_ctx.h"
#include "gs_expo.h"

namespace gs {

constexpr int EXPO_THREADS = 256;
constexpr int EXPO_BWD_BLOCKS = 512;            // the backward's grid: a constant, so the gradient's summation order is one
constexpr int EXPO_SEGS = 16;                    // the final kernel: block segments summed side by side, then in order
static_assert(EXPO_BWD_BLOCKS % EXPO_SEGS == 0, "segments cover the blocks");
static_assert(12 * EXPO_SEGS <= EXPO_THREADS, "one thread per component and segment");

// Four pixels (12 floats) per thread: three float4 where the buffers are 16-byte aligned, twelve floats otherwise
template <bool VEC>
__device__ __forceinline__ void expo_load(const float* p, long long q, float v[12])
{
    if (VEC) {
        const float4* p4 = reinterpret_cast<const float4*>(p) + 3 * q;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float4 t = p4[k];
            v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = p[12 * q + k];
    }
}

template <bool VEC>
__device__ __forceinline__ void expo_store(float* p, long long q, const float v[12])
{
    if (VEC) {
        float4* p4 = reinterpret_cast<float4*>(p) + 3 * q;
#pragma unroll
        for (int k = 0; k < 3; k++) p4[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) p[12 * q + k] = v[k];
    }
}

// in and out may be the same buffer (each thread reads its pixels before it writes them)
template <bool VEC>
__global__ __launch_bounds__(EXPO_THREADS) void exposure_apply_kernel(long long n, const float* __restrict__ M, const float* in,
                                                                      float* out)
{
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = M[k];
    const long long nq = n >> 2, stride = (long long)gridDim.x * EXPO_THREADS;
    const long long t = (long long)blockIdx.x * EXPO_THREADS + threadIdx.x;
    for (long long q = t; q < nq; q += stride) {
        float v[12];
        expo_load<VEC>(in, q, v);
#pragma unroll
        for (int p = 0; p < 4; p++) expo_apply(m, v[3 * p], v[3 * p + 1], v[3 * p + 2], &v[3 * p]);
        expo_store<VEC>(out, q, v);
    }
    const long long tail = nq * 4 + t;          // the last n % 4 pixels, one per thread
    if (tail < n) {
        float o[3];
        expo_apply(m, in[3 * tail], in[3 * tail + 1], in[3 * tail + 2], o);
        out[3 * tail] = o[0]; out[3 * tail + 1] = o[1]; out[3 * tail + 2] = o[2];
    }
}

__device__ __forceinline__ void expo_accum(double acc[12], float g0, float g1, float g2, float r0, float r1, float r2)
{
    const float g[3] = {g0, g1, g2};
    const double r[3] = {(double)r0, (double)r1, (double)r2};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double gc = (double)g[c];
#pragma unroll
        for (int j = 0; j < 3; j++) acc[4 * c + j] = fma(gc, r[j], acc[4 * c + j]);      // (float products are exact in float64)
        acc[4 * c + 3] += gc;
    }
}

// cot holds g = dL/dc (the loss kernel's output); render is the caller's uncorrected image.  Rewrites cot with A^T g and
// writes this workgroup's 12 sums to partials[blockIdx.x * 12 ..].  Pixel order within a thread, then a fixed butterfly over
// the wave, then the four waves in order: the same bits on every run.
template <bool VEC>
__global__ __launch_bounds__(EXPO_THREADS) void exposure_bwd_kernel(long long n, const float* __restrict__ M,
                                                                    const float* __restrict__ render, float* __restrict__ cot,
                                                                    double* __restrict__ partials)
{
    __shared__ double waveSums[EXPO_THREADS / 64][12];
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = M[k];
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    const long long nq = n >> 2, stride = (long long)EXPO_BWD_BLOCKS * EXPO_THREADS;
    const long long t = (long long)blockIdx.x * EXPO_THREADS + threadIdx.x;
    for (long long q = t; q < nq; q += stride) {
        float g[12], r[12];
        expo_load<VEC>(cot, q, g);
        expo_load<VEC>(render, q, r);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            expo_accum(acc, g[3 * p], g[3 * p + 1], g[3 * p + 2], r[3 * p], r[3 * p + 1], r[3 * p + 2]);
            float o[3];
            expo_vjp(m, g[3 * p], g[3 * p + 1], g[3 * p + 2], o);
            g[3 * p] = o[0]; g[3 * p + 1] = o[1]; g[3 * p + 2] = o[2];
        }
        expo_store<VEC>(cot, q, g);
    }
    for (long long p = nq * 4 + t; p < n; p += stride) {        // the last n % 4 pixels
        const float g0 = cot[3 * p], g1 = cot[3 * p + 1], g2 = cot[3 * p + 2];
        expo_accum(acc, g0, g1, g2, render[3 * p], render[3 * p + 1], render[3 * p + 2]);
        float o[3];
        expo_vjp(m, g0, g1, g2, o);
        cot[3 * p] = o[0]; cot[3 * p + 1] = o[1]; cot[3 * p + 2] = o[2];
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        double s = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        acc[k] = s;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) waveSums[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double s = waveSums[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EXPO_THREADS / 64; w++) s += waveSums[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 12 + threadIdx.x] = s;
    }
}

// One workgroup: thread (k, s) sums component k over blocks [s B, (s + 1) B) in block order, B = EXPO_BWD_BLOCKS / EXPO_SEGS;
// thread k then sums its EXPO_SEGS segment sums in order and overwrites grad[k].
__global__ __launch_bounds__(EXPO_THREADS) void exposure_final_kernel(const double* __restrict__ partials, float* __restrict__ grad)
{
    __shared__ double segSums[12][EXPO_SEGS];
    constexpr int B = EXPO_BWD_BLOCKS / EXPO_SEGS;
    const int k = threadIdx.x / EXPO_SEGS, s = threadIdx.x % EXPO_SEGS;
    if (k < 12) {
        double v[B];
#pragma unroll
        for (int b = 0; b < B; b++) v[b] = partials[(size_t)(s * B + b) * 12 + k];
        double sum = v[0];
#pragma unroll
        for (int b = 1; b < B; b++) sum += v[b];
        segSums[k][s] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double sum = segSums[threadIdx.x][0];
        for (int q = 1; q < EXPO_SEGS; q++) sum += segSums[threadIdx.x][q];
        grad[threadIdx.x] = (float)sum;
    }
}

static bool expo_aligned(const void* a, const void* b)
{
    return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

int launch_exposure_apply(gs_ctx* c, long long n, const float* M, const float* in, float* out)
{
    if (n <= 0) return GS_OK;
    const long long nq = n >> 2;
    long long nb = (nq + EXPO_THREADS - 1) / EXPO_THREADS;
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    if (expo_aligned(in, out))
        hipLaunchKernelGGL(exposure_apply_kernel<true>, dim3((unsigned)nb), dim3(EXPO_THREADS), 0, c->stream, n, M, in, out);
    else
        hipLaunchKernelGGL(exposure_apply_kernel<false>, dim3((unsigned)nb), dim3(EXPO_THREADS), 0, c->stream, n, M, in, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

long long exposure_partials_doubles() { return 12LL * EXPO_BWD_BLOCKS; }

int launch_exposure_backward(gs_ctx* c, long long n, const float* M, const float* render, float* cot, double* partials,
                             float* grad)
{
    if (expo_aligned(render, cot))
        hipLaunchKernelGGL(exposure_bwd_kernel<true>, dim3(EXPO_BWD_BLOCKS), dim3(EXPO_THREADS), 0, c->stream, n, M, render,
                           cot, partials);
    else
        hipLaunchKernelGGL(exposure_bwd_kernel<false>, dim3(EXPO_BWD_BLOCKS), dim3(EXPO_THREADS), 0, c->stream, n, M, render,
                           cot, partials);
    hipLaunchKernelGGL(exposure_final_kernel, dim3(1), dim3(EXPO_THREADS), 0, c->stream, partials, grad);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
