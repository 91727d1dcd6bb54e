// depth_loss.hip -- depth supervision on the render's depth and alpha images (include/gsplat.h gs_depth_loss /
// gs_depth_normalize; tests/depth_loss_numpy.py restates it in numpy).
//
//   D = render depth (sum T alpha z), a = render alpha, t = scale * target + offset (two roundings: the file is built with
//   -ffp-contract=off, so a target transformed beforehand with the same two float32 operations gives the same bits)
//
//   mode                 x        valid iff mask and                cot_depth       cot_alpha
//   GS_DEPTH_ACCUMULATED D        --                                g               0
//   GS_DEPTH_EXPECTED    D / a    a >= alpha_min, a > 0             g / a           -g D / a^2
//   GS_DEPTH_DISPARITY   a / D    a >= alpha_min, a > 0, D > 0      -g a / D^2      g / D
//
//   n = max(#valid, 1e-6),  Ld = sum_valid |x - t| / n,  g = lambda sign(x - t) / n (sign 0 on a tie), 0 on invalid pixels
//
// (a > 0 beside a >= alpha_min: with alpha_min = 0 a pixel nothing was blended into has no expected depth, and D / a would be
// 0 / 0 there.)  Three launches, every one a grid-stride loop over the pixels:
//   depth_loss_reduce_kernel   reads D, a, target, mask (13 B / pixel; 9 in mode 0, which never loads a): per-block partial sums
//                              of |x - t| (double) and of the valid count -- written, not added: nothing to clear beforehand
//   depth_loss_final_kernel    one workgroup: the <= 512 partials in a fixed order, in double; loss[3] = Ld, loss[0] += lambda Ld,
//                              and n for the third kernel
//   depth_loss_cot_kernel      reads the same four and writes cot_depth and cot_alpha (21 B / pixel; 13 in mode 0 without
//                              cot_alpha): every element, zeros on the invalid pixels
// No float atomics anywhere: per thread the pixels in index order, the wave by butterfly, the block's waves and the blocks in
// index order -- two calls on the same inputs give the same bits.  Mode 0 with scale 1, offset 0 is the depth term of
// gs_loss_forward_backward (ssim.hip depth_reduce_kernel / depth_cot_kernel): the count is exact in both, the cotangent is
// the same one division lambda sign / (float)n, so cot_depth agrees with it bit for bit.
#include "gs_ctx.h"
#include "gs_wavesum.h"

namespace gs {

constexpr int DL_THREADS = 256;
constexpr int DL_MAX_BLOCKS = 512;      // the partials' capacity (gs_ctx::depthLossWs: 2 doubles per block + 2)

struct DepthLossArgs {
    int mode;
    float lambda, alphaMin, scale, offset;
};

// is pixel (D, a, masked in) part of the sum, and with which x?
template <int MODE>
__device__ __forceinline__ bool depth_loss_x(float D, float a, float alphaMin, float& x)
{
    if (MODE == GS_DEPTH_ACCUMULATED) { x = D; return true; }
    if (!(a >= alphaMin) || !(a > 0.0f)) return false;
    if (MODE == GS_DEPTH_EXPECTED) { x = D / a; return true; }
    if (!(D > 0.0f)) return false;
    x = a / D;
    return true;
}

template <int MODE>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_reduce_kernel(size_t np, DepthLossArgs p, const float* __restrict__ depth,
                                                                       const float* __restrict__ alpha,
                                                                       const float* __restrict__ target,
                                                                       const unsigned char* __restrict__ mask,
                                                                       double* __restrict__ partials)
{
    __shared__ double smSum[DL_THREADS / 64];
    __shared__ float smCnt[DL_THREADS / 64];
    double sum = 0.0;
    float cnt = 0.0f;      // (whole numbers far below 2^24: exact)
    const size_t stride = (size_t)gridDim.x * DL_THREADS;
    for (size_t i = (size_t)blockIdx.x * DL_THREADS + threadIdx.x; i < np; i += stride) {
        if (mask && !mask[i]) continue;
        float x;
        if (!depth_loss_x<MODE>(depth[i], MODE == GS_DEPTH_ACCUMULATED ? 1.0f : alpha[i], p.alphaMin, x)) continue;
        const float t = p.scale * target[i] + p.offset;
        sum += (double)fabsf(x - t);
        cnt += 1.0f;
    }
    // the wave: the count through the lane swaps of gs_wavesum.h (halves of the wave, rows of a half), then inside the row; the
    // sum, a double, by butterfly as loss_final_kernel's
    cnt = swap_add32(cnt, cnt);
    cnt = swap_add16(cnt, cnt);
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if ((threadIdx.x & 63) == 0) { smSum[threadIdx.x >> 6] = sum; smCnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, c = 0.0;
#pragma unroll
        for (int w = 0; w < DL_THREADS / 64; w++) { s += smSum[w]; c += (double)smCnt[w]; }
        partials[2 * blockIdx.x] = s;
        partials[2 * blockIdx.x + 1] = c;
    }
}

// one workgroup: lossOut[3] = Ld, lossOut[0] += lambda Ld; partials[2 DL_MAX_BLOCKS] = n = max(#valid, 1e-6)
__global__ __launch_bounds__(DL_MAX_BLOCKS) void depth_loss_final_kernel(int nb, float lambda, double* __restrict__ partials,
                                                                        float* __restrict__ lossOut)
{
    __shared__ double sm[DL_MAX_BLOCKS / 64][2];
    double s = 0.0, c = 0.0;
    if ((int)threadIdx.x < nb) { s = partials[2 * threadIdx.x]; c = partials[2 * threadIdx.x + 1]; }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { s += __shfl_xor(s, k, 64); c += __shfl_xor(c, k, 64); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = s; sm[threadIdx.x >> 6][1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = c = 0.0;
        for (int w = 0; w < DL_MAX_BLOCKS / 64; w++) { s += sm[w][0]; c += sm[w][1]; }
        const double safe = c > 1e-6 ? c : 1e-6;
        const double ld = s / safe;
        lossOut[3] = (float)ld;
        lossOut[0] = (float)((double)lossOut[0] + (double)lambda * ld);
        partials[2 * DL_MAX_BLOCKS] = safe;
    }
}

template <int MODE>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_cot_kernel(size_t np, DepthLossArgs p, const float* __restrict__ depth,
                                                                    const float* __restrict__ alpha,
                                                                    const float* __restrict__ target,
                                                                    const unsigned char* __restrict__ mask,
                                                                    const double* __restrict__ partials, float* __restrict__ cotDepth,
                                                                    float* __restrict__ cotAlpha)
{
    const float n = (float)partials[2 * DL_MAX_BLOCKS];
    const size_t stride = (size_t)gridDim.x * DL_THREADS;
    for (size_t i = (size_t)blockIdx.x * DL_THREADS + threadIdx.x; i < np; i += stride) {
        float cd = 0.0f, ca = 0.0f;
        if (!mask || mask[i]) {
            const float D = depth[i], a = MODE == GS_DEPTH_ACCUMULATED ? 1.0f : alpha[i];
            float x;
            if (depth_loss_x<MODE>(D, a, p.alphaMin, x)) {
                const float d = x - (p.scale * target[i] + p.offset);
                const float g = p.lambda * (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f)) / n;
                if (MODE == GS_DEPTH_ACCUMULATED) cd = g;
                else if (MODE == GS_DEPTH_EXPECTED) { cd = g / a; ca = -g * D / (a * a); }
                else { cd = -g * a / (D * D); ca = g / D; }
            }
        }
        cotDepth[i] = cd;
        if (cotAlpha) cotAlpha[i] = ca;
    }
}

// (out may be depth itself: a thread reads its pixel before it writes it, and the two are not declared __restrict__)
__global__ __launch_bounds__(DL_THREADS) void depth_normalize_kernel(size_t np, const float* depth, const float* __restrict__ alpha,
                                                                     float alphaMin, float* out)
{
    const size_t stride = (size_t)gridDim.x * DL_THREADS;
    for (size_t i = (size_t)blockIdx.x * DL_THREADS + threadIdx.x; i < np; i += stride) {
        float x;
        out[i] = depth_loss_x<GS_DEPTH_EXPECTED>(depth[i], alpha[i], alphaMin, x) ? x : 0.0f;
    }
}

long long depth_loss_ws_doubles() { return 2LL * DL_MAX_BLOCKS + 2; }

static inline int dl_blocks(size_t np)
{
    const size_t nb = (np + DL_THREADS - 1) / DL_THREADS;
    return (int)(nb < (size_t)DL_MAX_BLOCKS ? nb : (size_t)DL_MAX_BLOCKS);
}

int launch_depth_loss(gs_ctx* c, int mode, float lambda, float alphaMin, float scale, float offset, const float* depth,
                      const float* alpha, const float* target, const unsigned char* mask, float* loss, float* cotDepth,
                      float* cotAlpha)
{
    const size_t np = (size_t)c->H * c->W;
    if (np == 0) return GS_OK;
    const DepthLossArgs p = {mode, lambda, alphaMin, scale, offset};
    const int nb = dl_blocks(np);
    double* ws = c->depthLossWs;
#define GS_DL_LAUNCH(MODE)                                                                                                     \
    do {                                                                                                                       \
        hipLaunchKernelGGL(depth_loss_reduce_kernel<MODE>, dim3(nb), dim3(DL_THREADS), 0, c->stream, np, p, depth, alpha, target, \
                           mask, ws);                                                                                          \
        hipLaunchKernelGGL(depth_loss_final_kernel, dim3(1), dim3(DL_MAX_BLOCKS), 0, c->stream, nb, lambda, ws, loss);         \
        hipLaunchKernelGGL(depth_loss_cot_kernel<MODE>, dim3(nb), dim3(DL_THREADS), 0, c->stream, np, p, depth, alpha, target,  \
                           mask, ws, cotDepth, cotAlpha);                                                                      \
    } while (0)
    if (mode == GS_DEPTH_ACCUMULATED) GS_DL_LAUNCH(GS_DEPTH_ACCUMULATED);
    else if (mode == GS_DEPTH_EXPECTED) GS_DL_LAUNCH(GS_DEPTH_EXPECTED);
    else GS_DL_LAUNCH(GS_DEPTH_DISPARITY);
#undef GS_DL_LAUNCH
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_depth_normalize(gs_ctx* c, long long n, const float* depth, const float* alpha, float alphaMin, float* out)
{
    if (n <= 0) return GS_OK;
    hipLaunchKernelGGL(depth_normalize_kernel, dim3(dl_blocks((size_t)n)), dim3(DL_THREADS), 0, c->stream, (size_t)n, depth, alpha,
                       alphaMin, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
