// metrics.hip -- held-out evaluation: PSNR / SSIM sums of a render against its target and the colour moments of the best affine
// colour transform between them (include/gsplat.h gs_image_metrics / gs_colour_moments; DESIGN.md section 24;
// tests/metrics_numpy.py restates both in numpy).
//
//   r, g = clamp(render, 0, 1), clamp(target, 0, 1);  w = (float)mask / 255.0f per pixel, 1 without a mask
//   sse      = sum_pixels w sum_c (r_c - g_c)^2                       wsum = sum_pixels w
//   ssim_sum = sum_{pixels, c} w ssim_map(w r, w g)                   ssim_map: Inria's loss_utils.ssim -- the CENTRED 11 x 11
//              Gaussian window (sigma 1.5), taps outside the image zero, C1 = 1e-4, C2 = 9e-4
//   out      = {sse, ssim_sum, wsum, 3 wsum}:  psnr = -10 log10(sse / out[3]),  ssim = ssim_sum / out[3]
//
// image_metrics_kernel is the forward-only sibling of ssim.hip's loss_fused_kernel: one workgroup takes a MT x MT tile of one
// channel, stages the (MT+10)^2 patch of both images in LDS -- clamped, and weighted on the way in --, runs the separable
// window (rows, then columns, taps ascending) for the five statistics mu1, mu2, E11, E22, E12 and forms the SSIM value of its
// own pixels.  The squared error and the weight of a tile's own pixels are taken where the patch is staged, from the values
// before the weighting.  Nothing but the two images and the mask is read and nothing but three doubles per block is written:
// no statistic map ever leaves LDS.  The file is built with -ffp-contract=off: every product and sum below is rounded as
// written, which is what the float32 mirror of the tests evaluates, and a mask of all 255 (w = 1.0f) gives the bits of no mask.
//
// No float atomics: a thread sums its own values in a fixed order into doubles, the wave by butterfly, the block's waves in
// index order (depth_loss.hip's reduction), the blocks' partials -- written, not added: nothing to clear -- in index order by
// one workgroup.  Two calls on the same inputs give the same bits.
#include "gs_ctx.h"

namespace gs {

constexpr int MK = 11, MPAD = 5;            // the window and its reach
constexpr float MET_C1 = 0.0001f, MET_C2 = 0.0009f;
// Tile.  The passes cost ((MT+10) MT + MT MT) 55 multiply-adds per tile, 127 per pixel at 32 x 32 against 110 with no halo at
// all and 144 at 32 x 16; the patches and the row sums then take 43 KB of LDS: three workgroups a CU (160 KB).  256 threads:
// the column pass has exactly one item a thread (32 columns x 8 strips of four rows), the row pass 42 rows x 6 strips.
constexpr int MT = 32, MNT = 256;
constexpr int MP = MT + MK - 1;             // patch edge: 42
constexpr int MPS = MP + 1;                 // patch row stride in LDS (odd: a wave's lanes run down the rows)
constexpr int MHS = MT + 1;                 // row-sum row stride in LDS (odd, likewise, for the row pass's stores)
// outputs per work item of a pass: the shortest strips with which the pass's items fit the block's threads in one round
constexpr int MHW = 6, MVW = 4;             // row pass: 42 rows x 6 strips of six columns; column pass: 32 columns x 8 strips of four rows
static_assert(MP * ((MT + MHW - 1) / MHW) <= MNT && MT * ((MT + MVW - 1) / MVW) <= MNT, "one round per pass");
constexpr int MM_THREADS = 256, MM_MAX_BLOCKS = 512, MM_N = 22;      // colour_moments_kernel

struct MetricTaps {
    float g[MK];
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__device__ __forceinline__ double wave_sum_double(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// Block -> (tile, channel) as loss_fused_kernel's: workgroups go round-robin over the 8 XCDs; XCD x owns a contiguous band of
// tiles and its consecutive blocks are the three channels of one tile, so the second and third find the interleaved RGB lines
// in that XCD's L2.  The grid is 8 * 3 * perXcd blocks; a block beyond the last tile writes a zero partial.
template <bool MASK>
__global__ __launch_bounds__(MNT) void image_metrics_kernel(int H, int W, int ntx, int nty, const float* __restrict__ img1,
                                                           const float* __restrict__ img2,
                                                           const unsigned char* __restrict__ mask, MetricTaps taps,
                                                           double* __restrict__ partials)
{
    __shared__ float in1[MP * MPS], in2[MP * MPS];      // w r, w g
    __shared__ float Hs[5][MP * MHS];                   // row sums of a, b, a a, b b, a b: rows = patch rows, cols = tile cols
    __shared__ float ownW[MASK ? MT * MT : 1];          // the weights of the tile's own pixels
    __shared__ double red[MNT / 64][3];
    const float* const g = taps.g;
    const int tid = threadIdx.x;
    const int nTiles = ntx * nty, perXcd = (nTiles + 7) >> 3;
    const int seq = (int)(blockIdx.x >> 3), tileId = (int)(blockIdx.x & 7u) * perXcd + seq / 3, c = seq % 3;
    if (tileId >= nTiles) {             // whole block
        if (tid < 3) partials[(size_t)blockIdx.x * 3 + tid] = 0.0;
        return;
    }
    const int ty = tileId / ntx, tx = tileId - ty * ntx;
    const int h0 = ty * MT, w0 = tx * MT;
    double sse = 0.0, wsum = 0.0, ssimSum = 0.0;
    {   // the two patches: all of a thread's loads are issued before the first is used (unconditional, from clamped addresses)
        constexpr int NLD = (MP * MP + MNT - 1) / MNT;
        float va[NLD], vb[NLD];
        unsigned char vm[MASK ? NLD : 1];
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + k * MNT;
            const int r = i / MP, q = i - r * MP;
            const int shc = min(max(h0 - MPAD + r, 0), H - 1), swc = min(max(w0 - MPAD + q, 0), W - 1);
            const size_t si = ((size_t)shc * W + swc) * 3 + c;
            va[k] = img1[si]; vb[k] = img2[si];
            if constexpr (MASK) vm[k] = mask[(size_t)shc * W + swc];
        }
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + k * MNT;
            const int r = i / MP, q = i - r * MP;
            const int sh = h0 - MPAD + r, sw = w0 - MPAD + q;
            const bool inside = sh >= 0 && sh < H && sw >= 0 && sw < W;
            float a = clamp01(va[k]), b = clamp01(vb[k]);
            float w = 1.0f;
            if constexpr (MASK) w = (float)vm[k] / 255.0f;
            const bool own = r >= MPAD && r < MPAD + MT && q >= MPAD && q < MPAD + MT;
            if (own && inside && i < MP * MP) {
                const float d = a - b;
                float e = d * d;
                if constexpr (MASK) { e = w * e; ownW[(r - MPAD) * MT + (q - MPAD)] = w; }
                sse += (double)e;
                if (c == 0) wsum += (double)w;          // once per pixel, not once per channel
            }
            if constexpr (MASK) { a = w * a; b = w * b; }
            if (i < MP * MP) {
                in1[r * MPS + q] = inside ? a : 0.0f;
                in2[r * MPS + q] = inside ? b : 0.0f;
            }
        }
    }
    __syncthreads();
    // row pass: tile column x sums patch columns x .. x+10.  Item = (patch row r, strip of HW tile columns), r fastest: a wave's
    // lanes read and write different rows, an odd stride apart.
    {
        constexpr int HW = MHW, SH = (MT + HW - 1) / HW;
        for (int it = tid; it < MP * SH; it += MNT) {
            const int sidx = it / MP, r = it - sidx * MP;
            const int q0 = HW * sidx, nout = min(HW, MT - q0);
            float a[HW + 10], b[HW + 10], aa[HW + 10], bb[HW + 10], ab[HW + 10];
#pragma unroll
            for (int i = 0; i < HW + 10; i++) {
                const bool ok = q0 + i < MP;
                a[i] = ok ? in1[r * MPS + q0 + i] : 0.0f;
                b[i] = ok ? in2[r * MPS + q0 + i] : 0.0f;
                aa[i] = a[i] * a[i]; bb[i] = b[i] * b[i]; ab[i] = a[i] * b[i];
            }
#pragma unroll
            for (int j = 0; j < HW; j++) {
                if (j < nout) {
                    float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
                    for (int k = 0; k < MK; k++) {
                        const float wk = g[k];
                        s1 = s1 + wk * a[j + k]; s2 = s2 + wk * b[j + k];
                        s11 = s11 + wk * aa[j + k]; s22 = s22 + wk * bb[j + k]; s12 = s12 + wk * ab[j + k];
                    }
                    const int o = r * MHS + q0 + j;
                    Hs[0][o] = s1; Hs[1][o] = s2; Hs[2][o] = s11; Hs[3][o] = s22; Hs[4][o] = s12;
                }
            }
        }
    }
    __syncthreads();
    // column pass and the SSIM value of the tile's own pixels.  Item = (tile column q, strip of VW tile rows), q fastest.
    {
        constexpr int VW = MVW, SV = (MT + VW - 1) / VW;
        for (int it = tid; it < MT * SV; it += MNT) {
            const int sp = it / MT, q = it - sp * MT;
            const int p0 = VW * sp, nout = min(VW, MT - p0);
            float st[5][VW];
#pragma unroll
            for (int pl = 0; pl < 5; pl++) {
                float col[VW + 10];
#pragma unroll
                for (int i = 0; i < VW + 10; i++) col[i] = (p0 + i < MP) ? Hs[pl][(p0 + i) * MHS + q] : 0.0f;
#pragma unroll
                for (int j = 0; j < VW; j++) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < MK; k++) acc = acc + g[k] * col[j + k];
                    st[pl][j] = acc;
                }
            }
#pragma unroll
            for (int j = 0; j < VW; j++) {
                const int pp = p0 + j;
                if (j < nout && h0 + pp < H && w0 + q < W) {
                    const float m1 = st[0][j], m2 = st[1][j], E11 = st[2][j], E22 = st[3][j], E12 = st[4][j];
                    const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
                    const float s1 = E11 - m11, s2 = E22 - m22, s12 = E12 - m12;
                    const float num = (2.0f * m12 + MET_C1) * (2.0f * s12 + MET_C2);
                    const float den = (m11 + m22 + MET_C1) * (s1 + s2 + MET_C2);
                    float v = num / den;
                    if constexpr (MASK) v = ownW[pp * MT + q] * v;
                    ssimSum += (double)v;
                }
            }
        }
    }
    ssimSum = wave_sum_double(ssimSum); sse = wave_sum_double(sse); wsum = wave_sum_double(wsum);
    if ((tid & 63) == 0) { red[tid >> 6][0] = ssimSum; red[tid >> 6][1] = sse; red[tid >> 6][2] = wsum; }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < MNT / 64; k++) s += red[k][tid];
        partials[(size_t)blockIdx.x * 3 + tid] = s;
    }
}

// one workgroup: the nb partials (ssim_sum, sse, wsum) in index order; out = {sse, ssim_sum, wsum, 3 wsum}
__global__ __launch_bounds__(MNT) void image_metrics_final_kernel(int nb, const double* __restrict__ partials,
                                                                 double* __restrict__ out)
{
    __shared__ double sm[MNT / 64][3];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nb; i += MNT) {
        a += partials[(size_t)i * 3]; b += partials[(size_t)i * 3 + 1]; c += partials[(size_t)i * 3 + 2];
    }
    a = wave_sum_double(a); b = wave_sum_double(b); c = wave_sum_double(c);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; sm[threadIdx.x >> 6][2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = c = 0.0;
        for (int w = 0; w < MNT / 64; w++) { a += sm[w][0]; b += sm[w][1]; c += sm[w][2]; }
        out[0] = b; out[1] = a; out[2] = c; out[3] = 3.0 * c;
    }
}

// The 22 moment sums of the affine colour fit, p = (r, g, b, 1) the clamped render, t the clamped target:
//   m[0..9]   S[i][j] = sum w p_i p_j, upper triangle by rows: 00 01 02 03 11 12 13 22 23 33  (S[3][3] = sum w)
//   m[10..21] T[i][c] = sum w p_i t_c, m[10 + 3 i + c]
// A grid-stride loop, every product and sum in double; per-block partials [block][22], written.
template <bool MASK>
__global__ __launch_bounds__(MM_THREADS) void colour_moments_kernel(size_t np, const float* __restrict__ render,
                                                                   const float* __restrict__ target,
                                                                   const unsigned char* __restrict__ mask,
                                                                   double* __restrict__ partials)
{
    __shared__ double sm[MM_THREADS / 64][MM_N];
    double m[MM_N];
#pragma unroll
    for (int k = 0; k < MM_N; k++) m[k] = 0.0;
    const size_t stride = (size_t)gridDim.x * MM_THREADS;
    for (size_t i = (size_t)blockIdx.x * MM_THREADS + threadIdx.x; i < np; i += stride) {
        double w = 1.0;
        if constexpr (MASK) w = (double)((float)mask[i] / 255.0f);
        const double p[4] = {(double)clamp01(render[3 * i]), (double)clamp01(render[3 * i + 1]), (double)clamp01(render[3 * i + 2]), 1.0};
        const double t[3] = {(double)clamp01(target[3 * i]), (double)clamp01(target[3 * i + 1]), (double)clamp01(target[3 * i + 2])};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const double wp = w * p[a];
#pragma unroll
            for (int b = a; b < 4; b++) m[k++] += wp * p[b];
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const double wp = w * p[a];
#pragma unroll
            for (int cc = 0; cc < 3; cc++) m[10 + 3 * a + cc] += wp * t[cc];
        }
    }
#pragma unroll
    for (int k = 0; k < MM_N; k++) m[k] = wave_sum_double(m[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < MM_N; k++) sm[threadIdx.x >> 6][k] = m[k];
    }
    __syncthreads();
    if (threadIdx.x < MM_N) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < MM_THREADS / 64; w++) s += sm[w][threadIdx.x];
        partials[(size_t)blockIdx.x * MM_N + threadIdx.x] = s;
    }
}

// one workgroup of 16 waves, wave v the moments v and v + 16: a lane sums the blocks lane, lane + 64, ... in that order, the
// wave by butterfly
__global__ __launch_bounds__(1024) void colour_moments_final_kernel(int nb, const double* __restrict__ partials,
                                                                   double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < MM_N; k += 16) {      // (uniform per wave)
        double s = 0.0;
        for (int b = lane; b < nb; b += 64) s += partials[(size_t)b * MM_N + k];
        s = wave_sum_double(s);
        if (lane == 0) out[k] = s;
    }
}

// ---- launchers --------------------------------------------------------------------------------
static inline int metrics_blocks(int H, int W)
{
    const long long nTiles = (long long)gs_div_up(W, MT) * gs_div_up(H, MT);
    return (int)(8 * 3 * ((nTiles + 7) / 8));
}

// doubles of workspace (gs_ctx::metricsWs) that both entry points are served from at an H x W image
long long metrics_ws_doubles(int H, int W)
{
    const long long a = 3LL * metrics_blocks(H, W), b = (long long)MM_N * MM_MAX_BLOCKS;
    return a > b ? a : b;
}

int launch_image_metrics(gs_ctx* c, int H, int W, const float* render, const float* target, const unsigned char* mask, double* out)
{
    if (H == 0 || W == 0) {
        GS_HIP_CHECK(c, hipMemsetAsync(out, 0, 4 * sizeof(double), c->stream));
        return GS_OK;
    }
    MetricTaps taps;
    {   // Inria's gaussian(11, 1.5): exp(-(x - 5)^2 / (2 sigma^2)), normalised -- centred, unlike gs_ssim_window's
        float sum = 0.0f;
        for (int x = 0; x < MK; x++) {
            const float d = (float)(x - MK / 2);
            taps.g[x] = expf(-(d * d) / (2.0f * (1.5f * 1.5f)));
            sum += taps.g[x];
        }
        for (int x = 0; x < MK; x++) taps.g[x] = taps.g[x] / sum;
    }
    const int ntx = gs_div_up(W, MT), nty = gs_div_up(H, MT), nb = metrics_blocks(H, W);
    if (mask)
        hipLaunchKernelGGL(image_metrics_kernel<true>, dim3(nb), dim3(MNT), 0, c->stream, H, W, ntx, nty, render, target, mask, taps,
                           c->metricsWs);
    else
        hipLaunchKernelGGL(image_metrics_kernel<false>, dim3(nb), dim3(MNT), 0, c->stream, H, W, ntx, nty, render, target, mask, taps,
                           c->metricsWs);
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3(1), dim3(MNT), 0, c->stream, nb, c->metricsWs, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_colour_moments(gs_ctx* c, long long n, const float* render, const float* target, const unsigned char* mask, double* out)
{
    if (n == 0) {
        GS_HIP_CHECK(c, hipMemsetAsync(out, 0, MM_N * sizeof(double), c->stream));
        return GS_OK;
    }
    const size_t np = (size_t)n, want = (np + MM_THREADS - 1) / MM_THREADS;
    const int nb = (int)(want < (size_t)MM_MAX_BLOCKS ? want : (size_t)MM_MAX_BLOCKS);
    if (mask)
        hipLaunchKernelGGL(colour_moments_kernel<true>, dim3(nb), dim3(MM_THREADS), 0, c->stream, np, render, target, mask, c->metricsWs);
    else
        hipLaunchKernelGGL(colour_moments_kernel<false>, dim3(nb), dim3(MM_THREADS), 0, c->stream, np, render, target, mask, c->metricsWs);
    hipLaunchKernelGGL(colour_moments_final_kernel, dim3(1), dim3(1024), 0, c->stream, nb, c->metricsWs, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
