// bilateral_grid.hip -- per-view bilateral grid colour correction (include/gsplat.h gs_set_bilateral_grid, DESIGN.md section
// 13; Wang et al. 2024, "Bilateral Guided Radiance Field Processing"): a grid of 3 x 4 affine colour transforms over (x, y,
// luminance), sliced per pixel by its position and the render's luminance, applied before the loss and trained with it.
// Compiled with -ffp-contract=off: every product and sum below is written out (fmaf where the specification has one), so a
// constant grid slices to its value exactly and gives exposure's results bit for bit, and the gradient's sums round the same
// way on every build.
//
// Three passes, one launch each, around the unchanged loss kernel:
//   bilateral_apply_kernel  c = A(p) r + b(p) into the ctx's scratch image (never in place: the fused blend backward reads
//                           the forward's own colour image);
//   bilateral_bwd_kernel    one workgroup per chunk of a cell (a cell: the pixels with the same (x0, y0)): cot <- dL/dr in
//                           place, and per grid layer the chunk's sums over its 4 xy-corners x 12 coefficients (a grid fixed
//                           by the image size and the grid shape, a fixed order, no atomics);
//   bilateral_final_kernel  per node coefficient: the partials of the <= 4 cells around the node, cells in row-major order
//                           and each cell's chunks in order, plus the TV term -> grad.
#include <algorithm>

#include "gs_ctx.h"
#include "gs_expo.h"

namespace gs {

constexpr int BG_THREADS = 256;
constexpr int BG_PPT = 4;                          // pixels per thread of the backward
constexpr int BG_CHUNK = BG_THREADS * BG_PPT;      // pixels per backward workgroup: a cell is cut into chunks of this many
constexpr int BG_MAX_L = 32;                       // grid_l limit (the backward's LDS copy of a cell's columns)

// u = ((2x + 1)(n - 1)) / (2W): one correctly rounded division of two exact integers, on the host and the device alike
__host__ __device__ __forceinline__ float bg_coord(int x, int n, int W)
{
    return (float)((2 * x + 1) * (n - 1)) / (float)(2 * W);
}

__host__ __device__ __forceinline__ int bg_cell(float u, int n)
{
    const int i = (int)u;
    return i < n - 2 ? i : n - 2;
}

__device__ __forceinline__ float bg_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// a pixel's place in the grid: its cell (x0, y0, z0), the fractions (fu, fv, fw), and the guidance gray (unclamped)
struct BgPixel {
    int x0, y0, z0;
    float fu, fv, fw, gray;
};

__device__ __forceinline__ BgPixel bg_pixel(int x, int y, int W, int H, int gw, int gh, int gl, float r0, float r1, float r2)
{
    BgPixel q;
    const float u = bg_coord(x, gw, W), v = bg_coord(y, gh, H);
    q.x0 = bg_cell(u, gw);
    q.fu = u - (float)q.x0;
    q.y0 = bg_cell(v, gh);
    q.fv = v - (float)q.y0;
    q.gray = fmaf(0.299f, r0, fmaf(0.587f, r1, 0.114f * r2));
    const float w = fminf(fmaxf(q.gray, 0.0f), 1.0f) * (float)(gl - 1);
    q.z0 = bg_cell(w, gl);
    q.fw = w - (float)q.z0;
    return q;
}

// a = the trilinear slice (x first, then y, then z: 4 + 2 + 1 lerps per coefficient) and dP = P_hi - P_lo, the bilinear values
// at layers z0 + 1 and z0.  q00, q01, q10, q11: the grid columns G[y0][x0], G[y0][x0 + 1], G[y0 + 1][x0], G[y0 + 1][x0 + 1]
// (gl x 12 floats each)
__device__ __forceinline__ void bg_slice(const float* q00, const float* q01, const float* q10, const float* q11, const BgPixel& q,
                                         float a[12], float dP[12])
{
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const int lo = 12 * q.z0 + k, hi = lo + 12;
        const float plo = bg_lerp(bg_lerp(q00[lo], q01[lo], q.fu), bg_lerp(q10[lo], q11[lo], q.fu), q.fv);
        const float phi = bg_lerp(bg_lerp(q00[hi], q01[hi], q.fu), bg_lerp(q10[hi], q11[hi], q.fu), q.fv);
        a[k] = bg_lerp(plo, phi, q.fw);
        dP[k] = phi - plo;
    }
}

// dL/da at a pixel: da[4c + j] = g[c] r[j], da[4c + 3] = g[c]
__device__ __forceinline__ void bg_da(const float g[3], const float r[3], float da[12])
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int j = 0; j < 3; j++) da[4 * c + j] = g[c] * r[j];
        da[4 * c + 3] = g[c];
    }
}

// in and out may be the same buffer (each thread reads its pixel before it writes it)
__global__ __launch_bounds__(BG_THREADS) void bilateral_apply_kernel(int W, int H, const float* __restrict__ G, int gw, int gh,
                                                                     int gl, const float* in, float* out)
{
    const long long n = (long long)W * H, stride = (long long)gridDim.x * BG_THREADS;
    const size_t col = (size_t)gl * 12;
    for (long long p = (long long)blockIdx.x * BG_THREADS + threadIdx.x; p < n; p += stride) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const float r0 = in[3 * p], r1 = in[3 * p + 1], r2 = in[3 * p + 2];
        const BgPixel q = bg_pixel(x, y, W, H, gw, gh, gl, r0, r1, r2);
        const float* q00 = G + ((size_t)q.y0 * gw + q.x0) * col;
        const float* q10 = q00 + (size_t)gw * col;
        float a[12], dP[12];
        bg_slice(q00, q00 + col, q10, q10 + col, q, a, dP);
        float o[3];
        expo_apply(a, r0, r1, r2, o);
        out[3 * p] = o[0]; out[3 * p + 1] = o[1]; out[3 * p + 2] = o[2];
    }
}

// the first pixel column (or row) of cell c on an axis of W pixels and n nodes (W for c = n - 1): the cell index of a
// pixel never decreases along the axis, so a binary search over the same arithmetic finds the boundary exactly
__device__ __forceinline__ int bg_first(int c, int n, int W)
{
    if (c >= n - 1) return W;
    int lo = 0, hi = W;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bg_cell(bg_coord(mid, n, W), n) >= c) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// One workgroup per (cell, chunk): blockIdx.x = cell * nch + chunk, cell = y0 (gw - 1) + x0; chunk k holds the cell's pixels
// k BG_CHUNK .. (k + 1) BG_CHUNK - 1 in row-major order (a chunk past the cell's pixels writes zeros).  cot holds g = dL/dc
// (the loss kernel's output), render is the caller's uncorrected image.  Rewrites cot with dL/dr and writes, for every layer
// l, partials[(blockIdx.x gl + l) 48 + 12 corner + k] = the chunk's sum of wt(p, node) da_p[k] over the node
// (x0 + (corner & 1), y0 + (corner >> 1), l).  Per thread its pixels in order, then a fixed butterfly over the wave, then the
// four waves in order: the same bits on every run.
__global__ __launch_bounds__(BG_THREADS) void bilateral_bwd_kernel(int W, int H, const float* __restrict__ G, int gw, int gh,
                                                                   int gl, int nch, const float* __restrict__ render,
                                                                   float* __restrict__ cot, float* __restrict__ partials)
{
    __shared__ float cols[4][BG_MAX_L * 12];       // the cell's four xy-corner columns of the grid
    __shared__ float waveSums[BG_THREADS / 64][48];
    const int cell = blockIdx.x / nch, chunk = blockIdx.x - cell * nch;
    const int cx = cell % (gw - 1), cy = cell / (gw - 1);
    const int xs = bg_first(cx, gw, W), xe = bg_first(cx + 1, gw, W);
    const int ys = bg_first(cy, gh, H), ye = bg_first(cy + 1, gh, H);
    const int cw = xe - xs, npx = cw * (ye - ys), first = chunk * BG_CHUNK;
    float* out = partials + (size_t)blockIdx.x * gl * 48;
    if (first >= npx) {                            // an empty cell, or a chunk behind the cell's pixels
        for (int i = threadIdx.x; i < gl * 48; i += BG_THREADS) out[i] = 0.0f;
        return;
    }
    const int col = gl * 12;
    for (int i = threadIdx.x; i < 4 * col; i += BG_THREADS) {
        const int c = i / col, e = i - c * col;
        cols[c][e] = G[((size_t)(cy + (c >> 1)) * gw + cx + (c & 1)) * col + e];
    }
    __syncthreads();
    const float lum[3] = {0.299f, 0.587f, 0.114f};
    const float gscale = (float)(gl - 1);
    float g[BG_PPT][3], r[BG_PPT][3], wxy[BG_PPT][4], fw[BG_PPT];
    int z0[BG_PPT];
#pragma unroll
    for (int j = 0; j < BG_PPT; j++) {
        const int i = first + j * BG_THREADS + threadIdx.x;
        z0[j] = -2;                                // (a slot behind the chunk's pixels: on no layer)
        fw[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) g[j][c] = r[j][c] = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) wxy[j][c] = 0.0f;
        if (i >= npx) continue;
        const int ly = i / cw, x = xs + (i - ly * cw), y = ys + ly;
        const long long p = (long long)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            g[j][c] = cot[3 * p + c];
            r[j][c] = render[3 * p + c];
        }
        const BgPixel q = bg_pixel(x, y, W, H, gw, gh, gl, r[j][0], r[j][1], r[j][2]);
        float a[12], dP[12], da[12], base[3];
        bg_slice(cols[0], cols[1], cols[2], cols[3], q, a, dP);
        expo_vjp(a, g[j][0], g[j][1], g[j][2], base);
        bg_da(g[j], r[j], da);
        float s = dP[0] * da[0];
#pragma unroll
        for (int k = 1; k < 12; k++) s = fmaf(dP[k], da[k], s);
        const float dgray = (q.gray > 0.0f && q.gray < 1.0f) ? s * gscale : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) cot[3 * p + c] = fmaf(dgray, lum[c], base[c]);
        z0[j] = q.z0;
        fw[j] = q.fw;
        const float u0 = 1.0f - q.fu, v0 = 1.0f - q.fv;
        wxy[j][0] = u0 * v0; wxy[j][1] = q.fu * v0; wxy[j][2] = u0 * q.fv; wxy[j][3] = q.fu * q.fv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int l = 0; l < gl; l++) {
        bool mine = false;
#pragma unroll
        for (int j = 0; j < BG_PPT; j++) mine = mine || z0[j] == l || z0[j] + 1 == l;
        if (!__syncthreads_or(mine)) {             // no pixel of the chunk reaches this layer (uniform over the workgroup)
            if (threadIdx.x < 48) out[l * 48 + threadIdx.x] = 0.0f;
            continue;
        }
        float acc[48];
#pragma unroll
        for (int k = 0; k < 48; k++) acc[k] = 0.0f;
#pragma unroll
        for (int j = 0; j < BG_PPT; j++) {
            if (z0[j] != l && z0[j] + 1 != l) continue;
            const float wz = z0[j] == l ? 1.0f - fw[j] : fw[j];
            float da[12];
            bg_da(g[j], r[j], da);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float wt = wxy[j][c] * wz;
#pragma unroll
                for (int k = 0; k < 12; k++) acc[12 * c + k] = fmaf(wt, da[k], acc[12 * c + k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 48; k++) {
            float s = acc[k];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            acc[k] = s;
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 48; k++) waveSums[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < 48) {
            float s = waveSums[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < BG_THREADS / 64; w++) s += waveSums[w][threadIdx.x];
            out[l * 48 + threadIdx.x] = s;
        }
        // (the next layer's __syncthreads_or orders these reads before the next writes of waveSums)
    }
}

// One thread per node coefficient t = 12 node + k, node = (y gw + x) gl + z: the partials of the <= 4 cells around the node
// (cells in row-major order, each cell's chunks in order), plus tv_weight times the gradient of
// TV(G) = sum over the axes of (1 / n_axis) sum (G_next - G)^2, overwriting grad[t].
__global__ __launch_bounds__(BG_THREADS) void bilateral_final_kernel(const float* __restrict__ G, int gw, int gh, int gl, int nch,
                                                                     float tvWeight, const float* __restrict__ partials,
                                                                     float* __restrict__ grad)
{
    const int t = blockIdx.x * BG_THREADS + threadIdx.x;
    if (t >= gw * gh * gl * 12) return;
    const int k = t % 12, node = t / 12;
    const int z = node % gl, x = (node / gl) % gw, y = node / (gl * gw);
    float sum = 0.0f;
    for (int dy = 1; dy >= 0; dy--) {
        const int cy = y - dy;
        if (cy < 0 || cy > gh - 2) continue;
        for (int dx = 1; dx >= 0; dx--) {
            const int cx = x - dx;
            if (cx < 0 || cx > gw - 2) continue;
            const float* q = partials + ((size_t)(cy * (gw - 1) + cx) * nch * gl + z) * 48 + 12 * (2 * dy + dx) + k;
            for (int c = 0; c < nch; c++) sum += q[(size_t)c * gl * 48];
        }
    }
    // d TV / dG = sum over the axes of (2 / n_axis) ((G - G_prev) - (G_next - G)), a missing neighbour's term left out
    const float* gn = G + t;
    const float v = gn[0];
    const int pos[3] = {x, y, z}, len[3] = {gw, gh, gl};
    const long long step[3] = {(long long)gl * 12, (long long)gw * gl * 12, 12};
    float tv = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float d = 0.0f;
        if (pos[a] > 0) d = v - gn[-step[a]];
        if (pos[a] < len[a] - 1) d = d - (gn[step[a]] - v);
        const long long terms = 12LL * gw * gh * gl / len[a] * (len[a] - 1);
        tv = fmaf(2.0f / (float)terms, d, tv);
    }
    grad[t] = sum + tvWeight * tv;
}

bool bilateral_shape_ok(int gw, int gh, int gl)
{
    return gw >= 2 && gw <= 64 && gh >= 2 && gh <= 64 && gl >= 2 && gl <= BG_MAX_L;
}

// the most pixels any cell holds along an axis of W pixels and n nodes (the host runs the device's arithmetic)
static int bg_widest_cell(int n, int W)
{
    int best = 0, run = 0, prev = -1;
    for (int x = 0; x < W; x++) {
        const int c = bg_cell(bg_coord(x, n, W), n);
        run = c == prev ? run + 1 : 1;
        prev = c;
        best = std::max(best, run);
    }
    return best;
}

int bilateral_chunks(int W, int H, int gw, int gh)
{
    const long long most = (long long)bg_widest_cell(gw, W) * bg_widest_cell(gh, H);
    return (int)std::max(1LL, (most + BG_CHUNK - 1) / BG_CHUNK);
}

long long bilateral_partials_floats(int gw, int gh, int gl, int nch) { return 48LL * (gw - 1) * (gh - 1) * nch * gl; }

int launch_bilateral_apply(gs_ctx* c, int W, int H, const float* G, int gw, int gh, int gl, const float* in, float* out)
{
    const long long n = (long long)W * H;
    if (n <= 0) return GS_OK;
    const long long nb = std::min(4096LL, (n + BG_THREADS - 1) / BG_THREADS);
    hipLaunchKernelGGL(bilateral_apply_kernel, dim3((unsigned)nb), dim3(BG_THREADS), 0, c->stream, W, H, G, gw, gh, gl, in, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_bilateral_backward(gs_ctx* c, int W, int H, const float* G, int gw, int gh, int gl, int nch, float tvWeight,
                              const float* render, float* cot, float* partials, float* grad)
{
    const unsigned blocks = (unsigned)((gw - 1) * (gh - 1) * nch);
    hipLaunchKernelGGL(bilateral_bwd_kernel, dim3(blocks), dim3(BG_THREADS), 0, c->stream, W, H, G, gw, gh, gl, nch, render, cot,
                       partials);
    const int coeffs = gw * gh * gl * 12;
    hipLaunchKernelGGL(bilateral_final_kernel, dim3((unsigned)((coeffs + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0,
                       c->stream, G, gw, gh, gl, nch, tvWeight, partials, grad);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
