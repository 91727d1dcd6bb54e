// normal_loss.hip -- normal regularisation from the render's depth and alpha images (include/gsplat.h gs_normal_loss /
// gs_depth_normals; tests/normal_loss_numpy.py restates it in numpy).
//
//   Pixel (i, j) (column, row) has the ray (rx, ry, 1), rx = ((i + 0.5) - cx) / fx, ry = ((j + 0.5) - cy) / fy, and the expected
//   depth z = D / a where it is depth-valid: a >= alpha_min, a > 0, D > 0.  An interior pixel whose four neighbours and itself
//   are depth-valid (and, with max_jump > 0, max(|A|, |B|) <= max_jump z) has the normal n = m / |m|,
//     A = z+ - z-,  S = (z+ + z-) / fx,  B = zd - zu,  T = (zd + zu) / fy,  m = (A T, B S, -((A T rx + B S ry) + S T))
//   which is (Pdown - Pup) x (Pright - Pleft) of the back-projected points with only A and B cancelling.  The file is built with
//   -ffp-contract=off: every product and sum below is rounded as written, and the numpy restatement follows the same order.
//
// Five launches, every one a grid-stride loop over the pixels (256 threads; the reduction at most 512 blocks, the per-pixel
// kernels at most 8192):
//   normals_kernel        reads D, a at the pixel and its four neighbours (8 B / pixel from memory, the rest from cache), writes
//                         n (12 B / pixel), the zero vector where there is no normal
//   nl_reduce_kernel      reads n at the pixel, its right and its lower neighbour, the target, the mask and the edge image
//                         (12 + 12 + 1 + 12 B / pixel): per-block partial sums of the three terms (double) and the two counts
//   nl_final_kernel       one workgroup: the <= 512 partials in a fixed order, in double; normal_out[3], loss[0] +=, and the two
//                         denominators for the fourth kernel
//   nl_q_kernel           reads n at the pixel and its four neighbours, D, a as normals_kernel does, target, mask, edge image;
//                         writes q = (q+, q-, qd, qu), the term's derivative by the four neighbours' z (16 B / pixel)
//   nl_gather_kernel      reads q at the four neighbours, D, a; writes (or adds to) cot_depth and cot_alpha (16 + 8 + 8 B / pixel)
// The fourth kernel writes what a pixel's normal does to its neighbours, the fifth GATHERS it: no float atomics anywhere, per
// thread the pixels in index order, the wave through gs_wavesum.h's lane swaps, the block's waves and the blocks in index
// order -- two calls on the same inputs give the same bits.
#include "gs_ctx.h"
#include "gs_wavesum.h"

namespace gs {

constexpr int NL_THREADS = 256;
constexpr int NL_MAX_BLOCKS = 512;      // the partials' capacity: 5 doubles per block + 2
constexpr int NL_PART = 5;              // sum l1, sum cos, sum smooth, #prior pixels, #pairs

struct NormalArgs {
    float fx, fy, cx, cy;
    int H, W;
    float lamL1, lamCos, lamS, alphaMin, maxJump, gamma;
    int accumulate;
};

// what a pixel's normal is made of; everything the q kernel differentiates
struct NormalGeom {
    float A, B, S, T, rx, ry, len, nx, ny, nz;
};

// the row of pixel k (a 32-bit division wherever the index fits: the 64-bit one is a long sequence)
__device__ __forceinline__ int nl_row(size_t k, int W)
{
    return (k >> 32) == 0 ? (int)((unsigned)k / (unsigned)W) : (int)(k / (size_t)W);
}

__device__ __forceinline__ bool nl_z(const float* __restrict__ depth, const float* __restrict__ alpha, size_t p, float alphaMin,
                                     float& z)
{
    const float D = depth[p], a = alpha[p];
    if (!(a >= alphaMin) || !(a > 0.0f) || !(D > 0.0f)) return false;
    z = D / a;
    return true;
}

// does pixel (i, j) have a normal, and which?
__device__ __forceinline__ bool nl_geom(const NormalArgs& p, const float* __restrict__ depth, const float* __restrict__ alpha, int i,
                                        int j, NormalGeom& g)
{
    if (i < 1 || i > p.W - 2 || j < 1 || j > p.H - 2) return false;
    const size_t c = (size_t)j * p.W + i;
    float z, zp, zm, zd, zu;
    if (!nl_z(depth, alpha, c, p.alphaMin, z) || !nl_z(depth, alpha, c + 1, p.alphaMin, zp) ||
        !nl_z(depth, alpha, c - 1, p.alphaMin, zm) || !nl_z(depth, alpha, c + p.W, p.alphaMin, zd) ||
        !nl_z(depth, alpha, c - p.W, p.alphaMin, zu))
        return false;
    g.A = zp - zm;
    g.B = zd - zu;
    if (p.maxJump > 0.0f && !(fmaxf(fabsf(g.A), fabsf(g.B)) <= p.maxJump * z)) return false;
    g.S = (zp + zm) / p.fx;
    g.T = (zd + zu) / p.fy;
    g.rx = (((float)i + 0.5f) - p.cx) / p.fx;
    g.ry = (((float)j + 0.5f) - p.cy) / p.fy;
    const float mx = g.A * g.T, my = g.B * g.S;
    const float mz = -((mx * g.rx + my * g.ry) + g.S * g.T);
    g.len = sqrtf((mx * mx + my * my) + mz * mz);
    if (!(g.len > 0.0f)) return false;
    g.nx = mx / g.len;
    g.ny = my / g.len;
    g.nz = mz / g.len;
    return true;
}

__global__ __launch_bounds__(NL_THREADS) void normals_kernel(size_t np, NormalArgs p, const float* __restrict__ depth,
                                                             const float* __restrict__ alpha, float* __restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * NL_THREADS;
    for (size_t k = (size_t)blockIdx.x * NL_THREADS + threadIdx.x; k < np; k += stride) {
        const int j = nl_row(k, p.W), i = (int)(k - (size_t)j * p.W);
        NormalGeom g;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (nl_geom(p, depth, alpha, i, j, g)) { nx = g.nx; ny = g.ny; nz = g.nz; }
        out[3 * k] = nx;
        out[3 * k + 1] = ny;
        out[3 * k + 2] = nz;
    }
}

// a stored normal: a unit vector, or the zero vector where the pixel has none
__device__ __forceinline__ bool nl_load(const float* __restrict__ normals, size_t k, float& x, float& y, float& z)
{
    x = normals[3 * k];
    y = normals[3 * k + 1];
    z = normals[3 * k + 2];
    return x != 0.0f || y != 0.0f || z != 0.0f;
}

// the pair's weight exp(-gamma mean_c |I_p - I_q|); exactly 1 without an edge image or with gamma = 0
__device__ __forceinline__ float nl_weight(const float* __restrict__ edge, float gamma, size_t a, size_t b)
{
    if (!edge || !(gamma > 0.0f)) return 1.0f;
    const float d = ((fabsf(edge[3 * a] - edge[3 * b]) + fabsf(edge[3 * a + 1] - edge[3 * b + 1])) +
                     fabsf(edge[3 * a + 2] - edge[3 * b + 2])) / 3.0f;
    return expf(-gamma * d);
}

// the pixel's target, normalised; false on a hole (squared norm < 0.25), a cleared mask or no target at all
__device__ __forceinline__ bool nl_target(const float* __restrict__ target, const unsigned char* __restrict__ mask, size_t k, float& tx,
                                          float& ty, float& tz)
{
    if (!target || (mask && !mask[k])) return false;
    tx = target[3 * k];
    ty = target[3 * k + 1];
    tz = target[3 * k + 2];
    const float s = (tx * tx + ty * ty) + tz * tz;
    if (!(s >= 0.25f)) return false;
    const float l = sqrtf(s);
    tx = tx / l;
    ty = ty / l;
    tz = tz / l;
    return true;
}

__device__ __forceinline__ float nl_wave_count(float cnt)
{   // whole numbers far below 2^24: exact.  Halves of the wave, rows of a half (gs_wavesum.h), then inside the row
    cnt = swap_add32(cnt, cnt);
    cnt = swap_add16(cnt, cnt);
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    return cnt;
}

__device__ __forceinline__ double nl_wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(NL_THREADS) void nl_reduce_kernel(size_t np, NormalArgs p, const float* __restrict__ normals,
                                                               const float* __restrict__ target,
                                                               const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ edge, double* __restrict__ partials)
{
    __shared__ double sm[NL_THREADS / 64][NL_PART];
    double sL1 = 0.0, sCos = 0.0, sS = 0.0;
    float cP = 0.0f, cS = 0.0f;
    const size_t stride = (size_t)gridDim.x * NL_THREADS;
    for (size_t k = (size_t)blockIdx.x * NL_THREADS + threadIdx.x; k < np; k += stride) {
        float nx, ny, nz;
        if (!nl_load(normals, k, nx, ny, nz)) continue;
        float tx, ty, tz;
        if (nl_target(target, mask, k, tx, ty, tz)) {
            sL1 += (double)((fabsf(nx - tx) + fabsf(ny - ty)) + fabsf(nz - tz));
            sCos += (double)(1.0f - ((nx * tx + ny * ty) + nz * tz));
            cP += 1.0f;
        }
        // the pairs this pixel opens: with its right and its lower neighbour (a pixel with a normal is interior, so both exist)
        float qx, qy, qz;
        if (nl_load(normals, k + 1, qx, qy, qz)) {
            sS += (double)(nl_weight(edge, p.gamma, k, k + 1) * (1.0f - ((nx * qx + ny * qy) + nz * qz)));
            cS += 1.0f;
        }
        if (nl_load(normals, k + p.W, qx, qy, qz)) {
            sS += (double)(nl_weight(edge, p.gamma, k, k + p.W) * (1.0f - ((nx * qx + ny * qy) + nz * qz)));
            cS += 1.0f;
        }
    }
    sL1 = nl_wave_sum(sL1);
    sCos = nl_wave_sum(sCos);
    sS = nl_wave_sum(sS);
    cP = nl_wave_count(cP);
    cS = nl_wave_count(cS);
    if ((threadIdx.x & 63) == 0) {
        double* row = sm[threadIdx.x >> 6];
        row[0] = sL1; row[1] = sCos; row[2] = sS; row[3] = (double)cP; row[4] = (double)cS;
    }
    __syncthreads();
    if (threadIdx.x < NL_PART) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NL_THREADS / 64; w++) s += sm[w][threadIdx.x];
        partials[(size_t)NL_PART * blockIdx.x + threadIdx.x] = s;
    }
}

// one workgroup: normalOut = (L_l1, L_cos, L_s), lossOut[0] += their weighted sum; partials[NL_PART NL_MAX_BLOCKS + 0 | 1] =
// max(#prior pixels, 1e-6) | max(#pairs, 1e-6)
__global__ __launch_bounds__(NL_MAX_BLOCKS) void nl_final_kernel(int nb, NormalArgs p, double* __restrict__ partials,
                                                                 float* __restrict__ lossOut, float* __restrict__ normalOut)
{
    __shared__ double sm[NL_MAX_BLOCKS / 64][NL_PART];
    double v[NL_PART];
#pragma unroll
    for (int q = 0; q < NL_PART; q++) {
        v[q] = (int)threadIdx.x < nb ? partials[(size_t)NL_PART * threadIdx.x + q] : 0.0;
        v[q] = nl_wave_sum(v[q]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NL_PART; q++) sm[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NL_PART; q++) {
            v[q] = 0.0;
            for (int w = 0; w < NL_MAX_BLOCKS / 64; w++) v[q] += sm[w][q];
        }
        const double nP = v[3] > 1e-6 ? v[3] : 1e-6, nS = v[4] > 1e-6 ? v[4] : 1e-6;
        const double l1 = v[0] / nP, lc = v[1] / nP, ls = v[2] / nS;
        normalOut[0] = (float)l1;
        normalOut[1] = (float)lc;
        normalOut[2] = (float)ls;
        lossOut[0] = (float)((double)lossOut[0] + (((double)p.lamL1 * l1 + (double)p.lamCos * lc) + (double)p.lamS * ls));
        partials[(size_t)NL_PART * NL_MAX_BLOCKS] = nP;
        partials[(size_t)NL_PART * NL_MAX_BLOCKS + 1] = nS;
    }
}

__global__ __launch_bounds__(NL_THREADS) void nl_q_kernel(size_t np, NormalArgs p, const float* __restrict__ depth,
                                                          const float* __restrict__ alpha, const float* __restrict__ normals,
                                                          const float* __restrict__ target, const unsigned char* __restrict__ mask,
                                                          const float* __restrict__ edge, const double* __restrict__ partials,
                                                          float4* __restrict__ q)
{
    const float nP = (float)partials[(size_t)NL_PART * NL_MAX_BLOCKS], nS = (float)partials[(size_t)NL_PART * NL_MAX_BLOCKS + 1];
    const float wS = p.lamS / nS;
    const size_t stride = (size_t)gridDim.x * NL_THREADS;
    for (size_t k = (size_t)blockIdx.x * NL_THREADS + threadIdx.x; k < np; k += stride) {
        const int j = nl_row(k, p.W), i = (int)(k - (size_t)j * p.W);
        NormalGeom g;
        float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (nl_geom(p, depth, alpha, i, j, g)) {
            // g_n: the prior terms, then the four pairs (right, left, down, up)
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            float tx, ty, tz;
            if (nl_target(target, mask, k, tx, ty, tz)) {
                const float dx = g.nx - tx, dy = g.ny - ty, dz = g.nz - tz;
                const float a = p.lamL1 / nP, b = p.lamCos / nP;
                gx = a * (dx > 0.f ? 1.0f : (dx < 0.f ? -1.0f : 0.0f)) - b * tx;
                gy = a * (dy > 0.f ? 1.0f : (dy < 0.f ? -1.0f : 0.0f)) - b * ty;
                gz = a * (dz > 0.f ? 1.0f : (dz < 0.f ? -1.0f : 0.0f)) - b * tz;
            }
            const size_t nb4[4] = {k + 1, k - 1, k + (size_t)p.W, k - (size_t)p.W};
#pragma unroll
            for (int d = 0; d < 4; d++) {
                float qx, qy, qz;
                if (nl_load(normals, nb4[d], qx, qy, qz)) {
                    const float w = wS * nl_weight(edge, p.gamma, k, nb4[d]);
                    gx = gx - w * qx;
                    gy = gy - w * qy;
                    gz = gz - w * qz;
                }
            }
            // through n = m / |m|, then through m to A, T, B, S
            const float dot = (g.nx * gx + g.ny * gy) + g.nz * gz;
            const float mx = (gx - g.nx * dot) / g.len, my = (gy - g.ny * dot) / g.len, mz = (gz - g.nz * dot) / g.len;
            const float gA = mx * g.T - mz * (g.T * g.rx);
            const float gT = mx * g.A - mz * (g.A * g.rx + g.S);
            const float gB = my * g.S - mz * (g.S * g.ry);
            const float gS = my * g.B - mz * (g.B * g.ry + g.T);
            const float sx = gS / p.fx, ty2 = gT / p.fy;
            out = make_float4(gA + sx, -gA + sx, gB + ty2, -gB + ty2);
        }
        q[k] = out;
    }
}

__global__ __launch_bounds__(NL_THREADS) void nl_gather_kernel(size_t np, NormalArgs p, const float* __restrict__ depth,
                                                               const float* __restrict__ alpha, const float4* __restrict__ q,
                                                               float* __restrict__ cotDepth, float* __restrict__ cotAlpha)
{
    const size_t stride = (size_t)gridDim.x * NL_THREADS;
    for (size_t k = (size_t)blockIdx.x * NL_THREADS + threadIdx.x; k < np; k += stride) {
        const int j = nl_row(k, p.W), i = (int)(k - (size_t)j * p.W);
        float cd = 0.0f, ca = 0.0f;
        const float D = depth[k], a = alpha[k];
        if (a >= p.alphaMin && a > 0.0f && D > 0.0f) {
            // what the pixel is to its neighbours: the right one of its left neighbour, the left one of its right, ...
            float gz = 0.0f;
            if (i > 0) gz = gz + q[k - 1].x;
            if (i < p.W - 1) gz = gz + q[k + 1].y;
            if (j > 0) gz = gz + q[k - p.W].z;
            if (j < p.H - 1) gz = gz + q[k + p.W].w;
            cd = gz / a;
            ca = -gz * D / (a * a);
        }
        if (p.accumulate) {
            cotDepth[k] = cotDepth[k] + cd;
            cotAlpha[k] = cotAlpha[k] + ca;
        } else {
            cotDepth[k] = cd;
            cotAlpha[k] = ca;
        }
    }
}

long long normal_loss_ws_floats(long long np) { return 3 * ((np + 3) / 4 * 4) + 4 * np; }
long long normal_loss_ws_doubles() { return (long long)NL_PART * NL_MAX_BLOCKS + 2; }

static inline int nl_blocks(size_t np, int cap = NL_MAX_BLOCKS)
{
    const size_t nb = (np + NL_THREADS - 1) / NL_THREADS;
    return (int)(nb < (size_t)cap ? nb : (size_t)cap);
}
// the per-pixel kernels (normals, q, gather) keep no partials: a block per 256 pixels up to 32 blocks a CU, which hides their
// loads' latency where the reduction's 512 blocks (2 a CU) do not
constexpr int NL_STREAM_BLOCKS = 256 * 32;

static inline NormalArgs nl_args(const gs_normal_loss_params& s)
{
    return {s.fx, s.fy, s.cx, s.cy, s.H, s.W, s.lambda_l1, s.lambda_cos, s.lambda_smooth, s.alpha_min, s.max_jump, s.edge_gamma,
            s.accumulate};
}

int launch_depth_normals(gs_ctx* c, const gs_normal_loss_params& s, const float* depth, const float* alpha, float* out)
{
    const size_t np = (size_t)s.H * s.W;
    hipLaunchKernelGGL(normals_kernel, dim3(nl_blocks(np, NL_STREAM_BLOCKS)), dim3(NL_THREADS), 0, c->stream, np, nl_args(s), depth,
                       alpha, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// ws: [7 np] floats (normals, then q, which starts 16-byte aligned: np is rounded up to 4 pixels); partials: normal_loss_ws_doubles()
int launch_normal_loss(gs_ctx* c, const gs_normal_loss_params& s, const float* depth, const float* alpha, const float* target,
                       const unsigned char* mask, const float* edge, float* loss, float* normalOut, float* cotDepth,
                       float* cotAlpha, float* ws, double* partials)
{
    const size_t np = (size_t)s.H * s.W;
    const NormalArgs p = nl_args(s);
    const int nb = nl_blocks(np), ns = nl_blocks(np, NL_STREAM_BLOCKS);
    float* normals = ws;
    float4* q = reinterpret_cast<float4*>(ws + 3 * ((np + 3) / 4 * 4));
    hipLaunchKernelGGL(normals_kernel, dim3(ns), dim3(NL_THREADS), 0, c->stream, np, p, depth, alpha, normals);
    hipLaunchKernelGGL(nl_reduce_kernel, dim3(nb), dim3(NL_THREADS), 0, c->stream, np, p, normals, target, mask, edge, partials);
    hipLaunchKernelGGL(nl_final_kernel, dim3(1), dim3(NL_MAX_BLOCKS), 0, c->stream, nb, p, partials, loss, normalOut);
    hipLaunchKernelGGL(nl_q_kernel, dim3(ns), dim3(NL_THREADS), 0, c->stream, np, p, depth, alpha, normals, target, mask, edge,
                       partials, q);
    hipLaunchKernelGGL(nl_gather_kernel, dim3(ns), dim3(NL_THREADS), 0, c->stream, np, p, depth, alpha, q, cotDepth, cotAlpha);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
