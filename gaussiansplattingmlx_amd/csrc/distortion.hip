// distortion.hip -- the depth distortion loss (2DGS eq. 13, gsplat's distloss) as two sweeps over the lists and records of the
// last binning / the last fused forward, and the term's loss kernel (include/gsplat.h, gs_blend_distortion / gs_render_distortion
// and their _backward, gs_distortion_loss; distortion.py restates all of it in numpy).
//
// Per pixel, over the entries i of its list up to its stop, with contrib.hip's weight rule to the bit (splat_alpha<true>, clamp
// 0.99, a pixel stops after the entry that brings T below 1e-4, no 1/255 skip, no background) and m_i = map(z_i):
//   D = sum_{i<j} w_i w_j (m_i - m_j)^2 = A S,    A = sum w_i,  mu = sum w_i m_i / A,  S = sum w_i (m_i - mu)^2
// (A, mu, S) are carried with the weighted Welford update
//   A' = A + w,  mu' = mu + (w / A') (m - mu),  S' = S + w (m - mu) (m - mu')
// which cancels nothing where the loss does its work, on thin distributions; A M2 - M1^2 and 2DGS's running prefix form lose every
// digit there in float32.  The update runs on m - c, c the m of the pixel's first weighted entry (the variance does not see the
// shift; the reported mean is c + mu): on a distribution of relative width 1e-4 the running mean of m itself is rounded to an
// ulp of m, 1e-3 of the deviations it is subtracted from, and D comes out with three digits; shifted, with all but a few ulps.
// With the pixel's totals the derivatives are closed:
//   g_i = dD/dw_i = A (m_i - mu)^2 + S,   dD/dm_i = 2 w_i A (m_i - mu),   dD/dalpha_i = T_i g_i - R_i / (1 - alpha_i),
//   R_i = sum_{j>i} g_j w_j = 2 D - sum_{j<=i} g_j w_j          (sum_j g_j w_j = 2 D)
//
// Shape, both sweeps (as features.hip): a workgroup owns one 16x16 pixel block (contrib_rect: image grid, per tile, or the fused
// path's block lists), one pixel per lane, four waves; the block's list goes through LDS in chunks of 256 entries -- the 32 B of
// record the weight needs and (m, map'(z)), computed once by the staging lane: 40 B per entry, 10 KB per block.
//
// Forward: a register sweep carrying (T, A, mu, S); D [H, W] and the totals [H, W, 3] of every pixel of the block's rectangle are
// written, zeros included.  No atomics: the same bits on every run.
//
// Backward: a second front-to-back sweep with the same T (so weights and stops are the forward's to the bit), the prefix of
// g_j w_j beside it and R_i as total minus prefix -- the rounding of that difference is 2^-24 of 2 D, far inside what the float
// atomics leave.  Per (pixel, entry) seven values (dmx dmy dc00 dc01 dc11 dop ddepth) from dD/dalpha by blend.hip's bwd_step
// (the clamp passes the gradient iff raw <= 0.99, the floor of 1 - alpha is 1e-6) and from dD/dm through map'(z).  They are no
// weight-times-payload product, so features.hip's matrix-core reduction does not apply: the wave's 64 pixels are summed by the blend
// backward's transposed DPP reduction (gs_wavesum.h, the three colour inputs zero), and the eight lanes that hold a column's
// total issue one float atomicAdd each per wave and entry into the 16-float row, none where the sum is exactly 0.  A pixel whose
// cotangent is 0 (a masked pixel) is done from the start; a wave whose pixels have all stopped leaves the chunk, a block whose
// pixels have all stopped leaves the list; rows of Gaussians in no list or behind every stop are never touched.
#include "gs_ctx.h"
#include "gs_blend_geom.h"
#include "gs_wavesum.h"

namespace gs {

constexpr int DS_NT = 256;             // threads per block = pixels per block = list entries per chunk
constexpr int DSL_THREADS = 256;       // the loss kernel
constexpr int DSL_MAX_BLOCKS = 512;    // ... and the capacity of its partials (gs_ctx::distortionWs)

// m = scale (1 - near / z) (GS_DISTORTION_NDC, scale = far / (far - near)) or m = z
struct DistMap {
    int map;
    float scale, near;
};

static inline DistMap dist_map(const gs_distortion_params& p)
{
    DistMap d = {p.map, 1.0f, 0.0f};
    if (p.map == GS_DISTORTION_NDC) { d.scale = p.far / (p.far - p.near); d.near = p.near; }
    return d;
}

// stage the chunk's entry `i`: (a: mx my c00 c01 | b: c10 c11 opacity index | m: map(z), map'(z)); positions behind the list's end
// hold zero records (weight 0), which the sweeps do not reach
__device__ __forceinline__ void ds_stage(float4* sa, float4* sb, float2* sm, int tid, uint32_t i, uint32_t count, uint32_t start,
                                         const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx,
                                         uint32_t idxMask, const DistMap& dm)
{
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    float2 m = make_float2(0.f, 0.f);
    if (i < count) {
        const uint32_t g = sortedIdx[start + i] & idxMask;
        const float4* src = packed12 + (size_t)g * 3;
        a = src[0];
        const float4 b0 = src[1];
        const float4 c0 = src[2];      // b opacity depth pad
        b = make_float4(b0.x, b0.y, c0.y, __uint_as_float(g));
        const float z = c0.z;
        if (dm.map == GS_DISTORTION_NDC) {
            m.x = dm.scale * (1.0f - dm.near / z);
            m.y = dm.scale * dm.near / (z * z);
        } else {
            m.x = z;
            m.y = 1.0f;
        }
    }
    sa[tid] = a;
    sb[tid] = b;
    sm[tid] = m;
}

// outDistort [H, W], outTotals [H, W, 3]: every pixel of the block's rectangle is written
__global__ __launch_bounds__(DS_NT) void blend_distortion_kernel(
    ContribGeom geom, const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx, uint32_t idxMask,
    const uint32_t* __restrict__ tileRanges, DistMap dm, float* __restrict__ outDistort, float* __restrict__ outTotals)
{
    __shared__ float4 sa[DS_NT];
    __shared__ float4 sb[DS_NT];
    __shared__ float2 sm[DS_NT];
    const int tid = threadIdx.x;
    const BlockRect br = contrib_rect(geom, (int)blockIdx.x);
    const uint32_t start = tileRanges[2 * br.tile], end = tileRanges[2 * br.tile + 1];
    const uint32_t count = end > start ? end - start : 0u;

    const int x = br.x0 + (tid & 15), y = br.y0 + (tid >> 4);
    const bool exists = x < br.xEnd && y < br.yEnd;   // pixels outside the image (or the tile) do not exist
    bool done = !exists;
    const float px = (float)x, py = (float)y;
    float T = 1.0f, A = 0.0f, mu = 0.0f, S = 0.0f, c = 0.0f;    // mu: of m - c

    for (uint32_t chunk = 0; chunk < count; chunk += DS_NT) {
        if (__syncthreads_and(done)) break;           // also fences the previous chunk's LDS reads
        ds_stage(sa, sb, sm, tid, chunk + tid, count, start, packed12, sortedIdx, idxMask, dm);
        __syncthreads();
        const uint32_t n = min((uint32_t)DS_NT, count - chunk);
        for (uint32_t j = 0; j < n; j++) {
            if (__all(done)) break;                   // wave-uniform: nothing of this wave blends the rest of the chunk
            if (!done) {
                const float4 ea = sa[j], eb = sb[j];
                const float alpha = splat_alpha<true>(px, py, ea, eb, eb.z).alpha;
                const float w = T * alpha;
                if (w > 0.0f) {                       // (w = 0 changes nothing, and A' could still be 0)
                    const float m = sm[j].x;
                    if (A == 0.0f) c = m;             // the pixel's first weighted entry: the origin of the rest
                    const float e = m - c;            // exact where m is within a factor 2 of c
                    const float An = A + w;
                    const float d = e - mu;
                    const float mun = mu + (w / An) * d;
                    S = S + (w * d) * (e - mun);
                    A = An;
                    mu = mun;
                }
                T = T * (1.0f - alpha);
                if (T < 1e-4f) done = true;
            }
        }
    }
    if (exists) {
        const size_t pix = (size_t)y * (size_t)geom.g.W + (size_t)x;
        outDistort[pix] = A * S;
        float* t = outTotals + pix * 3;
        t[0] = A; t[1] = c + mu; t[2] = S;
    }
}

// cot [H, W], totals [H, W, 3]; rows16 [N, 16] accumulates (float atomics) in gradAcc16's column order: columns 0 .. 5, 9 and 10
// of the rows whose Gaussians weigh on the block
__global__ __launch_bounds__(DS_NT) void blend_distortion_backward_kernel(
    ContribGeom geom, const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx, uint32_t idxMask,
    const uint32_t* __restrict__ tileRanges, DistMap dm, const float* __restrict__ cot, const float* __restrict__ totals,
    float* __restrict__ rows16)
{
    __shared__ float4 sa[DS_NT];
    __shared__ float4 sb[DS_NT];
    __shared__ float2 sm[DS_NT];
    const int tid = threadIdx.x, lane = tid & 63;
    const BlockRect br = contrib_rect(geom, (int)blockIdx.x);
    const uint32_t start = tileRanges[2 * br.tile], end = tileRanges[2 * br.tile + 1];
    const uint32_t count = end > start ? end - start : 0u;
    if (count == 0) return;

    const int x = br.x0 + (tid & 15), y = br.y0 + (tid >> 4);
    const float px = (float)x, py = (float)y;
    float cp = 0.0f, A = 0.0f, mu = 0.0f, S = 0.0f;
    if (x < br.xEnd && y < br.yEnd) {
        const size_t pix = (size_t)y * (size_t)geom.g.W + (size_t)x;
        cp = cot[pix];
        const float* t = totals + pix * 3;
        A = t[0]; mu = t[1]; S = t[2];
    }
    bool done = cp == 0.0f;                           // no pixel, or one the loss does not see: every value it adds is 0
    const float twoD = 2.0f * (A * S);
    float T = 1.0f, P = 0.0f;

    // where wave_sum10_transposed leaves the totals (gs_wavesum.h): every lane of quad q of row r holds
    //   r = 0: dmx dc00 dmy dc01   r = 1: dop dop ddepth ddepth   r = 2: dc11 . . .
    // one lane per packed column (dc10 is dc01 again, taken by the quad's second lane)
    int col = -1;
    switch (lane) {
    case 0: col = 0; break;
    case 4: col = 2; break;
    case 8: col = 1; break;
    case 12: col = 3; break;
    case 13: col = 4; break;
    case 16: col = 9; break;
    case 24: col = 10; break;
    case 32: col = 5; break;
    default: break;
    }

    for (uint32_t chunk = 0; chunk < count; chunk += DS_NT) {
        if (__syncthreads_and(done)) break;           // also fences the previous chunk's LDS reads
        ds_stage(sa, sb, sm, tid, chunk + tid, count, start, packed12, sortedIdx, idxMask, dm);
        __syncthreads();
        const uint32_t n = min((uint32_t)DS_NT, count - chunk);
        for (uint32_t j = 0; j < n; j++) {
            if (__all(done)) break;                   // wave-uniform: nothing of this wave blends the rest of the chunk
            const float4 ea = sa[j], eb = sb[j];
            // dmx dmy dc00 dc01 dc11 (dr dg db) dop ddepth
            float u[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (!done) {
                const SplatAlpha s = splat_alpha<true>(px, py, ea, eb, eb.z);
                const float alpha = s.alpha;
                const float w = T * alpha;
                const float2 mz = sm[j];
                const float d = mz.x - mu;
                const float Ad = A * d;
                const float g = Ad * d + S;
                P = P + g * w;
                const float R = twoD - P;
                float denom = 1.0f - alpha;
                if (denom < 1e-6f) denom = 1e-6f;
                const float dAlpha = cp * (T * g - R * __builtin_amdgcn_rcpf(denom));
                // reverse of the alpha (blend.hip bwd_step): the clamp passes iff raw <= 0.99
                const float S32 = s.raw > 0.99f ? 0.0f : dAlpha;
                const float exS = s.ex * S32;
                const float S36 = -0.5f * (eb.z * exS);
                const float S39 = s.dy * (eb.y * S36);
                const float S41 = s.dx * (ea.z * S36);
                const float S42 = eb.x * S36 + ea.w * S36;
                u[0] = -(S41 + S41 + s.dy * S42);
                u[1] = -(S39 + S39 + s.dx * S42);
                u[2] = s.dx * s.dx * S36;
                u[3] = s.dxdy * S36;
                u[4] = s.dy * s.dy * S36;
                u[8] = exS;
                u[9] = cp * ((2.0f * w) * Ad) * mz.y;
                T = T * (1.0f - alpha);
                if (T < 1e-4f) done = true;
            }
            const float tot = wave_sum10_transposed<false>(u);
            if (col >= 0 && tot != 0.0f) atomicAdd(rows16 + (size_t)__float_as_uint(eb.w) * 16 + (size_t)col, tot);
        }
    }
}

// per-block partial sums of v D (double; written, not added: nothing to clear beforehand) and the cotangent image weight v / n
__global__ __launch_bounds__(DSL_THREADS) void distortion_loss_kernel(size_t np, float weight, float nPixels,
                                                                      const float* __restrict__ distort,
                                                                      const unsigned char* __restrict__ mask,
                                                                      double* __restrict__ partials, float* __restrict__ cotOut)
{
    __shared__ double smSum[DSL_THREADS / 64];
    double sum = 0.0;
    const size_t stride = (size_t)gridDim.x * DSL_THREADS;
    for (size_t i = (size_t)blockIdx.x * DSL_THREADS + threadIdx.x; i < np; i += stride) {
        const float v = mask ? (float)mask[i] / 255.0f : 1.0f;
        sum += (double)(v * distort[i]);
        cotOut[i] = weight * v / nPixels;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if ((threadIdx.x & 63) == 0) smSum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < DSL_THREADS / 64; w++) s += smSum[w];
        partials[blockIdx.x] = s;
    }
}

// one workgroup: the partials in a fixed order; lossOut[0] += weight sum / n
__global__ __launch_bounds__(DSL_MAX_BLOCKS) void distortion_loss_final_kernel(int nb, float weight, float nPixels,
                                                                              const double* __restrict__ partials,
                                                                              float* __restrict__ lossOut)
{
    __shared__ double sm[DSL_MAX_BLOCKS / 64];
    double s = (int)threadIdx.x < nb ? partials[threadIdx.x] : 0.0;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        for (int w = 0; w < DSL_MAX_BLOCKS / 64; w++) s += sm[w];
        lossOut[0] = (float)((double)lossOut[0] + (double)weight * s / (double)nPixels);
    }
}

static int ds_lists(gs_ctx* c, ContribGeom& cg, const uint32_t*& idx, uint32_t& mask)
{
    const int nBlocks = contrib_geom(c, cg);
    idx = c->sortedPlainValid ? c->sortedIdx : c->sortedRaw;
    mask = c->sortedPlainValid ? 0xFFFFFFFFu : c->idxMask;
    return c->binN <= 0 ? 0 : nBlocks;
}

// over the lists of the context's last binning, in the geometry the context describes at the time of the call (launch_blend_contrib)
int launch_blend_distortion(gs_ctx* c, const gs_distortion_params& p, float* outDistort, float* outTotals)
{
    const size_t np = (size_t)c->W * (size_t)c->H;
    if (np == 0) return GS_OK;
    ContribGeom cg;
    const uint32_t* idx; uint32_t mask;
    const int nBlocks = ds_lists(c, cg, idx, mask);
    if (nBlocks <= 0) {           // no Gaussians: no lists to sweep, and the images are still the caller's to read
        GS_HIP_CHECK(c, hipMemsetAsync(outDistort, 0, np * sizeof(float), c->stream));
        GS_HIP_CHECK(c, hipMemsetAsync(outTotals, 0, np * 3 * sizeof(float), c->stream));
        return GS_OK;
    }
    hipLaunchKernelGGL(blend_distortion_kernel, dim3(nBlocks), dim3(DS_NT), 0, c->stream, cg,
                       reinterpret_cast<const float4*>(c->packed12), idx, mask, c->tileRanges, dist_map(p), outDistort, outTotals);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_blend_distortion_backward(gs_ctx* c, const gs_distortion_params& p, const float* cot, const float* totals, float* rows16)
{
    ContribGeom cg;
    const uint32_t* idx; uint32_t mask;
    const int nBlocks = ds_lists(c, cg, idx, mask);
    if (nBlocks <= 0) return GS_OK;
    hipLaunchKernelGGL(blend_distortion_backward_kernel, dim3(nBlocks), dim3(DS_NT), 0, c->stream, cg,
                       reinterpret_cast<const float4*>(c->packed12), idx, mask, c->tileRanges, dist_map(p), cot, totals, rows16);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

long long distortion_loss_ws_doubles() { return DSL_MAX_BLOCKS; }

int launch_distortion_loss(gs_ctx* c, float weight, long long n, const float* distort, const unsigned char* mask, float* loss,
                           float* cotOut)
{
    if (n <= 0) return GS_OK;
    const size_t np = (size_t)n;
    const size_t want = (np + DSL_THREADS - 1) / DSL_THREADS;
    const int nb = (int)(want < (size_t)DSL_MAX_BLOCKS ? want : (size_t)DSL_MAX_BLOCKS);
    hipLaunchKernelGGL(distortion_loss_kernel, dim3(nb), dim3(DSL_THREADS), 0, c->stream, np, weight, (float)n, distort, mask,
                       c->distortionWs, cotOut);
    hipLaunchKernelGGL(distortion_loss_final_kernel, dim3(1), dim3(DSL_MAX_BLOCKS), 0, c->stream, nb, weight, (float)n,
                       c->distortionWs, loss);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
