// features.hip -- N-channel per-Gaussian feature rendering and its backward with respect to the features (include/gsplat.h,
// gs_blend_features / gs_render_features and their _backward).
//
// Both directions are the product of the (pixels x entries) matrix of blend weights w(p, g) = T alpha with a C-wide matrix:
//   forward   out[p, c]     = sum over the entries g of p's list of  w(p, g) f[g, c]
//   backward  grad_f[g, c] += sum over the pixels p               of  w(p, g) cot[p, c]
// over the lists and records of the last binning / the last fused forward, with contrib.hip's weight rule to the bit
// (splat_alpha<true>, clamp 0.99, a pixel stops after the entry that brings T below 1e-4, no 1/255 skip, no background), so
// that weights, stops and lists agree with the forward, with gs_blend_contrib and with contrib_prune.blend_weights.
//
// Shape, both kernels: a workgroup owns one 16x16 pixel block (contrib_rect: image grid, per tile, or the fused path's block
// lists) and one GROUP of G = GS_FEATURE_GROUP channels (blockIdx.y); one pixel per lane, four waves; the block's list goes
// through LDS in chunks of 256 entries (32 B of record per entry, as contrib.hip).  A lane carries T alone besides the payload.
// The list is swept again for every group: the weight (~22 VALU instructions) is paid once per G channels.
//
// Forward: the chunk's feature rows of the group are staged next to the records (256 x G floats), read back as wave-uniform
// ds_read_b128 broadcasts; a lane keeps G accumulators and spends one v_fma per channel and entry.  A pixel's sum runs in list
// order on its own lane: no atomics, the same bits on every run.  Every pixel of the block's rectangle is written, zeros included.
//
// Backward: the reduction over the block's pixels is what costs -- with the DPP reduction of contrib.hip it is six DPP steps per
// channel and entry.  Here the matrix core does it: per wave and batch of 16 entries the lanes write their 16 weights to a
// wave-private LDS tile [entry][pixel], read them back as the A operand of v_mfma_f32_16x16x4_f32 (lane l: entry l & 15, pixels
// 16 (l >> 4) + m for m = 0 .. 15: four ds_read_b128), and sixteen MFMAs against the cotangent tile the lane holds in registers
// since the group began (B operand, lane l: pixel 16 (l >> 4) + m, channel l & 15) leave D[entry 4 (l >> 4) + r][channel l & 15]:
// the wave's sums over its 64 pixels, exact f32 (the f32 MFMA is a chain of fmaf).  One float atomicAdd per wave, entry and
// channel, none where the sum is 0 -- which it is, exactly, where the wave's weights are all 0: rows of Gaussians in no list or
// behind every pixel's stop are never touched.  (cot must be finite: 0 x inf would not be 0.)  A wave whose pixels have all
// stopped leaves the chunk, a block whose pixels have all stopped leaves the list.
#include "gs_ctx.h"
#include "gs_blend_geom.h"

#ifndef GS_FEATURE_GROUP
#define GS_FEATURE_GROUP 16
#endif

namespace gs {

constexpr int FT_NT = 256;                        // threads per block = pixels per block = list entries per chunk
constexpr int FT_G = GS_FEATURE_GROUP;            // channels per sweep of the list
constexpr int FT_BATCH = 16;                      // entries per MFMA batch of the backward (the M of 16x16x4)
constexpr int FT_NTILES = (FT_G + 15) / 16;       // 16-channel column tiles of the backward per group
constexpr int FT_WSTRIDE = 68;                    // floats per entry row of the wave's weight tile: 64 pixels + 4 (b128 reads of 16
                                                  // rows then cover all 64 banks once)
static_assert(FT_G >= 4 && (FT_G & (FT_G - 1)) == 0 && FT_G <= 64, "GS_FEATURE_GROUP: a power of two in [4, 64]");

typedef float ft_f32x4 __attribute__((ext_vector_type(4)));

// stage the records of the chunk's entry `i` (a: mx my c00 c01 | b: c10 c11 opacity index); positions behind the list's end
// hold zero records (weight 0)
__device__ __forceinline__ void ft_stage_records(float4* sa, float4* sb, int tid, uint32_t i, uint32_t count, uint32_t start,
                                                 const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx,
                                                 uint32_t idxMask)
{
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (i < count) {
        const uint32_t g = sortedIdx[start + i] & idxMask;
        const float4* src = packed12 + (size_t)g * 3;
        a = src[0];
        const float4 b0 = src[1];
        b = make_float4(b0.x, b0.y, reinterpret_cast<const float*>(src + 2)[1], __uint_as_float(g));
    }
    sa[tid] = a;
    sb[tid] = b;
}

// one entry against one pixel: the weight (0 for a pixel that has stopped), T and the stop carried along -- contrib.hip's rule
__device__ __forceinline__ float ft_weight(float px, float py, const float4& ea, const float4& eb, float& T, bool& done)
{
    float w = 0.0f;
    if (!done) {
        const float alpha = splat_alpha<true>(px, py, ea, eb, eb.z).alpha;
        w = T * alpha;
        T = T * (1.0f - alpha);
        if (T < 1e-4f) done = true;
    }
    return w;
}

// out [H, W, C]: channels [c0, c0 + G) of every pixel of the block's rectangle are written
__global__ __launch_bounds__(FT_NT) void blend_features_kernel(
    ContribGeom geom, const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx, uint32_t idxMask,
    const uint32_t* __restrict__ tileRanges, int C, const float* __restrict__ features, float* __restrict__ out)
{
    __shared__ float4 sa[FT_NT];
    __shared__ float4 sb[FT_NT];
    __shared__ float4 sf[FT_NT * FT_G / 4];           // the group's channels of the chunk's feature rows, zero behind channel C
    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.y * FT_G, gc = min(FT_G, C - c0);
    const BlockRect br = contrib_rect(geom, (int)blockIdx.x);
    const uint32_t start = tileRanges[2 * br.tile], end = tileRanges[2 * br.tile + 1];
    const uint32_t count = end > start ? end - start : 0u;

    const int x = br.x0 + (tid & 15), y = br.y0 + (tid >> 4);
    const bool exists = x < br.xEnd && y < br.yEnd;   // pixels outside the image (or the tile) do not exist
    bool done = !exists;
    const float px = (float)x, py = (float)y;
    float T = 1.0f;
    float acc[FT_G];
#pragma unroll
    for (int k = 0; k < FT_G; k++) acc[k] = 0.0f;

    for (uint32_t chunk = 0; chunk < count; chunk += FT_NT) {
        if (__syncthreads_and(done)) break;           // also fences the previous chunk's LDS reads
        ft_stage_records(sa, sb, tid, chunk + tid, count, start, packed12, sortedIdx, idxMask);
        __syncthreads();
        const uint32_t m = min((uint32_t)FT_NT, count - chunk);
        float* sfl = reinterpret_cast<float*>(sf);
        for (uint32_t t = tid; t < m * FT_G; t += FT_NT) {        // consecutive lanes: consecutive channels of a row
            const uint32_t e = t / FT_G;
            const int k = (int)(t % FT_G);
            const uint32_t g = __float_as_uint(sb[e].w);
            sfl[t] = k < gc ? features[(size_t)g * (size_t)C + (size_t)(c0 + k)] : 0.0f;
        }
        __syncthreads();
        for (uint32_t j = 0; j < m; j++) {
            if (__all(done)) break;                   // wave-uniform: nothing of this wave blends the rest of the chunk
            const float w = ft_weight(px, py, sa[j], sb[j], T, done);
#pragma unroll
            for (int q = 0; q < FT_G / 4; q++) {
                const float4 f = sf[j * (FT_G / 4) + q];
                acc[4 * q + 0] = fmaf(w, f.x, acc[4 * q + 0]);
                acc[4 * q + 1] = fmaf(w, f.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(w, f.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(w, f.w, acc[4 * q + 3]);
            }
        }
    }
    if (exists) {
        float* o = out + ((size_t)y * (size_t)geom.g.W + (size_t)x) * (size_t)C + (size_t)c0;
#pragma unroll
        for (int k = 0; k < FT_G; k++)
            if (k < gc) o[k] = acc[k];
    }
}

// cot [H, W, C]; grad [N, C] accumulates (float atomics), channels [c0, c0 + G) of the rows whose Gaussians weigh on the block
__global__ __launch_bounds__(FT_NT) void blend_features_backward_kernel(
    ContribGeom geom, const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx, uint32_t idxMask,
    const uint32_t* __restrict__ tileRanges, int C, const float* __restrict__ cot, float* __restrict__ grad)
{
    __shared__ float4 sa[FT_NT];
    __shared__ float4 sb[FT_NT];
    __shared__ float4 swt[4][FT_BATCH * FT_WSTRIDE / 4];          // per wave: weights [entry of the batch][pixel of the wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.y * FT_G, cEnd = min(C, c0 + FT_G);
    const BlockRect br = contrib_rect(geom, (int)blockIdx.x);
    const uint32_t start = tileRanges[2 * br.tile], end = tileRanges[2 * br.tile + 1];
    const uint32_t count = end > start ? end - start : 0u;
    if (count == 0) return;

    const int x = br.x0 + (tid & 15), y = br.y0 + (tid >> 4);
    bool done = !(x < br.xEnd && y < br.yEnd);
    const float px = (float)x, py = (float)y;
    float T = 1.0f;

    // B operand: the cotangents of pixel 16 (lane >> 4) + m of this wave -- column m of block row 4 wave + (lane >> 4) -- in
    // channel c0 + 16 t + (lane & 15); 0 outside the rectangle and behind the group's (or the image's) last channel
    const int lcol = lane & 15, lrow = lane >> 4;
    float cb[FT_NTILES][16];
    {
        const int yy = br.y0 + 4 * wave + lrow;
#pragma unroll
        for (int t = 0; t < FT_NTILES; t++) {
            const int c = c0 + 16 * t + lcol;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                const int xx = br.x0 + m;
                float v = 0.0f;
                if (xx < br.xEnd && yy < br.yEnd && c < cEnd)
                    v = cot[((size_t)yy * (size_t)geom.g.W + (size_t)xx) * (size_t)C + (size_t)c];
                cb[t][m] = v;
            }
        }
    }
    float* wt = reinterpret_cast<float*>(swt[wave]);

    for (uint32_t chunk = 0; chunk < count; chunk += FT_NT) {
        if (__syncthreads_and(done)) break;           // also fences the previous chunk's LDS reads
        ft_stage_records(sa, sb, tid, chunk + tid, count, start, packed12, sortedIdx, idxMask);
        __syncthreads();
        const uint32_t m = min((uint32_t)FT_NT, count - chunk);
        for (uint32_t j = 0; j < m; j += FT_BATCH) {  // (m rounded up to the batch stays inside the chunk's 256 slots)
            if (__all(done)) break;                   // wave-uniform: nothing of this wave blends the rest of the chunk
#pragma unroll
            for (int k = 0; k < FT_BATCH; k++)
                wt[k * FT_WSTRIDE + lane] = ft_weight(px, py, sa[j + k], sb[j + k], T, done);
            // the tile is this wave's own: its LDS instructions execute in order, the fence keeps the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float a[16];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 v = *reinterpret_cast<const float4*>(wt + lcol * FT_WSTRIDE + 16 * lrow + 4 * q);
                a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t gIdx[4];
#pragma unroll
            for (int r = 0; r < 4; r++) gIdx[r] = __float_as_uint(sb[j + 4 * lrow + r].w);
#pragma unroll
            for (int t = 0; t < FT_NTILES; t++) {
                // two chains: the instruction issues every 32 cycles but a dependent one waits 40
                ft_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int mm = 0; mm < 16; mm += 2) {
                    d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mm], cb[t][mm], d0, 0, 0, 0);
                    d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mm + 1], cb[t][mm + 1], d1, 0, 0, 0);
                }
                const int c = c0 + 16 * t + lcol;
                if (c < cEnd) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float d = d0[r] + d1[r];
                        if (d != 0.0f) atomicAdd(grad + (size_t)gIdx[r] * (size_t)C + (size_t)c, d);
                    }
                }
            }
        }
    }
}

static int ft_lists(gs_ctx* c, ContribGeom& cg, const uint32_t*& idx, uint32_t& mask)
{
    const int nBlocks = contrib_geom(c, cg);
    idx = c->sortedPlainValid ? c->sortedIdx : c->sortedRaw;
    mask = c->sortedPlainValid ? 0xFFFFFFFFu : c->idxMask;
    return c->binN <= 0 ? 0 : nBlocks;
}

// over the lists of the context's last binning, in the geometry the context describes at the time of the call (launch_blend_contrib)
int launch_blend_features(gs_ctx* c, int C, const float* features, float* out)
{
    if ((long long)c->W * c->H <= 0) return GS_OK;
    ContribGeom cg;
    const uint32_t* idx; uint32_t mask;
    const int nBlocks = ft_lists(c, cg, idx, mask);
    if (nBlocks <= 0) {           // no Gaussians: no lists to sweep, and the image is still the caller's to read
        GS_HIP_CHECK(c, hipMemsetAsync(out, 0, (size_t)c->W * (size_t)c->H * (size_t)C * sizeof(float), c->stream));
        return GS_OK;
    }
    hipLaunchKernelGGL(blend_features_kernel, dim3(nBlocks, gs_div_up(C, FT_G)), dim3(FT_NT), 0, c->stream, cg,
                       reinterpret_cast<const float4*>(c->packed12), idx, mask, c->tileRanges, C, features, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_blend_features_backward(gs_ctx* c, int C, const float* cot, float* grad)
{
    ContribGeom cg;
    const uint32_t* idx; uint32_t mask;
    const int nBlocks = ft_lists(c, cg, idx, mask);
    if (nBlocks <= 0) return GS_OK;
    hipLaunchKernelGGL(blend_features_backward_kernel, dim3(nBlocks, gs_div_up(C, FT_G)), dim3(FT_NT), 0, c->stream, cg,
                       reinterpret_cast<const float4*>(c->packed12), idx, mask, c->tileRanges, C, cot, grad);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int feature_channel_group() { return FT_G; }

}  // namespace gs
