// contrib.hip -- per-Gaussian blend weight scores (include/gsplat.h, gs_blend_contrib / gs_render_contrib).
//
// The blend computes w = T alpha for every (pixel, list entry) and keeps only the sums over the entries; this pass keeps the
// maximum and the sum over the PIXELS, per Gaussian.  Shaped like the op-level forward (blend.hip): a workgroup owns one 16x16
// pixel block, one pixel per lane, four waves; the block's list goes through LDS in chunks of 256 entries, of which only the
// seven floats of the weight and the Gaussian's index are staged (32 B per entry).  A lane carries T alone.
//
// The cost that decides the speed is the reduction of the block's 256 weights to one maximum and one sum per entry.  Entries
// are taken four at a time: a lane runs its pixel through the four (T is sequential), then the wave reduces the four sums and
// the four maxima together in one hand-placed DPP block -- eight independent chains interleaved step by step, so that every
// DPP read is eight instructions behind the write it depends on and no wait states are spent between the steps: 48 DPP
// instructions per four entries and wave, 12 per entry, against the ~20 of the weight itself.  Lane 63 then holds the wave's
// totals and applies at most one integer atomicMax (the bit pattern of a non-negative float orders as the float does: exact,
// order-independent, the same bits on every run) and one float atomicAdd per entry, none where the wave's maximum is 0 -- a
// wave whose pixels have all stopped leaves the chunk, a block whose pixels have all stopped leaves the list.
// The result does not depend on the forward's lastContrib: a pixel's stop is re-derived from its own T, as the forward does.
#include "gs_ctx.h"
#include "gs_blend_geom.h"

namespace gs {

constexpr int CB_NT = 256;       // threads per block = pixels per block = list entries per chunk
constexpr int CB_BATCH = 4;      // entries per wave reduction

// wave64 sums of s0..s3 and maxima of m0..m3 (all eight >= 0); lane 63 holds the totals afterwards
#define GS_CB_STEP(CTRL)                         \
    "v_add_f32_dpp %0, %0, %0 " CTRL "\n\t"      \
    "v_add_f32_dpp %1, %1, %1 " CTRL "\n\t"      \
    "v_add_f32_dpp %2, %2, %2 " CTRL "\n\t"      \
    "v_add_f32_dpp %3, %3, %3 " CTRL "\n\t"      \
    "v_max_f32_dpp %4, %4, %4 " CTRL "\n\t"      \
    "v_max_f32_dpp %5, %5, %5 " CTRL "\n\t"      \
    "v_max_f32_dpp %6, %6, %6 " CTRL "\n\t"      \
    "v_max_f32_dpp %7, %7, %7 " CTRL "\n\t"

__device__ __forceinline__ void wave_sum4_max4(float (&s)[CB_BATCH], float (&m)[CB_BATCH])
{
    asm volatile(
        "s_nop 1\n\t"
        GS_CB_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
        GS_CB_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
        GS_CB_STEP("row_half_mirror row_mask:0xf bank_mask:0xf")
        GS_CB_STEP("row_mirror row_mask:0xf bank_mask:0xf")
        GS_CB_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
        GS_CB_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
        "s_nop 1"
        : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]), "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]));
}
#undef GS_CB_STEP

// maxW / sumW: [N] by Gaussian index, either may be null; both accumulate (max with what is there, add to what is there)
__global__ __launch_bounds__(CB_NT) void blend_contrib_kernel(
    ContribGeom geom, const float4* __restrict__ packed12, const uint32_t* __restrict__ sortedIdx, uint32_t idxMask,
    const uint32_t* __restrict__ tileRanges, int* __restrict__ maxW, float* __restrict__ sumW)
{
    // a: mx my c00 c01 | b: c10 c11 opacity index.  Positions of a chunk behind the list's end hold zero records (weight 0).
    __shared__ float4 sa[CB_NT];
    __shared__ float4 sb[CB_NT];
    const int tid = threadIdx.x, lane = tid & 63;
    const BlockRect br = contrib_rect(geom, (int)blockIdx.x);
    const uint32_t start = tileRanges[2 * br.tile], end = tileRanges[2 * br.tile + 1];
    const uint32_t count = end > start ? end - start : 0u;

    const int x = br.x0 + (tid & 15), y = br.y0 + (tid >> 4);
    bool done = !(x < br.xEnd && y < br.yEnd);        // pixels outside the image (or the tile) do not exist
    const float px = (float)x, py = (float)y;
    float T = 1.0f;

    for (uint32_t chunk = 0; chunk < count; chunk += CB_NT) {
        if (__syncthreads_and(done)) break;           // also fences the previous chunk's LDS reads
        const uint32_t i = chunk + tid;
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
        __syncthreads();
        const uint32_t m = min((uint32_t)CB_NT, count - chunk);
        for (uint32_t j = 0; j < m; j += CB_BATCH) {  // (m rounded up to the batch stays inside the chunk's 256 slots)
            if (__all(done)) break;                   // wave-uniform: nothing of this wave blends the rest of the chunk
            float s[CB_BATCH], mx[CB_BATCH];
#pragma unroll
            for (int k = 0; k < CB_BATCH; k++) {
                const float4 ea = sa[j + k], eb = sb[j + k];
                float w = 0.0f;
                if (!done) {
                    const float alpha = splat_alpha<true>(px, py, ea, eb, eb.z).alpha;
                    w = T * alpha;
                    T = T * (1.0f - alpha);
                    if (T < 1e-4f) done = true;
                }
                s[k] = w; mx[k] = w;
            }
            wave_sum4_max4(s, mx);
            if (lane == 63) {
#pragma unroll
                for (int k = 0; k < CB_BATCH; k++) {
                    if (mx[k] > 0.0f) {
                        const uint32_t g = __float_as_uint(sb[j + k].w);
                        if (maxW) atomicMax(&maxW[g], __float_as_int(mx[k]));
                        if (sumW) atomicAdd(&sumW[g], s[k]);
                    }
                }
            }
        }
    }
}

// the prune decision on a score, in the words of gs_classify_gaussians: action 3 / count 0 below the threshold, else 0 / 1
__global__ void contrib_actions_kernel(int N, const float* __restrict__ score, float threshold, int* __restrict__ actions,
                                       int* __restrict__ outputCounts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const bool prune = score[i] < threshold;
    actions[i] = prune ? 3 : 0;
    outputCounts[i] = prune ? 0 : 1;
}

// over the lists of the context's last binning, in the geometry the context describes at the time of the call (the caller's
// tile grid for the op-level form; the fused path's own -- block lists included -- behind a fused forward)
int launch_blend_contrib(gs_ctx* c, float* maxW, float* sumW)
{
    ContribGeom cg;
    const int nBlocks = contrib_geom(c, cg);
    if (nBlocks <= 0 || c->binN <= 0) return GS_OK;
    const uint32_t* idx = c->sortedPlainValid ? c->sortedIdx : c->sortedRaw;
    const uint32_t mask = c->sortedPlainValid ? 0xFFFFFFFFu : c->idxMask;
    hipLaunchKernelGGL(blend_contrib_kernel, dim3(nBlocks), dim3(CB_NT), 0, c->stream, cg,
                       reinterpret_cast<const float4*>(c->packed12), idx, mask, c->tileRanges, reinterpret_cast<int*>(maxW), sumW);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_contrib_actions(gs_ctx* c, int N, const float* score, float threshold, int* actions, int* outputCounts)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(contrib_actions_kernel, dim3(gs_div_up(N, 256)), dim3(256), 0, c->stream, N, score, threshold, actions,
                       outputCounts);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
