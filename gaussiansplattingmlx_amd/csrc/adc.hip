// adc.hip -- adaptive density control (Kerbl et al. 2023, gsplat's DefaultStrategy): the strategy beside
// densify.hip's (Trainer/GaussianTrainer.swift:343-393 classify, :858-893 gather, which it replaces under strategy="adc").
//
// Streaming passes over N or over the output rows, as densify.hip's are: 256 threads, one row per thread, float4 where a row's
// length and alignment allow.  The scan, the plan and the output map between classify and gather are densify.hip's, unchanged.
#include <math.h>

#include "gs_ctx.h"

namespace gs {

constexpr int ADC_THREADS = 256;

// The step's statistic, behind the blend backward (api.hip blend_backward_of_forward) or on the caller's rows (gs_adc_accumulate):
// for every Gaussian the forward gave a radius > 0
//   gradSum += hypot(W/2 gx, H/2 gy),  count += 1,  maxRadius = max(maxRadius, radius)
// (gx, gy) = columns col, col + 1 of the Gaussian's gradAcc16 row: 0 the signed 2-D mean gradient, 12 the absolute sums of an
// absgrad backward.  A Gaussian of radius 0 (or NaN) keeps the bits of all three words.  gate: as absgrad_accum_kernel's.
__global__ __launch_bounds__(ADC_THREADS) void adc_accum_kernel(int N, const float* __restrict__ rows16, const float* __restrict__ radii,
                                                                int col, float halfW, float halfH, const uint32_t* __restrict__ gate,
                                                                float* gradSum, float* count, float* maxRadius)
{
    const int i = blockIdx.x * ADC_THREADS + threadIdx.x;
    if (i >= N) return;
    if (gate && *gate) return;
    const float r = radii[i];
    if (!(r > 0.0f)) return;
    const float2 a = *reinterpret_cast<const float2*>(rows16 + (size_t)i * 16 + col);
    gradSum[i] += hypotf(halfW * a.x, halfH * a.y);      // (not sqrtf(x x + y y): sums below 1e-19 would square to zero)
    count[i] += 1.0f;                                    // (exact up to 2^24 visits)
    maxRadius[i] = fmaxf(maxRadius[i], r);
}

// The decision, in classify_kernel's words (0 keep, 1 split, 2 clone, 3 prune; output counts 1 / 2 / 2 / 0), in this order:
//   1. sigmoid(opacity) < minOpacity                                              prune
//   2. allowDensify and gradSum / count >= gradThreshold                          clone if max exp(scale) <= denseMax, else split
//   3. sizePrune and (maxRadius > maxScreenSize or max exp(scale) > worldMax)     prune
//   4.                                                                            keep
// count == 0: the average is 0.  maxScreenSize <= 0: no screen test.
__global__ __launch_bounds__(ADC_THREADS) void adc_classify_kernel(int N, const float* __restrict__ gradSum,
                                                                   const float* __restrict__ count,
                                                                   const float* __restrict__ maxRadius,
                                                                   const float* __restrict__ scales, int scaleStride,
                                                                   const float* __restrict__ opacity, float gradThreshold,
                                                                   float denseMax, float minOpacity, float maxScreenSize,
                                                                   float worldMax, int allowDensify, int sizePrune,
                                                                   int* __restrict__ actions, int* __restrict__ outputCounts)
{
    const int i = blockIdx.x * ADC_THREADS + threadIdx.x;
    if (i >= N) return;
    const float n = count[i];
    const float avg = n > 0.0f ? gradSum[i] / n : 0.0f;
    const float* s = scales + (size_t)i * scaleStride;
    const float smax = fmaxf(fmaxf(expf(s[0]), expf(s[1])), expf(s[2]));
    const float op = 1.0f / (1.0f + expf(-opacity[i]));
    int action, cnt;
    if (op < minOpacity) { action = 3; cnt = 0; }
    else if (allowDensify && avg >= gradThreshold) { action = smax <= denseMax ? 2 : 1; cnt = 2; }
    else if (sizePrune && ((maxScreenSize > 0.0f && maxRadius[i] > maxScreenSize) || smax > worldMax)) { action = 3; cnt = 0; }
    else { action = 0; cnt = 1; }
    actions[i] = action;
    outputCounts[i] = cnt;
}

// raw opacity of alpha' with 1 - (1 - alpha')^2 = alpha (Bulo et al. 2024; gsplat's revised_opacity), alpha = sigmoid(o):
// with t = 1 - alpha = 1 / (1 + e^o) and r = sqrt(t):  alpha' = 1 - r = alpha / (1 + r),  1 - alpha' = r  -- no difference of
// nearly equal numbers on either side
__device__ __forceinline__ float revised_opacity_raw(float o)
{
    const float a = 1.0f / (1.0f + expf(-o));
    const float r = sqrtf(1.0f / (1.0f + expf(o)));
    return logf(a / ((1.0f + r) * r));
}

// The small tensors of the output rows (gather_small_kernel's sibling, on build_map_kernel's gather / noiseMode):
//   mode 1, 2 (the two children of a split)   xyz + R(q) (exp(scale) * z_j), z_j the row's own noise; scales + scaleReduction
//   mode 0, 3 (kept; a clone's two copies)    every parameter copied
// q is normalised as build_cov3d normalises it (gs_math.h).  revisedOpacity: the split children and both copies of a clone
// (the first is the mode-0 row in front of its mode-3 row) get revised_opacity_raw.
__global__ __launch_bounds__(ADC_THREADS) void adc_gather_small_kernel(
    int total, const float* __restrict__ xyz, const float* __restrict__ fdc, const float* __restrict__ scales,
    const float* __restrict__ rot, const float* __restrict__ opacity, const int* __restrict__ gather,
    const int* __restrict__ noiseMode, const float* __restrict__ noise, float scaleReduction, int revisedOpacity,
    float* __restrict__ oXyz, float* __restrict__ oFdc, float* __restrict__ oScales, float* __restrict__ oRot,
    float* __restrict__ oOpacity)
{
    const int j = blockIdx.x * ADC_THREADS + threadIdx.x;
    if (j >= total) return;
    const size_t s = (size_t)gather[j];
    const int mode = noiseMode[j];
    const bool isSplit = mode == 1 || mode == 2;
    const float sc[3] = {scales[s * 3], scales[s * 3 + 1], scales[s * 3 + 2]};
    const float q[4] = {rot[s * 4], rot[s * 4 + 1], rot[s * 4 + 2], rot[s * 4 + 3]};
    float p[3] = {xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2]};
    if (isSplit) {
        const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        const float norm = sqrtf(n2);
        const float safeNorm = norm > 1e-8f ? norm : 1e-8f;
        const float qw = q[0] / safeNorm, qx = q[1] / safeNorm, qy = q[2] / safeNorm, qz = q[3] / safeNorm;
        float R[3][3];
        R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz);
        R[0][1] = 2.0f * (qx * qy - qw * qz);
        R[0][2] = 2.0f * (qx * qz + qw * qy);
        R[1][0] = 2.0f * (qx * qy + qw * qz);
        R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz);
        R[1][2] = 2.0f * (qy * qz - qw * qx);
        R[2][0] = 2.0f * (qx * qz - qw * qy);
        R[2][1] = 2.0f * (qy * qz + qw * qx);
        R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
        float e[3];
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = expf(sc[k]) * noise[(size_t)j * 3 + k];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            float acc = R[a][0] * e[0];
            acc = acc + R[a][1] * e[1];
            acc = acc + R[a][2] * e[2];
            p[a] = p[a] + acc;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        oXyz[(size_t)j * 3 + a] = p[a];
        oScales[(size_t)j * 3 + a] = isSplit ? sc[a] + scaleReduction : sc[a];
        oFdc[(size_t)j * 3 + a] = fdc[s * 3 + a];
    }
#pragma unroll
    for (int a = 0; a < 4; a++) oRot[(size_t)j * 4 + a] = q[a];
    const float o = opacity[s];
    bool revise = false;
    if (revisedOpacity) {
        const bool cloneFirst = mode == 0 && j + 1 < total && noiseMode[j + 1] == 3 && (size_t)gather[j + 1] == s;
        revise = isSplit || mode == 3 || cloneFirst;
    }
    oOpacity[j] = revise ? revised_opacity_raw(o) : o;
}

// The Adam moments through the event (Inria's _prune_optimizer / cat_tensors_to_optimizer): a kept Gaussian and a clone's
// original keep their rows bit for bit, both children of a split and a clone's copy start at zero:
//   out[j, :] = noiseMode[j] == 0 && actions[gather[j]] != 1 ? in[gather[j], :] : 0
// One thread per float; the float4 form below for rows of whole quads between 16-byte aligned tensors, as gather_rows4_kernel.
__global__ __launch_bounds__(ADC_THREADS) void adc_gather_moments_kernel(long long totalElems, int rowLen,
                                                                         const float* __restrict__ in,
                                                                         const int* __restrict__ gather,
                                                                         const int* __restrict__ noiseMode,
                                                                         const int* __restrict__ actions, float* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * ADC_THREADS + threadIdx.x;
    if (e >= totalElems) return;
    const long long j = e / rowLen;
    const int k = (int)(e - j * rowLen);
    const size_t s = (size_t)gather[j];
    const bool kept = noiseMode[j] == 0 && actions[s] != 1;
    out[e] = kept ? in[s * rowLen + k] : 0.0f;
}

__global__ __launch_bounds__(ADC_THREADS) void adc_gather_moments4_kernel(long long totalQuads, int rowQuads,
                                                                          const float4* __restrict__ in,
                                                                          const int* __restrict__ gather,
                                                                          const int* __restrict__ noiseMode,
                                                                          const int* __restrict__ actions, float4* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * ADC_THREADS + threadIdx.x;
    if (e >= totalQuads) return;
    const long long j = e / rowQuads;
    const int k = (int)(e - j * rowQuads);
    const size_t s = (size_t)gather[j];
    const bool kept = noiseMode[j] == 0 && actions[s] != 1;
    out[e] = kept ? in[s * rowQuads + k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The opacity reset (Inria's reset_opacity: inverse_sigmoid(min(sigmoid(o), 0.01)), in raw space; its replaced optimizer
// tensor starts with zero moments): o = min(o, logit(reset value)), m = v = 0 on the opacity segment.
__global__ __launch_bounds__(ADC_THREADS) void adc_reset_opacity_kernel(int N, float* __restrict__ opacity, float* __restrict__ m,
                                                                        float* __restrict__ v, float resetRaw)
{
    const int i = blockIdx.x * ADC_THREADS + threadIdx.x;
    if (i >= N) return;
    opacity[i] = fminf(opacity[i], resetRaw);
    m[i] = 0.0f;
    v[i] = 0.0f;
}

// ---- launchers ---------------------------------------------------------------------------------------------
int launch_adc_accum(gs_ctx* c, int N, const float* rows16, const float* radii, bool useAbs, const uint32_t* gate, float* gradSum,
                     float* count, float* maxRadius)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(adc_accum_kernel, dim3(gs_div_up(N, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, N, rows16, radii,
                       useAbs ? 12 : 0, 0.5f * (float)c->W, 0.5f * (float)c->H, gate, gradSum, count, maxRadius);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_adc_classify(gs_ctx* c, int N, const float* gradSum, const float* count, const float* maxRadius, const float* scales,
                        int scaleStride, const float* opacity, float gradThreshold, float denseMax, float minOpacity,
                        float maxScreenSize, float worldMax, int allowDensify, int sizePrune, int* actions, int* outputCounts)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(adc_classify_kernel, dim3(gs_div_up(N, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, N, gradSum, count,
                       maxRadius, scales, scaleStride, opacity, gradThreshold, denseMax, minOpacity, maxScreenSize, worldMax,
                       allowDensify, sizePrune, actions, outputCounts);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

static void launch_adc_moment_rows(gs_ctx* c, long long rows, int L, const float* in, const int* gather, const int* noiseMode,
                                   const int* actions, float* out)
{
    if ((L & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
        const long long quads = rows * (L / 4);
        hipLaunchKernelGGL(adc_gather_moments4_kernel, dim3(gs_div_up(quads, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, quads,
                           L / 4, reinterpret_cast<const float4*>(in), gather, noiseMode, actions, reinterpret_cast<float4*>(out));
    } else {
        const long long elems = rows * L;
        hipLaunchKernelGGL(adc_gather_moments_kernel, dim3(gs_div_up(elems, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, elems, L,
                           in, gather, noiseMode, actions, out);
    }
}

int launch_adc_gather(gs_ctx* c, int total, int K, const float* xyz, const float* fdc, const float* frest, const float* scales,
                      const float* rot, const float* opacity, const int* gather, const int* noiseMode, const float* noise,
                      int revisedOpacity, float* oXyz, float* oFdc, float* oFrest, float* oScales, float* oRot, float* oOpacity)
{
    if (total == 0) return GS_OK;
    const float scaleReduction = (float)(-log(1.6));                    // Float(-log(1.6)), GaussianTrainer.swift:866
    hipLaunchKernelGGL(adc_gather_small_kernel, dim3(gs_div_up(total, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, total, xyz,
                       fdc, scales, rot, opacity, gather, noiseMode, noise, scaleReduction, revisedOpacity, oXyz, oFdc, oScales,
                       oRot, oOpacity);
    const int L = (K - 1) * 3;
    if (L > 0) launch_gather_rows(c, total, L, frest, gather, oFrest, nullptr);      // (densify.hip: the existing row gather)
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_adc_gather_moments(gs_ctx* c, int total, int K, const int* gather, const int* noiseMode, const int* actions,
                              const float* const in[6], float* const out[6])
{
    if (total == 0) return GS_OK;
    const int per[6] = {3, 3, 3 * (K - 1), 3, 4, 1};       // xyz, features_dc, features_rest, scales, rotation, opacity
    for (int t = 0; t < 6; t++)
        if (per[t] > 0) launch_adc_moment_rows(c, total, per[t], in[t], gather, noiseMode, actions, out[t]);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_adc_reset_opacity(gs_ctx* c, int N, float* opacity, float* m, float* v, float resetRaw)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(adc_reset_opacity_kernel, dim3(gs_div_up(N, ADC_THREADS)), dim3(ADC_THREADS), 0, c->stream, N, opacity, m, v,
                       resetRaw);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
