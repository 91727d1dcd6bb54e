// gs_mcmc.h -- the per-step arithmetic of the MCMC densification strategy (include/gsplat.h gs_set_mcmc),
// shared by the fused projection backward + Adam (projection.hip) and the stand-alone ops (mcmc.hip) so that both paths
// compute the same float32 values from the same inputs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsplat.h"

namespace gs {

// Philox4x32-10 streams of the strategy: counter = (row or draw, iteration, MCMC_TAG0, tag), key = the seed.  densify.hip's
// split / clone noise uses counter (row, 0, 0x64656e73, 0x69667921): the streams never share a counter.
constexpr uint32_t MCMC_TAG0 = 0x6d636d63u;          // "mcmc"
constexpr uint32_t MCMC_TAG_NOISE = 0x6e6f6973u;     // "nois": the per-step position noise, keyed by (row, t)
constexpr uint32_t MCMC_TAG_RELOCATE = 0x72656c6fu;  // "relo": the relocation's source draws, keyed by (draw, t)
constexpr uint32_t MCMC_TAG_GROW = 0x67726f77u;      // "grow": the growth's source draws, keyed by (draw, t)

__device__ __forceinline__ void mcmc_philox(uint32_t i, uint32_t t, uint32_t tag, unsigned long long seed, uint32_t (&c)[4])
{
    c[0] = i; c[1] = t; c[2] = MCMC_TAG0; c[3] = tag;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// three standard normals from the four words (Box-Muller, as densify.hip's densify_noise3)
__device__ __forceinline__ void mcmc_normals(const uint32_t (&c)[4], float (&z)[3])
{
    const float u0 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = ((float)(c[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
    float sa, ca;
    sincosf(6.283185307179586f * u1, &sa, &ca);
    z[0] = ra * ca; z[1] = ra * sa; z[2] = rb * cosf(6.283185307179586f * u3);
}

// one uniform in (0, 1) with 53 bits from the first two words: ((w0 >> 5) 2^26 + (w1 >> 6) + 1/2) 2^-53
__device__ __forceinline__ double mcmc_uniform(const uint32_t (&c)[4])
{
    const unsigned long long m = ((unsigned long long)(c[0] >> 5) << 26) | (unsigned long long)(c[1] >> 6);
    return ((double)m + 0.5) * (1.0 / 9007199254740992.0);
}

// What a step adds (gs_set_mcmc): the regularisers' gradient coefficients opacity_reg / N and scale_reg / (3 N), and the
// noise's scale noise_lr lr_xyz(t) -- float32, formed on the host in float64 by the launchers
struct McmcFuse {
    float oCoef, sCoef, noiseScale;
    uint32_t iteration;
    unsigned long long seed;
};

// o (1 - o) of o = sigmoid(x), the opacity regulariser's derivative: e / (1 + e)^2 with e = exp(-|x|), good to a few ulp for
// every x (1 - sigmoid(x) in float32 loses all digits as o approaches 1)
__device__ __forceinline__ float mcmc_sigmoid_slope(float x)
{
    const float e = expf(-fabsf(x));
    return e / ((1.0f + e) * (1.0f + e));
}

// the position noise of row i from its parameters after the step's Adam update:
//   d = Sigma eps noise_scale / (1 + exp(-100 ((1 - o) - 0.995))),  Sigma = R diag(s^2) R^T
// s = exp(scales_raw), R from q / (|q| + 1e-8), o = sigmoid(opacity_raw), eps ~ N(0, I3) from (seed, t, i)
__device__ __forceinline__ void mcmc_noise(const McmcFuse& mc, uint32_t i, const float sr[3], const float rr[4], float opr,
                                           float (&d)[3])
{
    uint32_t w[4];
    mcmc_philox(i, mc.iteration, MCMC_TAG_NOISE, mc.seed, w);
    float z[3];
    mcmc_normals(w, z);
    const float den = sqrtf(rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3]) + 1e-8f;
    const float qw = rr[0] / den, qx = rr[1] / den, qy = rr[2] / den, qz = rr[3] / den;
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
    float a[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = expf(sr[k]);
        a[k] = (R[0][k] * z[0] + R[1][k] * z[1] + R[2][k] * z[2]) * (s * s);
    }
    const float o = 1.0f / (1.0f + expf(-opr));
    const float gate = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
    const float f = mc.noiseScale * gate;
#pragma unroll
    for (int r = 0; r < 3; r++) d[r] = (R[r][0] * a[0] + R[r][1] * a[1] + R[r][2] * a[2]) * f;
}

// the launchers' McmcFuse for a step over N Gaussians at xyz learning rate lrXyz
inline McmcFuse mcmc_fuse(const gs_mcmc_params& p, int N, float lrXyz)
{
    McmcFuse f;
    const double n = N > 0 ? (double)N : 1.0;
    f.oCoef = (float)(p.opacity_reg / n);
    f.sCoef = (float)(p.scale_reg / (3.0 * n));
    f.noiseScale = (float)(p.noise_lr * (double)lrXyz);
    f.iteration = (uint32_t)p.iteration;
    f.seed = p.seed;
    return f;
}

}  // namespace gs
