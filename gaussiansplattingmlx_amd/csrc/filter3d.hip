// filter3d.hip -- the 3-D smoothing filter's own kernels (include/gsplat.h gs_compute_filter3d / gs_filter3d_bake, DESIGN.md
// section 14): the per-Gaussian filter width from the training cameras, and the fused export.  The filtered activations and
// their VJP live in gs_math.h (filter3d_activate) and run inside the fused projection kernels (projection.hip).  Compiled with
// -ffp-contract=off: every product and sum below rounds where it is written, so a width does not depend on the build.
//
//   filter3d_width_kernel   one lane per Gaussian; the camera table goes through LDS in chunks of F3D_CHUNK cameras and is read
//                           wave-uniformly (a broadcast, no bank conflicts); a running min of z / focal_x over the cameras
//                           that see the Gaussian, cameras in table order, one fixed expression per (Gaussian, camera) -- the
//                           result does not depend on the launch shape.  Writes sqrt(0.2) min, or -1 where no camera sees the
//                           Gaussian, and raises the ctx's max word (the float bits of a positive float order as unsigned
//                           integers; one vector atomicMax per wave).
//   filter3d_fixup_kernel   the never-seen rule: -1 -> the largest width among the seen (0 when nothing was seen: the word's
//                           initial 0 bits).
//   filter3d_bake_kernel    elementwise: scales_raw' = log(s_eff), opacity_raw' = logit(sigma kappa).
#include "gs_ctx.h"
#include "gs_math.h"

namespace gs {

constexpr int F3D_THREADS = 256;
constexpr int F3D_CHUNK = 64;              // cameras per LDS chunk: 64 x 16 floats = 4 KB

__global__ __launch_bounds__(F3D_THREADS) void filter3d_width_kernel(int N, int V, const float* __restrict__ cams,
                                                                     const float* __restrict__ xyz, float* __restrict__ filter,
                                                                     uint32_t* __restrict__ maxBits)
{
    __shared__ float sCam[F3D_CHUNK * GS_F3D_CAM_FLOATS];
    const int p = blockIdx.x * F3D_THREADS + threadIdx.x;
    const bool live = p < N;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = xyz[3 * (size_t)p]; y = xyz[3 * (size_t)p + 1]; z = xyz[3 * (size_t)p + 2]; }
    float best = -1.0f;                    // (no camera yet)
    for (int v0 = 0; v0 < V; v0 += F3D_CHUNK) {          // (uniform: every thread of the block takes both barriers)
        const int nv = min(F3D_CHUNK, V - v0);
        __syncthreads();                   // the previous chunk has been read
        for (int i = threadIdx.x; i < nv * GS_F3D_CAM_FLOATS; i += F3D_THREADS) sCam[i] = cams[(size_t)v0 * GS_F3D_CAM_FLOATS + i];
        __syncthreads();
        if (live) {
            for (int v = 0; v < nv; v++) {
                const float* c = sCam + v * GS_F3D_CAM_FLOATS;      // view columns 0 .. 2 (rows 0 .. 3 each), limX, limY, focalX
                const float px = x * c[0] + y * c[1] + z * c[2] + c[3];
                const float py = x * c[4] + y * c[5] + z * c[6] + c[7];
                const float pz = x * c[8] + y * c[9] + z * c[10] + c[11];
                const bool seen = pz >= 0.2f && fabsf(px / pz) <= c[12] && fabsf(py / pz) <= c[13];
                const float t = pz / c[14];
                if (seen && (best < 0.0f || t < best)) best = t;
            }
        }
    }
    const float f = best < 0.0f ? -1.0f : sqrtf(0.2f) * best;
    if (live) filter[p] = f;
    // the device-wide max over the seen: f > 0 there (z >= 0.2, focal > 0), and unsigned order is float order on positive floats
    uint32_t bits = (live && f > 0.0f) ? __float_as_uint(f) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, o, 64));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(maxBits, bits);
}

__global__ __launch_bounds__(F3D_THREADS) void filter3d_fixup_kernel(int N, float* __restrict__ filter,
                                                                     const uint32_t* __restrict__ maxBits)
{
    const int p = blockIdx.x * F3D_THREADS + threadIdx.x;
    if (p >= N) return;
    if (filter[p] < 0.0f) filter[p] = __uint_as_float(*maxBits);
}

// logit(sigma kappa) = log kappa - log((1 - kappa) + exp(-o)), with 1 - kappa = (1 - r0) + r0 (1 - r1) + r0 r1 (1 - r2) and
// 1 - r_a = f^2 / (s_eff_a (s_eff_a + s_a)): no cancellation where kappa is close to 1 (f = 0 gives back o up to the two
// logarithms' rounding).  Outputs may alias inputs: every lane reads its row before it writes it.
__global__ __launch_bounds__(F3D_THREADS) void filter3d_bake_kernel(int N, const float* scalesRaw, const float* opacityRaw,
                                                                    const float* __restrict__ filter, float* outScales,
                                                                    float* outOpacity)
{
    const int p = blockIdx.x * F3D_THREADS + threadIdx.x;
    if (p >= N) return;
    const float s[3] = {expf(scalesRaw[3 * (size_t)p]), expf(scalesRaw[3 * (size_t)p + 1]), expf(scalesRaw[3 * (size_t)p + 2])};
    const float o = opacityRaw[p], f = filter[p];
    float se[3];
    const float kappa = filter3d_activate(s, f, se);
    const float f2 = f * f;
    float d[3], r[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { d[a] = f2 / (se[a] * (se[a] + s[a])); r[a] = s[a] / se[a]; }
    const float omk = d[0] + r[0] * d[1] + r[0] * r[1] * d[2];
#pragma unroll
    for (int a = 0; a < 3; a++) outScales[3 * (size_t)p + a] = logf(se[a]);
    outOpacity[p] = logf(kappa) - logf(omk + expf(-o));
}

int launch_filter3d_width(gs_ctx* c, int N, const float* xyz, float* filter)
{
    GS_HIP_CHECK(c, hipMemsetAsync(c->f3dMax, 0, sizeof(uint32_t), c->stream));
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(filter3d_width_kernel, dim3(gs_div_up(N, F3D_THREADS)), dim3(F3D_THREADS), 0, c->stream, N, c->f3dCamCount,
                       c->f3dCams, xyz, filter, c->f3dMax);
    hipLaunchKernelGGL(filter3d_fixup_kernel, dim3(gs_div_up(N, F3D_THREADS)), dim3(F3D_THREADS), 0, c->stream, N, filter, c->f3dMax);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_filter3d_bake(gs_ctx* c, int N, const float* scalesRaw, const float* opacityRaw, const float* filter, float* outScales,
                         float* outOpacity)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(filter3d_bake_kernel, dim3(gs_div_up(N, F3D_THREADS)), dim3(F3D_THREADS), 0, c->stream, N, scalesRaw, opacityRaw,
                       filter, outScales, outOpacity);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
