// projection.hip -- 3D->2D projection, EWA covariance, SH->RGB: forward + backward.
// Compiled with -ffp-contract=off (see gs_math.h).
//
// Two flavours of each direction:
//  * op-level kernels mirror the reference's custom-function boundary
//    (gaussian_projection_screen_fused_forward/backward,
//    slang/gaussian_projection_kernels.slang:36-173, 205-398): activated inputs,
//    8 output tensors / 5 gradient tensors;
//  * fused kernels start from the six RAW parameter tensors, fold the
//    activations (GaussianRenderer.swift:936-963) and the packing (:85-99) in,
//    and emit what binning needs (tile rectangle, tiles touched, depth key), so
//    the per-Gaussian data crosses HBM once.
// One lane per Gaussian; HBM-bound (408 B/Gaussian forward, 728 B backward at K=25).
#include <type_traits>

#include "gs_ctx.h"
#include "gs_mcmc.h"
#include "gs_rider.h"

namespace gs {

constexpr int PROJ_THREADS = 256;

CamParams make_cam(const gs_camera* cam, int W, int H)
{
    CamParams p;
    for (int i = 0; i < 16; i++) { p.V[i] = cam->view[i]; p.P[i] = cam->proj[i]; }
    for (int i = 0; i < 3; i++) p.cam[i] = cam->cam_center[i];
    p.fovX = cam->fov_x; p.fovY = cam->fov_y; p.focalX = cam->focal_x; p.focalY = cam->focal_y;
    p.limX = tanf(cam->fov_x * 0.5f) * 1.3f;
    p.limY = tanf(cam->fov_y * 0.5f) * 1.3f;
    p.W = (float)W; p.H = (float)H;
    return p;
}

// ---------------------------------------------------------------------------------------------
// op-level forward
// ---------------------------------------------------------------------------------------------
// FISHEYE: the camera model (gs_set_camera_model).  The pinhole kernel keeps its name and its code; the fisheye one stands beside it.
template <bool FISHEYE>
__device__ __forceinline__ void proj_fwd_op_body(
    int N, int K, int degree, const CamParams& cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, float* __restrict__ means2d,
    float* __restrict__ depths, float* __restrict__ color, float* __restrict__ cov2d, float* __restrict__ conic,
    float* __restrict__ radii, float* __restrict__ rectMin, float* __restrict__ rectMax)
{
    const int p = blockIdx.x * PROJ_THREADS + threadIdx.x;
    if (p >= N) return;
    const float m[3] = {means3d[3 * p], means3d[3 * p + 1], means3d[3 * p + 2]};
    const float s[3] = {scales[3 * p], scales[3 * p + 1], scales[3 * p + 2]};
    const float q[4] = {rot[4 * p], rot[4 * p + 1], rot[4 * p + 2], rot[4 * p + 3]};
    ProjOut o;
    project_geometry<FISHEYE>(m, s, q, cam, o);

    const float x = m[0] - cam.cam[0], y = m[1] - cam.cam[1], z = m[2] - cam.cam[2];
    const float* sh = shs + (size_t)p * K * 3;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    sh_foreach(degree, x, y, z, [&](int k, float b, float, float, float) {
        if (k == 0) { c0 = b * sh[0]; c1 = b * sh[1]; c2 = b * sh[2]; }
        else { c0 += b * sh[k * 3]; c1 += b * sh[k * 3 + 1]; c2 += b * sh[k * 3 + 2]; }
    });
    c0 += 0.5f; c1 += 0.5f; c2 += 0.5f;
    color[3 * p] = c0 > 0.f ? c0 : 0.f;
    color[3 * p + 1] = c1 > 0.f ? c1 : 0.f;
    color[3 * p + 2] = c2 > 0.f ? c2 : 0.f;

    means2d[2 * p] = o.sx; means2d[2 * p + 1] = o.sy;
    depths[p] = o.depth;
#pragma unroll
    for (int k = 0; k < 4; k++) { cov2d[4 * p + k] = o.cov2d[k]; conic[4 * p + k] = o.conic[k]; }
    radii[p] = o.radius;
    rectMin[2 * p] = o.rect[0]; rectMin[2 * p + 1] = o.rect[1];
    rectMax[2 * p] = o.rect[2]; rectMax[2 * p + 1] = o.rect[3];
}

// (two plain kernels over the body rather than one templated kernel: as a template instance the pinhole kernel compiled to 809
// instructions where the parent has 841 -- this way it keeps the parent's)
__global__ __launch_bounds__(PROJ_THREADS) void proj_fwd_op_kernel(
    int N, int K, int degree, CamParams cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, float* __restrict__ means2d,
    float* __restrict__ depths, float* __restrict__ color, float* __restrict__ cov2d, float* __restrict__ conic,
    float* __restrict__ radii, float* __restrict__ rectMin, float* __restrict__ rectMax)
{
    proj_fwd_op_body<false>(N, K, degree, cam, scales, rot, means3d, shs, means2d, depths, color, cov2d, conic, radii, rectMin, rectMax);
}
__global__ __launch_bounds__(PROJ_THREADS) void proj_fwd_op_fisheye_kernel(
    int N, int K, int degree, CamParams cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, float* __restrict__ means2d,
    float* __restrict__ depths, float* __restrict__ color, float* __restrict__ cov2d, float* __restrict__ conic,
    float* __restrict__ radii, float* __restrict__ rectMin, float* __restrict__ rectMax)
{
    proj_fwd_op_body<true>(N, K, degree, cam, scales, rot, means3d, shs, means2d, depths, color, cov2d, conic, radii, rectMin, rectMax);
}

// ---------------------------------------------------------------------------------------------
// colour reverse mode shared by both backward kernels.  SHLOAD(k, ch) reads a coefficient,
// SHSTORE(k, ch, v) writes its gradient.  Returns d(x,y,z).
// ---------------------------------------------------------------------------------------------
template <class Load, class Store>
__device__ __forceinline__ void color_backward(int degree, int K, float x, float y, float z, const float cotCol[3],
                                               Load&& shload, Store&& shstore, float dxyz[3], float* mgOut = nullptr)
{
    float acc[3] = {0.f, 0.f, 0.f};
    sh_foreach(degree, x, y, z, [&](int k, float b, float, float, float) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) acc[ch] = (k == 0) ? b * shload(k, ch) : acc[ch] + b * shload(k, ch);
    });
    float mg[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) mg[ch] = d_max_left(acc[ch] + 0.5f, 0.0f, cotCol[ch]);
    if (mgOut) { mgOut[0] = mg[0]; mgOut[1] = mg[1]; mgOut[2] = mg[2]; }
    float dx = 0.f, dy = 0.f, dz = 0.f;
    int written = 0;
    sh_foreach(degree, x, y, z, [&](int k, float b, float gx, float gy, float gz) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float coef = shload(k, ch);      // read first: the fused kernel stores the gradient in place
            shstore(k, ch, b * mg[ch]);
            const float w = coef * mg[ch];
            dx += gx * w; dy += gy * w; dz += gz * w;
        }
        written = k + 1;
    });
    for (int k = written; k < K; k++)
        for (int ch = 0; ch < 3; ch++) shstore(k, ch, 0.0f);
    dxyz[0] = dx; dxyz[1] = dy; dxyz[2] = dz;
}

// ---------------------------------------------------------------------------------------------
// op-level backward
// ---------------------------------------------------------------------------------------------
template <bool FISHEYE>
__device__ __forceinline__ void proj_bwd_op_body(
    int N, int K, int degree, const CamParams& cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, const float* __restrict__ cotDepths,
    const float* __restrict__ cotMeans2d, const float* __restrict__ cotCov2d, const float* __restrict__ cotColor,
    const float* __restrict__ cotConic, float* __restrict__ gScales, float* __restrict__ gRot,
    float* __restrict__ gMeans, float* __restrict__ gShs, float* __restrict__ gCam)
{
    const int p = blockIdx.x * PROJ_THREADS + threadIdx.x;
    if (p >= N) return;
    const float m[3] = {means3d[3 * p], means3d[3 * p + 1], means3d[3 * p + 2]};
    const float s[3] = {scales[3 * p], scales[3 * p + 1], scales[3 * p + 2]};
    const float q[4] = {rot[4 * p], rot[4 * p + 1], rot[4 * p + 2], rot[4 * p + 3]};
    const float cm[2] = {cotMeans2d[2 * p], cotMeans2d[2 * p + 1]};
    const float ccov[4] = {cotCov2d[4 * p], cotCov2d[4 * p + 1], cotCov2d[4 * p + 2], cotCov2d[4 * p + 3]};
    const float ccon[4] = {cotConic[4 * p], cotConic[4 * p + 1], cotConic[4 * p + 2], cotConic[4 * p + 3]};
    GeomGrads g;
    project_geometry_bwd<false, false, FISHEYE>(m, s, q, cam, cm, cotDepths[p], ccov, ccon, g);

    const float x = m[0] - cam.cam[0], y = m[1] - cam.cam[1], z = m[2] - cam.cam[2];
    const float* sh = shs + (size_t)p * K * 3;
    float* gsh = gShs + (size_t)p * K * 3;
    const float cc[3] = {cotColor[3 * p], cotColor[3 * p + 1], cotColor[3 * p + 2]};
    float d[3];
    color_backward(degree, K, x, y, z, cc, [&](int k, int ch) { return sh[k * 3 + ch]; },
                   [&](int k, int ch, float v) { gsh[k * 3 + ch] = v; }, d);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        gMeans[3 * p + a] = g.dm[a] + d[a];
        gCam[3 * p + a] = -d[a];
        gScales[3 * p + a] = g.ds[a];
    }
#pragma unroll
    for (int a = 0; a < 4; a++) gRot[4 * p + a] = g.dq[a];
}

__global__ __launch_bounds__(PROJ_THREADS) void proj_bwd_op_kernel(
    int N, int K, int degree, CamParams cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, const float* __restrict__ cotDepths,
    const float* __restrict__ cotMeans2d, const float* __restrict__ cotCov2d, const float* __restrict__ cotColor,
    const float* __restrict__ cotConic, float* __restrict__ gScales, float* __restrict__ gRot,
    float* __restrict__ gMeans, float* __restrict__ gShs, float* __restrict__ gCam)
{
    proj_bwd_op_body<false>(N, K, degree, cam, scales, rot, means3d, shs, cotDepths, cotMeans2d, cotCov2d, cotColor, cotConic, gScales,
                            gRot, gMeans, gShs, gCam);
}
__global__ __launch_bounds__(PROJ_THREADS) void proj_bwd_op_fisheye_kernel(
    int N, int K, int degree, CamParams cam, const float* __restrict__ scales, const float* __restrict__ rot,
    const float* __restrict__ means3d, const float* __restrict__ shs, const float* __restrict__ cotDepths,
    const float* __restrict__ cotMeans2d, const float* __restrict__ cotCov2d, const float* __restrict__ cotColor,
    const float* __restrict__ cotConic, float* __restrict__ gScales, float* __restrict__ gRot,
    float* __restrict__ gMeans, float* __restrict__ gShs, float* __restrict__ gCam)
{
    proj_bwd_op_body<true>(N, K, degree, cam, scales, rot, means3d, shs, cotDepths, cotMeans2d, cotCov2d, cotColor, cotConic, gScales,
                           gRot, gMeans, gShs, gCam);
}

// ---------------------------------------------------------------------------------------------
// SH-rest staging.  features_rest is [N][K-1][3]: 288 B per Gaussian at K = 25.  Read straight from a
// lane-per-Gaussian kernel every load instruction touches 64 different cache lines; instead each wavefront
// moves its 64 rows (one contiguous 18 KB span) through LDS with fully coalesced dwordx4 accesses and then
// reads / writes its own row at stride L+1 words (odd, so bank-conflict free).
// ---------------------------------------------------------------------------------------------
constexpr int PROJ_FUSED_THREADS = 128;   // 2 waves x 64 rows x 73 words = 37 KB of LDS per workgroup at K = 25

// float4 per lane of one wave's rows at K = 25: 64 rows x 72 floats / 64 lanes / 4
constexpr int SH_ROWS_MAX4 = 18;
#ifndef GS_PROJ_LATE_MOMENTS
#define GS_PROJ_LATE_MOMENTS 1
#endif

// The loads of a whole batch are issued before the first LDS store, unconditionally and from clamped addresses: as a
// plain loop (`v = g4[e]; store to LDS`) every iteration waited for its own load -- 18 memory latencies in a row at
// the head of every wave of an HBM-bound kernel.  `keep` returns the batch to the caller (the fused Adam update needs
// the parameter values again after their LDS rows have been overwritten with gradients).
__device__ __forceinline__ void sh_rows_load4(const float* __restrict__ g, int total4, int e0, int lane,
                                              float4 (&regs)[SH_ROWS_MAX4])
{
    const float4* g4 = reinterpret_cast<const float4*>(g);     // wave spans start 16-B aligned when L % 4 == 0
#pragma unroll
    for (int i = 0; i < SH_ROWS_MAX4; i++) regs[i] = g4[min(e0 + lane + 64 * i, total4 - 1)];
}
__device__ __forceinline__ void sh_rows_to_lds4(float* __restrict__ lds, int total4, int L, int e0, int lane,
                                                const float4 (&regs)[SH_ROWS_MAX4])
{
#pragma unroll
    for (int i = 0; i < SH_ROWS_MAX4; i++) {
        const int e = e0 + lane + 64 * i;
        if (e < total4) {
            const int r = (e * 4) / L, c = e * 4 - r * L;
            float* d = lds + r * (L + 1) + c;
            d[0] = regs[i].x; d[1] = regs[i].y; d[2] = regs[i].z; d[3] = regs[i].w;
        }
    }
}

__device__ __forceinline__ void sh_rows_in(float* __restrict__ lds, const float* __restrict__ g, int rows, int L,
                                           int lane)
{
    const int total = rows * L;
    if ((L & 3) == 0) {
        const int total4 = total >> 2;
        for (int e0 = 0; e0 < total4; e0 += 64 * SH_ROWS_MAX4) {
            float4 regs[SH_ROWS_MAX4];
            sh_rows_load4(g, total4, e0, lane, regs);
            sh_rows_to_lds4(lds, total4, L, e0, lane, regs);
        }
    } else {
        for (int e = lane; e < total; e += 64) {
            const int r = e / L, c = e - r * L;
            lds[r * (L + 1) + c] = g[e];
        }
    }
}

// (half-row staging for the fused forward: sh_half_load / sh_half_to_lds, gs_rider.h)
__device__ __forceinline__ void sh_rows_out(const float* __restrict__ lds, float* __restrict__ g, int rows, int L,
                                            int lane)
{
    const int total = rows * L;
    if ((L & 3) == 0) {
        float4* g4 = reinterpret_cast<float4*>(g);
        for (int e = lane; e * 4 < total; e += 64) {
            const int r = (e * 4) / L, c = e * 4 - r * L;
            const float* d = lds + r * (L + 1) + c;
            g4[e] = make_float4(d[0], d[1], d[2], d[3]);
        }
    } else {
        for (int e = lane; e < total; e += 64) {
            const int r = e / L, c = e - r * L;
            g[e] = lds[r * (L + 1) + c];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fused forward: raw parameters -> packed12 + binning inputs
// ---------------------------------------------------------------------------------------------
// COLOUR = false: geometry only -- the colour floats of the packed record are left to the riders of the binning kernels
// (gs_rider.h), no SH row is touched here, no LDS.
// SELF (with COLOUR = false): the wave computes its own Gaussians' colours right behind the geometry, as a rider unit would
// (colour_rider_wave: SH rows of Gaussians that touch no tile are not fetched) -- for the sizes where no binning kernel has
// room for riders and a large part of the Gaussians is outside the view (the 2 M garden scene: 48 %).
#ifndef GS_DEGENERATE_INVISIBLE
#define GS_DEGENERATE_INVISIBLE 1
#endif
#include "gs_proj_fwd_kernel.h"

// ---------------------------------------------------------------------------------------------
// fused backward: gradAcc16 (d packed) + raw parameters -> raw-parameter gradients
// ---------------------------------------------------------------------------------------------
// EMIT_MG: data-parallel variant.  The SH gradient of one view is the outer product basis_k(xyz - cam) x mg with
// mg[3] the colour cotangent after the max(., 0) gate, so a rank only has to publish mg (12 B per Gaussian instead
// of 12 K); every rank rebuilds and sums the SH gradients of all views itself (sh_grad_from_views_kernel).
//
// MODE 2 (ADAM): no gradient leaves the kernel; every parameter element is updated in place with its Adam step
// (optim.hip's arithmetic) against the moment arenas that mirror the parameter arena.  It saves the gradient
// arena's round trip (written here, read by adam_kernel): 344 B of the ~1 KB per Gaussian the two kernels move.
struct AdamFuse {
    const float* pBase;   // parameter arena base: every tensor of the forward lies inside it
    float* mBase;
    float* vBase;
    float lr[6];          // xyz, f_dc, f_rest, scales, rotation, opacity
    float b1, b2, eps, gscale;
    const uint32_t* gate; // device word: non-zero = leave parameters and moments alone (the forward overflowed its
                          // reserved pair capacity and rendered nothing: gs_ctx.h adamGate)
    // data-parallel steps (round 5: the step's gate rides in its first collective, dp.hip):
    const uint32_t* ovf;  // the forward's overflow word and
    float* rider;         // where the kernel's first thread stores it as 0.0f / 1.0f (gs_set_overflow_rider), or nullptr
    // the gate as the OR of `gwCount` words `gwStride` apart (the ranks' riders behind their gathered colour cotangents:
    // gs_set_gathered_gate), stored to gwOut for the optimizer kernels queued behind; gwWords == nullptr: *gate
    const uint32_t* gwWords;
    long long gwStride;
    int gwCount;
    uint32_t* gwOut;
    uint32_t* seen;       // set to 1 by a kernel that finds its gate raised (gs_set_gate_seen), or nullptr
};

// the gate of an optimizer kernel: its one word, or the OR of the gathered words (every thread reads the same few words)
__device__ __forceinline__ uint32_t adam_gate_word(const AdamFuse& A)
{
    if (!A.gwWords) return A.gate ? *A.gate : 0u;
    uint32_t g = 0;
    for (int r = 0; r < A.gwCount; r++) g |= A.gwWords[(long long)r * A.gwStride];
    return g;
}
// ... published by the kernel's first thread
__device__ __forceinline__ void adam_gate_publish(const AdamFuse& A, uint32_t g)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (A.gwWords && A.gwOut) *A.gwOut = g;
        if (g && A.seen) *A.seen = 1u;
    }
}

// one element's Adam step on values already in registers (the loads are issued long before, the stores after)
__device__ __forceinline__ void adam_step(const AdamFuse& A, float g, float lr, float& p, float& m, float& v)
{
    const float gr = g * A.gscale;
    m = A.b1 * m + (1.0f - A.b1) * gr;
    v = A.b2 * v + (1.0f - A.b2) * gr * gr;
    p = p - gs_adam_delta(lr, m, v, A.eps);
}

// Adam over the f_rest rows of one wave (64 Gaussians), gradients in the wave's LDS rows: walked in memory order
// against p, m, v, four consecutive elements per lane, the loads of a whole batch in flight before the first update
// (nothing may wait on a store).  16-B accesses need 16-B aligned addresses: scalar head up to the first aligned
// element, float4 body, scalar tail.
// SPARSE (sparse Adam, gs_set_sparse_adam): bit r of visBits = row r of the wave is visible.  Only the elements of visible rows
// move; a float4 none of whose rows is visible is neither loaded nor stored, one that straddles a visible and an invisible
// row (L % 4 != 0) is loaded and written back whole with the invisible row's elements as they came.
template <bool SPARSE = false>
__device__ __forceinline__ void adam_rows(const AdamFuse& adam, const float* frest, int row0, int rows, int L,
                                          const float* myRows, int lane, float lr, unsigned long long visBits = ~0ull)
{
    const size_t off0 = (size_t)(frest - adam.pBase) + (size_t)row0 * L;
    float* P = const_cast<float*>(adam.pBase) + off0;
    float* M = adam.mBase + off0;
    float* V = adam.vBase + off0;
    const int total = rows * L;
    auto grad_at = [&](int e) { const int r = e / L; return myRows[r * (L + 1) + (e - r * L)]; };
    auto vis_at = [&](int e) { return ((visBits >> (e / L)) & 1ull) != 0ull; };      // (SPARSE only)
    const int head = min(total, (int)((4 - (off0 & 3)) & 3));
    const int n4 = (total - head) >> 2;
    const int tail0 = head + 4 * n4;
    if (lane < head + (total - tail0)) {
        const int e = lane < head ? lane : tail0 + (lane - head);
        bool on = true;
        if constexpr (SPARSE) on = vis_at(e);
        if (on) {
            float pv = P[e], mv = M[e], vv = V[e];
            adam_step(adam, grad_at(e), lr, pv, mv, vv);
            P[e] = pv; M[e] = mv; V[e] = vv;
        }
    }
    float4* P4 = reinterpret_cast<float4*>(P + head);
    float4* M4 = reinterpret_cast<float4*>(M + head);
    float4* V4 = reinterpret_cast<float4*>(V + head);
    if constexpr (SPARSE) {
        // one float4 at a time (this form serves the spans the kept registers do not: K != 25, or an unaligned span).  A float4
        // spans at most two rows (L >= 3), and f, f + 3 name them.
        for (int e = lane; e < n4; e += 64) {
            const int f = head + 4 * e;
            const bool v0 = vis_at(f), v1 = vis_at(f + 1), v2 = vis_at(f + 2), v3 = vis_at(f + 3);
            if (!(v0 || v3)) continue;
            float4 p4 = P4[e], m4 = M4[e], w4 = V4[e];
            if (v0) adam_step(adam, grad_at(f), lr, p4.x, m4.x, w4.x);
            if (v1) adam_step(adam, grad_at(f + 1), lr, p4.y, m4.y, w4.y);
            if (v2) adam_step(adam, grad_at(f + 2), lr, p4.z, m4.z, w4.z);
            if (v3) adam_step(adam, grad_at(f + 3), lr, p4.w, m4.w, w4.w);
            P4[e] = p4; M4[e] = m4; V4[e] = w4;
        }
        return;
    }
    constexpr int B = 6;
    for (int e0 = lane; e0 < n4; e0 += 64 * B) {
        float4 pp[B], mm[B], vv[B];
#pragma unroll
        for (int b = 0; b < B; b++) {      // unconditional, clamped: every load of the batch in flight at once
            const int e = min(e0 + 64 * b, n4 - 1);
            pp[b] = P4[e]; mm[b] = M4[e]; vv[b] = V4[e];
        }
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int e = e0 + 64 * b;
            if (e < n4) {
                const int f = head + 4 * e;
                adam_step(adam, grad_at(f), lr, pp[b].x, mm[b].x, vv[b].x);
                adam_step(adam, grad_at(f + 1), lr, pp[b].y, mm[b].y, vv[b].y);
                adam_step(adam, grad_at(f + 2), lr, pp[b].z, mm[b].z, vv[b].z);
                adam_step(adam, grad_at(f + 3), lr, pp[b].w, mm[b].w, vv[b].w);
                P4[e] = pp[b]; M4[e] = mm[b]; V4[e] = vv[b];
            }
        }
    }
}

// The same update when the wave's parameter rows are still in registers from the staging load (sh_rows_load4: float4
// `lane + 64 i` of the span, 16-B aligned): f_rest is read from HBM once, not twice -- its LDS copy has been overwritten
// with the gradients by now, and a second read of the 18 KB span came from HBM again (the PMC fetch bytes of the
// kernel were 1.25x its algorithmic bytes, the excess = N x 288 B).  Moments in batches of 3 float4, one batch ahead
// (the 18 kept float4 leave room for no more under the 256 registers of two waves per SIMD).
// SPARSE: as adam_rows; L % 4 == 0 here, so a float4 lies in one row and is either updated whole or left alone (its moments
// not loaded, nothing stored).
template <bool SPARSE = false>
__device__ __forceinline__ void adam_rows_kept(const AdamFuse& adam, const float* frest, int row0, int total4, int L,
                                               const float* myRows, int lane, float lr,
                                               float4 (&pp)[SH_ROWS_MAX4], unsigned long long visBits = ~0ull)
{
    const size_t off0 = (size_t)(frest - adam.pBase) + (size_t)row0 * L;
    float4* P4 = reinterpret_cast<float4*>(const_cast<float*>(adam.pBase) + off0);
    float4* M4 = reinterpret_cast<float4*>(adam.mBase + off0);
    float4* V4 = reinterpret_cast<float4*>(adam.vBase + off0);
    auto grad_at = [&](int e) { const int r = e / L; return myRows[r * (L + 1) + (e - r * L)]; };
    constexpr int B = 3, NB = SH_ROWS_MAX4 / B;
    static_assert(NB * B == SH_ROWS_MAX4, "whole batches");
#ifndef GS_ADAM_ROWS_DEPTH
#define GS_ADAM_ROWS_DEPTH 2
#endif
    constexpr int D = GS_ADAM_ROWS_DEPTH;      // batches of moments in flight ahead of the update
    float4 mm[D][B], vv[D][B];
    auto vis4 = [&](int e) { return ((visBits >> ((4 * e) / L)) & 1ull) != 0ull; };      // (SPARSE only)
    auto load = [&](int k, float4 (&m)[B], float4 (&v)[B]) {
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int e = min(lane + 64 * (k * B + b), total4 - 1);
            if constexpr (SPARSE) {
                float4 mz = make_float4(0.f, 0.f, 0.f, 0.f), vz = mz;
                if (vis4(e)) { mz = M4[e]; vz = V4[e]; }
                m[b] = mz; v[b] = vz;
            } else {
                m[b] = M4[e]; v[b] = V4[e];
            }
        }
    };
    auto update = [&](int k, float4 (&m)[B], float4 (&v)[B]) {
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int e = lane + 64 * (k * B + b);
            bool on = e < total4;
            if constexpr (SPARSE) on = on && vis4(e);
            if (on) {
                float4& p = pp[k * B + b];
                adam_step(adam, grad_at(4 * e), lr, p.x, m[b].x, v[b].x);
                adam_step(adam, grad_at(4 * e + 1), lr, p.y, m[b].y, v[b].y);
                adam_step(adam, grad_at(4 * e + 2), lr, p.z, m[b].z, v[b].z);
                adam_step(adam, grad_at(4 * e + 3), lr, p.w, m[b].w, v[b].w);
                P4[e] = p; M4[e] = m[b]; V4[e] = v[b];
            }
        }
    };
#pragma unroll
    for (int k = 0; k < D - 1 && k < NB; k++) load(k, mm[k % D], vv[k % D]);
#pragma unroll
    for (int k = 0; k < NB; k++) {
        if (k + D - 1 < NB) load(k + D - 1, mm[(k + D - 1) % D], vv[(k + D - 1) % D]);
        update(k, mm[k % D], vv[k % D]);
    }
}

// BANDS (the band-limited forms of the fused Adam step, gs_set_sh_degree): of a row of L floats only the columns [0, Lact),
// Lact = 3 ((degree + 1)^2 - 1) < L, are staged, differentiated and updated.  Where the full-row form may use 16-byte accesses
// (L % 4 == 0 and an aligned span in all three arenas) a row's first A4 = ceil(Lact / 4) float4 are moved: item j = lane + 64 i of
// the wave's rows x A4 items is float4 (j % A4) of row (j / A4), so i < A4 and the parameter values stay in A4 <= SH_BAND_MAX4
// registers per lane for the update, as adam_rows_kept keeps them.  A float4 that straddles Lact (L = 72: columns 8..11 at degree
// 1, 44..47 at degree 3) is loaded and stored back whole, its inactive elements as they came -- the rule SPARSE has for a
// straddling float4; a float4 beyond it is neither loaded nor stored.  Other spans go element by element (sh_band_in, adam_band_rows).
// The LDS pitch stays L + 1; nothing reads an LDS column >= Lact (color_backward is given (degree + 1)^2 for K and writes none).
constexpr int SH_BAND_MAX4 = 12;      // K = 25 at degree 3: 48 of 72 columns

__device__ __forceinline__ void sh_band_load4(const float* __restrict__ g, int totalA, int L4, int A4, int lane,
                                              float4 (&regs)[SH_BAND_MAX4])
{
    const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll
    for (int i = 0; i < SH_BAND_MAX4; i++) {
        if (i < A4) {      // (wave-uniform)
            const int j = min(lane + 64 * i, totalA - 1), r = j / A4;
            regs[i] = g4[r * L4 + (j - r * A4)];
        }
    }
}
__device__ __forceinline__ void sh_band_to_lds4(float* __restrict__ lds, int totalA, int L, int A4, int lane,
                                                const float4 (&regs)[SH_BAND_MAX4])
{
#pragma unroll
    for (int i = 0; i < SH_BAND_MAX4; i++) {
        const int j = lane + 64 * i;
        if (i < A4 && j < totalA) {
            const int r = j / A4;
            float* d = lds + r * (L + 1) + 4 * (j - r * A4);
            d[0] = regs[i].x; d[1] = regs[i].y; d[2] = regs[i].z; d[3] = regs[i].w;
        }
    }
}
__device__ __forceinline__ void sh_band_in(float* __restrict__ lds, const float* __restrict__ g, int rows, int L, int Lact, int lane)
{
    const int total = rows * Lact;
    for (int e = lane; e < total; e += 64) {
        const int r = e / Lact, c = e - r * Lact;
        lds[r * (L + 1) + c] = g[r * L + c];
    }
}

// Adam over the active float4 of one wave's rows, parameters from the kept registers; moments in batches of 3 float4
__device__ __forceinline__ void adam_band_rows_kept(const AdamFuse& adam, const float* frest, int row0, int totalA, int L, int Lact,
                                                    int A4, const float* myRows, int lane, float lr, float4 (&pp)[SH_BAND_MAX4])
{
    const size_t off0 = (size_t)(frest - adam.pBase) + (size_t)row0 * L;
    float4* P4 = reinterpret_cast<float4*>(const_cast<float*>(adam.pBase) + off0);
    float4* M4 = reinterpret_cast<float4*>(adam.mBase + off0);
    float4* V4 = reinterpret_cast<float4*>(adam.vBase + off0);
    const int L4 = L >> 2;
    constexpr int B = 3, NB = SH_BAND_MAX4 / B;
    static_assert(NB * B == SH_BAND_MAX4, "whole batches");
    // (a batch of moments in flight ahead of the update, as adam_rows_kept has it, bought nothing here: measured)
#pragma unroll
    for (int k = 0; k < NB; k++) {
        if (k * B < A4) {      // (wave-uniform)
            float4 mm[B], vv[B];
#pragma unroll
            for (int b = 0; b < B; b++) {      // unconditional, clamped: the batch's loads in flight at once
                const int j = min(lane + 64 * (k * B + b), totalA - 1), r = j / A4, e = r * L4 + (j - r * A4);
                mm[b] = M4[e]; vv[b] = V4[e];
            }
#pragma unroll
            for (int b = 0; b < B; b++) {
                const int j = lane + 64 * (k * B + b);
                if (j < totalA) {
                    const int r = j / A4, c4 = j - r * A4, e = r * L4 + c4, c = 4 * c4;
                    const float* g = myRows + r * (L + 1) + c;
                    float4& p = pp[k * B + b];
                    adam_step(adam, g[0], lr, p.x, mm[b].x, vv[b].x);      // (c < Lact: A4 = ceil(Lact / 4))
                    if (c + 1 < Lact) adam_step(adam, g[1], lr, p.y, mm[b].y, vv[b].y);
                    if (c + 2 < Lact) adam_step(adam, g[2], lr, p.z, mm[b].z, vv[b].z);
                    if (c + 3 < Lact) adam_step(adam, g[3], lr, p.w, mm[b].w, vv[b].w);
                    P4[e] = p; M4[e] = mm[b]; V4[e] = vv[b];
                }
            }
        }
    }
}
// ... element by element (L % 4 != 0, or a span that is not 16-byte aligned), four elements' loads in flight at once
__device__ __forceinline__ void adam_band_rows(const AdamFuse& adam, const float* frest, int row0, int rows, int L, int Lact,
                                               const float* myRows, int lane, float lr)
{
    const size_t off0 = (size_t)(frest - adam.pBase) + (size_t)row0 * L;
    float* P = const_cast<float*>(adam.pBase) + off0;
    float* M = adam.mBase + off0;
    float* V = adam.vBase + off0;
    const int total = rows * Lact;
    constexpr int B = 4;
    for (int e0 = lane; e0 < total; e0 += 64 * B) {
        float pp[B], mm[B], vv[B];
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int e = min(e0 + 64 * b, total - 1), r = e / Lact, o = r * L + (e - r * Lact);
            pp[b] = P[o]; mm[b] = M[o]; vv[b] = V[o];
        }
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int e = e0 + 64 * b;
            if (e < total) {
                const int r = e / Lact, c = e - r * Lact, o = r * L + c;
                adam_step(adam, myRows[r * (L + 1) + c], lr, pp[b], mm[b], vv[b]);
                P[o] = pp[b]; M[o] = mm[b]; V[o] = vv[b];
            }
        }
    }
}

// A cotangent row that is not finite.  The blend backward gates a pixel's contribution to a splat branch-free (alpha and its
// gradient times 0 past the pixel's nContrib or under the 0.99 clamp), which is exact while the splat's weight exp(-q/2) is finite.
// A conic that is not positive definite -- float32 cancellation in the determinant of a needle tens of thousands of pixels long:
// the soak's Gaussian of scales (8.2, 0.007, 0.006), cov2d = (4.2e7, -3.8e7; -3.8e7, 3.5e7) -- has q < 0 without bound, the weight
// overflows and 0 x inf = NaN lands in the accumulator row of THAT splat (no other row, no pixel state: the NaN never enters T or
// the owed colour).  The reference's loop does not evaluate a pixel past its nContrib at all.  Such a row is dropped whole -- a zero
// gradient for this Gaussian in this step -- instead of poisoning its parameters and moments for good (one Gaussian of a million
// after ~8500 iterations of tools/soak.py, on the reference's lists and on trimmed rects alike).
__device__ __forceinline__ void drop_nonfinite_row(float4& g0, float4& g1, float4& g2)
{
#ifdef GS_KEEP_NONFINITE_ROWS      // (experiment build: the behaviour before the fix, to see that the test would have caught it)
    return;
#endif
    auto fin = [](float v) { return (v - v) == 0.0f; };
    if (!(fin(g0.x) && fin(g0.y) && fin(g0.z) && fin(g0.w) && fin(g1.x) && fin(g1.y) && fin(g1.z) && fin(g1.w) && fin(g2.x) &&
          fin(g2.y) && fin(g2.z))) {
        g0 = make_float4(0.f, 0.f, 0.f, 0.f); g1 = g0; g2 = g0;
    }
}

// A deterministic wave64 sum (butterfly, the same order on every run): every lane ends with the total.
__device__ __forceinline__ float wave_sum_xor(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// POSE: besides its own gradients the kernel writes the wave's share of dL/dV' (12 floats [3 k + a], project_geometry_bwd<true>)
// and of dL/dcam_center' (3 floats: minus the colour path's d) to posePartials[16 w .. 16 w + 14] (16 w + 15: 0), w the wave's index;
// pose_grad_kernel sums them.  A row with an all-zero cotangent contributes exactly 0 (as its own gradients do).
// AA (anti-aliased mode, gs_set_antialiasing): the forward blended sigma(o) rho; dop is the cotangent of that product, so
// dL/do_raw = dop rho sigma (1 - sigma) and the covariance cotangent gains the VJP of rho (project_geometry_bwd<., true>).
// MCMC (the MCMC strategy's per-step part, gs_set_mcmc; MODE 2 only): the regularisers' gradients join the opacity and scale
// gradients in front of adam_step, and the position noise (gs_mcmc.h mcmc_noise) of the updated parameters joins the
// updated xyz in front of the stores.
// F3D (3-D smoothing filter, gs_set_filter3d; MODE 0 and 2, never with MCMC): the forward projected s_eff = sqrt(s^2 + f^2) and
// blended sigma(o) kappa (rho); the geometry backward runs on s_eff, dop's share of the opacity and of the rho VJP carries kappa,
// and filter3d_activate (gs_math.h) turns dL/ds_eff into dL/dscales_raw.
// SPARSE (sparse Adam, gs_set_sparse_adam; MODE 2 only, never with MCMC or F3D): visMask[p] = the forward gave Gaussian p a radius
// > 0.  A wave whose 64 rows are all invisible returns before it has staged, loaded or stored anything (under POSE it writes
// its zero partials); in a mixed wave the invisible lanes store none of their 14 small elements and adam_rows / adam_rows_kept
// skip their rows.  An invisible row's cotangent is all zero, so it adds nothing to gradNormAccum or to the pose sums either way.
// FISHEYE (the equidistant camera model, gs_set_camera_model; never with POSE or F3D): project_geometry_bwd's FISHEYE.
// BANDS (an active degree below the one K allows, gs_set_sh_degree; MODE 2 only, never with POSE, MCMC, F3D or SPARSE): the f_rest
// columns >= 3 ((degree + 1)^2 - 1) are not staged, not written in LDS and not updated (sh_band_load4 .. adam_band_rows above); at
// degree 0 the kernel touches no f_rest byte and no LDS.  Everything else is the plain MODE 2 form's arithmetic in its order.
template <int MODE, bool POSE, bool AA = false, bool MCMC = false, bool F3D = false, bool SPARSE = false, bool FISHEYE = false,
          bool BANDS = false>
__device__ __forceinline__ void proj_bwd_fused_body(
    int N, int K, int degree, const CamParams& cam, const float* xyz, const float* fdc,
    const float* frest, const float* scalesRaw, const float* rotRaw,
    const float* opacityRaw, const float* __restrict__ gradAcc16, float* gXyz,
    float* gFdc, float* gFrest, float* gScales, float* gRot,
    float* gOpacity, float* __restrict__ gradNormAccum, AdamFuse adam, float* __restrict__ posePartials,
    McmcFuse mc = McmcFuse{}, const float* __restrict__ filter3d = nullptr, const unsigned char* __restrict__ visMask = nullptr)
{
    constexpr bool EMIT_MG = MODE == 1, ADAM = MODE == 2;
    extern __shared__ float shLds[];
    // no update from a forward that did not render (gs_ctx.h adamGate).  The word is requested here and looked at only
    // in front of the first store: a branch on it up here put a dependent scalar-load latency in front of every
    // block's loads (2 M Gaussians: 0.77 -> 0.88 ms)
    const uint32_t gateWord = ADAM ? *adam.gate : 0u;
    const int p = blockIdx.x * PROJ_FUSED_THREADS + threadIdx.x;
    if (MODE == 0 && adam.rider && p == 0) *adam.rider = *adam.ovf ? 1.0f : 0.0f;      // (data-parallel all-reduce: the gate rides behind the gradients)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool myVis = true;
    unsigned long long visBits = ~0ull;
    if constexpr (SPARSE) {
        myVis = p < N && visMask[p] != 0;
        visBits = __ballot(myVis);
        if (visBits == 0ull) {       // (wave-uniform; the kernel has no workgroup barrier)
            if constexpr (POSE) {
                if (lane < 16) posePartials[16 * ((size_t)blockIdx.x * (PROJ_FUSED_THREADS / 64) + wv) + lane] = 0.f;
            }
            return;
        }
    }
    const int L = (K - 1) * 3;
    float* myRows = shLds + wv * 64 * (L + 1);
    const int row0 = blockIdx.x * PROJ_FUSED_THREADS + wv * 64;
    const int rows = min(64, N - row0);
    // fused Adam: the wave's f_rest span stays in registers for the update at the bottom (adam_rows_kept) when it is
    // float4-addressable in all three arenas and fits the 18 registers (K <= 25)
    float4 keptRows[SH_ROWS_MAX4];
    const int total4 = (rows * L) >> 2;
    bool kept = ADAM && rows > 0 && L > 0 && (L & 3) == 0 && total4 <= 64 * SH_ROWS_MAX4 &&
                (((size_t)(frest - adam.pBase) + (size_t)row0 * L) & 3) == 0;
    // BANDS: the active columns alone; `kept` = the span takes 16-byte accesses and its active float4 fit the registers
    const int Kact = (degree + 1) * (degree + 1), Lact = 3 * (Kact - 1), A4 = (Lact + 3) >> 2, totalA = rows * A4;
    float4 bandRows[BANDS ? SH_BAND_MAX4 : 1];
    if constexpr (BANDS) {
        kept = kept && A4 <= SH_BAND_MAX4;
        if (rows > 0 && Lact > 0) {
            if (kept) {
                sh_band_load4(frest + (size_t)row0 * L, totalA, L >> 2, A4, lane, bandRows);
                sh_band_to_lds4(myRows, totalA, L, A4, lane, bandRows);
            } else sh_band_in(myRows, frest + (size_t)row0 * L, rows, L, Lact, lane);
        }
    } else
    if (kept) {
        sh_rows_load4(frest + (size_t)row0 * L, total4, 0, lane, keptRows);
        sh_rows_to_lds4(myRows, total4, L, 0, lane, keptRows);
    } else if (rows > 0 && L > 0) sh_rows_in(myRows, frest + (size_t)row0 * L, rows, L, lane);
    float pose[POSE ? 15 : 1];
    if constexpr (POSE) {
#pragma unroll
        for (int j = 0; j < 15; j++) pose[j] = 0.f;
    }
    if (p < N) {
    const float4* ga = reinterpret_cast<const float4*>(gradAcc16 + (size_t)p * 16);
    float4 g0 = ga[0], g1 = ga[1], g2 = ga[2];
    drop_nonfinite_row(g0, g1, g2);
    const float cm[2] = {g0.x, g0.y};
    // row: dmx dmy dc00 dc01 | dc10 dc11 dr dg | db dop ddepth
    const float ccon[4] = {g0.z, g0.w, g1.x, g1.y};
    const float ccol[3] = {g1.z, g1.w, g2.x};
    const float cotOpacity = g2.y, cotDepth = g2.z;
    const float ccov[4] = {0.f, 0.f, 0.f, 0.f};   // cov2d is unused downstream (GaussianRenderer.swift:796-802)

    const float m[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
    const float sr[3] = {scalesRaw[3 * p], scalesRaw[3 * p + 1], scalesRaw[3 * p + 2]};
    const float s[3] = {expf(sr[0]), expf(sr[1]), expf(sr[2])};
    const float rr[4] = {rotRaw[4 * p], rotRaw[4 * p + 1], rotRaw[4 * p + 2], rotRaw[4 * p + 3]};
    const float n2 = rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3];
    const float nrm = sqrtf(n2);
    const float den = nrm + 1e-8f;
    const float q[4] = {rr[0] / den, rr[1] / den, rr[2] / den, rr[3] / den};

    GeomGrads g;
    float aaRho = 1.0f;
    const float aaSg = AA ? 1.0f / (1.0f + expf(-opacityRaw[p])) : 0.0f;
    float f3dF = 0.0f, f3dKappa = 1.0f, se[3];
    if constexpr (F3D) {
        f3dF = filter3d[p];
        f3dKappa = filter3d_activate(s, f3dF, se);
        project_geometry_bwd<POSE, AA>(m, se, q, cam, cm, cotDepth, ccov, ccon, g, POSE ? pose : nullptr, cotOpacity * aaSg * f3dKappa,
                                       &aaRho);
    } else
    project_geometry_bwd<POSE, AA, FISHEYE>(m, s, q, cam, cm, cotDepth, ccov, ccon, g, POSE ? pose : nullptr, cotOpacity * aaSg, &aaRho);
    // A Gaussian no pixel blended (not visible, or off every tile) arrives with an all-zero cotangent row and its
    // gradient is exactly zero.  The reference's arithmetic evaluates J^T 0 term by term, which is 0 * inf = NaN when
    // the point sits within ~1e-3 of the camera plane (1 / t_z^2 overflows); one such NaN poisons Adam for good.
    // The fused path returns the exact value instead (the op-level gs_projection_backward keeps the 1:1 arithmetic).
    if (g0.x == 0.f && g0.y == 0.f && g0.z == 0.f && g0.w == 0.f && g1.x == 0.f && g1.y == 0.f && g1.z == 0.f &&
        g1.w == 0.f && g2.x == 0.f && g2.y == 0.f && g2.z == 0.f) {
#pragma unroll
        for (int a = 0; a < 3; a++) { g.dm[a] = 0.f; g.ds[a] = 0.f; }
#pragma unroll
        for (int a = 0; a < 4; a++) g.dq[a] = 0.f;
        if constexpr (POSE) {
#pragma unroll
            for (int j = 0; j < 12; j++) pose[j] = 0.f;
        }
    }

    const float x = m[0] - cam.cam[0], y = m[1] - cam.cam[1], z = m[2] - cam.cam[2];
    const float* d0 = fdc + (size_t)p * 3;
    float* rest = myRows + lane * (L + 1);     // coefficients in, gradients out, in place (own row only)
    float* gd0 = gFdc + (size_t)p * 3;
    float d[3];
    const float opr = opacityRaw[p];
    // fused Adam: arena offsets of this Gaussian's 14 small elements, their moments loaded now (independent loads,
    // in flight under the arithmetic below) -- gradients sg_, values from the registers that already hold them
    float sm_[14], sv_[14], sg_[14], d0v[3] = {0.f, 0.f, 0.f};
    // (the offsets are rebuilt in front of the stores rather than kept: 28 registers of a kernel at its 256)
    auto small_off = [&](int i) -> size_t {
        const float* ptr[14] = {xyz + 3 * p, xyz + 3 * p + 1, xyz + 3 * p + 2, scalesRaw + 3 * p, scalesRaw + 3 * p + 1,
                                scalesRaw + 3 * p + 2, rotRaw + 4 * p, rotRaw + 4 * p + 1, rotRaw + 4 * p + 2,
                                rotRaw + 4 * p + 3, opacityRaw + p, d0, d0 + 1, d0 + 2};
        return (size_t)(ptr[i] - adam.pBase);
    };
    if (ADAM) { d0v[0] = d0[0]; d0v[1] = d0[1]; d0v[2] = d0[2]; }
    // one 12- or 16-byte access per tensor and lane instead of one per element: the 14 elements' moments in and their
    // parameters and moments out were 70 four-byte memory instructions per lane, 12 % of the kernel's bytes for 19 % of
    // its time (a build without them: 0.138 -> 0.112 ms); 4-byte aligned is all the arena promises for [N,3] tensors
    struct __attribute__((packed, aligned(4))) V3 { float x, y, z; };
    struct __attribute__((packed, aligned(4))) V4 { float x, y, z, w; };
    auto small_moments = [&]() {
        auto in3 = [&](const float* base, int i0) {
            const size_t o = small_off(i0);
            const V3 a = *reinterpret_cast<const V3*>(adam.mBase + o), b = *reinterpret_cast<const V3*>(adam.vBase + o);
            sm_[i0] = a.x; sm_[i0 + 1] = a.y; sm_[i0 + 2] = a.z; sv_[i0] = b.x; sv_[i0 + 1] = b.y; sv_[i0 + 2] = b.z;
            (void)base;
        };
        in3(xyz, 0); in3(scalesRaw, 3); in3(fdc, 11);
        {
            const size_t o = small_off(6);
            const V4 a = *reinterpret_cast<const V4*>(adam.mBase + o), b = *reinterpret_cast<const V4*>(adam.vBase + o);
            sm_[6] = a.x; sm_[7] = a.y; sm_[8] = a.z; sm_[9] = a.w; sv_[6] = b.x; sv_[7] = b.y; sv_[8] = b.z; sv_[9] = b.w;
        }
        { const size_t o = small_off(10); sm_[10] = adam.mBase[o]; sv_[10] = adam.vBase[o]; }
    };
    if (ADAM && !GS_PROJ_LATE_MOMENTS) small_moments();
    if (EMIT_MG)      // no SH gradient is written; gFdc, when given, receives the [N,3] gated colour cotangent
        color_backward(degree, K, x, y, z, ccol,
                       [&](int k, int ch) { return k == 0 ? d0[ch] : rest[(k - 1) * 3 + ch]; },
                       [&](int, int, float) {}, d, gFdc ? gd0 : nullptr);
    else {
        float gdc[3] = {0.f, 0.f, 0.f};          // the DC gradient stays in registers for the fused Adam step
        color_backward(degree, BANDS ? Kact : K, x, y, z, ccol,
                       [&](int k, int ch) { return k == 0 ? d0[ch] : rest[(k - 1) * 3 + ch]; },
                       [&](int k, int ch, float v) {
                           if (k == 0) { if (ADAM) gdc[ch] = v; else gd0[ch] = v; }
                           else rest[(k - 1) * 3 + ch] = v;
                       }, d);
        if (ADAM) { sg_[11] = gdc[0]; sg_[12] = gdc[1]; sg_[13] = gdc[2]; }
    }
    if (ADAM && GS_PROJ_LATE_MOMENTS) small_moments();      // (SPARSE: an invisible lane of a mixed wave loads them too and stores nothing)
    if constexpr (POSE) {
        // xyz - cam' is the SH view direction's argument: dL/dcam' = -d (a zero row has d = 0 up to 0 x inf: selected away)
        const bool live = (g0.x != 0.f || g0.y != 0.f || g0.z != 0.f || g0.w != 0.f || g1.x != 0.f ||
                                                 g1.y != 0.f || g1.z != 0.f || g1.w != 0.f || g2.x != 0.f || g2.y != 0.f ||
                                                 g2.z != 0.f);
        pose[12] = live ? -d[0] : 0.f; pose[13] = live ? -d[1] : 0.f; pose[14] = live ? -d[2] : 0.f;
        // a row whose pose share is not finite (a point at the camera plane) is dropped from the view's sum, as
        // drop_nonfinite_row drops a cotangent row: one Gaussian must not poison the view's correction and its moments
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 15; j++) fin = fin && (pose[j] - pose[j]) == 0.0f;
        if (!fin) {
#pragma unroll
            for (int j = 0; j < 15; j++) pose[j] = 0.f;
        }
    }
    const float gx = g.dm[0] + d[0], gy = g.dm[1] + d[1], gz = g.dm[2] + d[2];
    if (ADAM) { sg_[0] = gx; sg_[1] = gy; sg_[2] = gz; }
    else { gXyz[3 * p] = gx; gXyz[3 * p + 1] = gy; gXyz[3 * p + 2] = gz; }
    if (gradNormAccum && !gateWord) gradNormAccum[p] += sqrtf(gx * gx + gy * gy + gz * gz);   // accum_grad_norm (densify.hip), fused
    if constexpr (F3D) {       // dL/dscales_raw through s_eff and through kappa (an all-zero row: g.ds = 0 and cotOpacity = 0)
        const float sgF = 1.0f / (1.0f + expf(-opr));
        filter3d_activate<true>(s, f3dF, se, g.ds, cotOpacity * sgF * (AA ? aaRho : 1.0f) * f3dKappa);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float v = F3D ? g.ds[a] : g.ds[a] * s[a];          // d exp
        if (ADAM) sg_[3 + a] = v; else gScales[3 * p + a] = v;
    }
    // rotation normalisation VJP: y = q / (|q| + 1e-8)
    const float dot = g.dq[0] * rr[0] + g.dq[1] * rr[1] + g.dq[2] * rr[2] + g.dq[3] * rr[3];
    const float dn = -dot / (den * den);
    const float dn2 = dn * 0.5f / nrm;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const float v = g.dq[a] / den + 2.0f * rr[a] * dn2;
        if (ADAM) sg_[6 + a] = v; else gRot[4 * p + a] = v;
    }
    const float sg = 1.0f / (1.0f + expf(-opr));
    const float gop = (F3D ? (AA ? cotOpacity * f3dKappa * aaRho : cotOpacity * f3dKappa) : AA ? cotOpacity * aaRho : cotOpacity) * sg * (1.0f - sg);
    if (ADAM) sg_[10] = gop; else gOpacity[p] = gop;
    if constexpr (MCMC) {      // + the gradients of opacity_reg mean(sigma(o)) and scale_reg mean(exp(s)) (mcmc_reg_kernel's sums)
        sg_[10] = sg_[10] + mc.oCoef * mcmc_sigmoid_slope(opr);
#pragma unroll
        for (int a = 0; a < 3; a++) sg_[3 + a] = sg_[3 + a] + mc.sCoef * s[a];
    }
    bool smallOn = ADAM && !gateWord;
    if constexpr (SPARSE) smallOn = smallOn && myVis;
    if (smallOn) {
        // the 14 small elements: values and moments were loaded at the top; one burst of stores here
        float sp[14] = {m[0], m[1], m[2], sr[0], sr[1], sr[2], rr[0], rr[1], rr[2], rr[3], opr, d0v[0], d0v[1], d0v[2]};
        const float slr[14] = {adam.lr[0], adam.lr[0], adam.lr[0], adam.lr[3], adam.lr[3], adam.lr[3], adam.lr[4],
                               adam.lr[4], adam.lr[4], adam.lr[4], adam.lr[5], adam.lr[1], adam.lr[1], adam.lr[1]};
#pragma unroll
        for (int i = 0; i < 14; i++) adam_step(adam, sg_[i], slr[i], sp[i], sm_[i], sv_[i]);
        if constexpr (MCMC) {
            float dn[3];
            mcmc_noise(mc, (uint32_t)p, sp + 3, sp + 6, sp[10], dn);
            sp[0] = sp[0] + dn[0]; sp[1] = sp[1] + dn[1]; sp[2] = sp[2] + dn[2];
        }
        float* pB = const_cast<float*>(adam.pBase);
        auto out3 = [&](int i0) {
            const size_t o = small_off(i0);
            *reinterpret_cast<V3*>(pB + o) = V3{sp[i0], sp[i0 + 1], sp[i0 + 2]};
            *reinterpret_cast<V3*>(adam.mBase + o) = V3{sm_[i0], sm_[i0 + 1], sm_[i0 + 2]};
            *reinterpret_cast<V3*>(adam.vBase + o) = V3{sv_[i0], sv_[i0 + 1], sv_[i0 + 2]};
        };
        out3(0); out3(3); out3(11);
        {
            const size_t o = small_off(6);
            *reinterpret_cast<V4*>(pB + o) = V4{sp[6], sp[7], sp[8], sp[9]};
            *reinterpret_cast<V4*>(adam.mBase + o) = V4{sm_[6], sm_[7], sm_[8], sm_[9]};
            *reinterpret_cast<V4*>(adam.vBase + o) = V4{sv_[6], sv_[7], sv_[8], sv_[9]};
        }
        { const size_t o = small_off(10); pB[o] = sp[10]; adam.mBase[o] = sm_[10]; adam.vBase[o] = sv_[10]; }
    }
    }
    if (MODE == 0 && rows > 0 && L > 0) sh_rows_out(myRows, gFrest + (size_t)row0 * L, rows, L, lane);
    if constexpr (BANDS) {
        if (!gateWord && rows > 0 && Lact > 0) {
            if (kept) adam_band_rows_kept(adam, frest, row0, totalA, L, Lact, A4, myRows, lane, adam.lr[2], bandRows);
            else adam_band_rows(adam, frest, row0, rows, L, Lact, myRows, lane, adam.lr[2]);
        }
    } else
    if (ADAM && !gateWord && rows > 0 && L > 0) {
        if (kept) adam_rows_kept<SPARSE>(adam, frest, row0, total4, L, myRows, lane, adam.lr[2], keptRows, visBits);
        else adam_rows<SPARSE>(adam, frest, row0, rows, L, myRows, lane, adam.lr[2], visBits);
    }
    if constexpr (POSE) {
        float* out = posePartials + 16 * ((size_t)blockIdx.x * (PROJ_FUSED_THREADS / 64) + wv);
#pragma unroll
        for (int j = 0; j < 15; j++) {
            const float t = wave_sum_xor(pose[j]);
            if (lane == j) out[j] = t;
        }
        if (lane == 15) out[15] = 0.f;
    }
}

// The forms that exist: MODE 2 {plain, F3D, MCMC, SPARSE} x POSE x AA, MODE 0 {plain, F3D} x POSE x AA, MODE 1 plain x AA (26);
// fisheye: MODE 2 {plain, MCMC, SPARSE} x AA, MODE 0 plain x AA (8); band-limited: MODE 2 plain x AA x {pinhole, fisheye} (4)
constexpr bool proj_bwd_form_exists(int MODE, bool POSE, bool MCMC, bool F3D, bool SPARSE, bool FISHEYE = false, bool BANDS = false)
{
    return (MODE == 0 || MODE == 1 || MODE == 2) &&
           (!BANDS || (MODE == 2 && !POSE && !MCMC && !F3D && !SPARSE)) &&      // band-limited: the plain fused Adam form only
           (!FISHEYE || (!POSE && !F3D && MODE != 1)) &&    // the fisheye model: no pose refinement, no 3-D filter, no data-parallel form
           (!POSE || MODE != 1) &&                          // no pose refinement in the data-parallel form
           (!MCMC || MODE == 2) &&                          // the MCMC step is fused into the Adam form only
           (!SPARSE || (MODE == 2 && !MCMC && !F3D)) &&     // sparse Adam: the plain fused Adam form only
           (!F3D || (!MCMC && MODE != 1));                  // the 3-D filter: single-device steps and the reference strategy only
}

// The arguments of every form.  A form reads the fields its template flags name and no others, so the unused ones cost the default
// forms nothing: every instantiation has the VGPRs, scratch and occupancy of the per-feature kernel it replaced (the four MODE 0 POSE
// forms one VGPR fewer), measured and timed in DESIGN.md section 21.  dcam stands last so that the fields in front of it keep the
// kernel-argument offsets they had.
struct ProjBwdArgs {
    int N, K, degree;
    CamParams cam;               // the host camera; POSE reads *dcam instead
    const float *xyz, *fdc, *frest, *scalesRaw, *rotRaw, *opacityRaw, *gradAcc16;
    float *gXyz, *gFdc, *gFrest, *gScales, *gRot, *gOpacity;      // MODE 0 / 1 (MODE 1: gFdc receives mg[N,3]); MODE 2: unused
    float* gradNormAccum;
    AdamFuse adam;
    float* posePartials;           // POSE
    McmcFuse mc;                   // MCMC
    const float* filter3d;         // F3D
    const unsigned char* visMask;  // SPARSE
    const CamParams* dcam;         // POSE: the camera pose_camera_kernel composed on the device
};

template <int MODE, bool POSE, bool AA, bool MCMC, bool F3D, bool SPARSE, bool FISHEYE = false, bool BANDS = false>
__global__ __launch_bounds__(PROJ_FUSED_THREADS) void proj_bwd_fused_kernel(ProjBwdArgs a)
{
    static_assert(proj_bwd_form_exists(MODE, POSE, MCMC, F3D, SPARSE, FISHEYE, BANDS), "no such form of the fused projection backward");
    CamParams posed;
    if constexpr (POSE) posed = *a.dcam;
    proj_bwd_fused_body<MODE, POSE, AA, MCMC, F3D, SPARSE, FISHEYE, BANDS>(a.N, a.K, a.degree, POSE ? posed : a.cam, a.xyz, a.fdc, a.frest, a.scalesRaw,
                                                           a.rotRaw, a.opacityRaw, a.gradAcc16, a.gXyz, a.gFdc, a.gFrest, a.gScales,
                                                           a.gRot, a.gOpacity, a.gradNormAccum, a.adam, a.posePartials, a.mc, a.filter3d,
                                                           a.visMask);
}

// what the fused forward leaves for the SPARSE forms: radius > 0 of every Gaussian, as a byte (gs_get_visibility reads the same)
__global__ __launch_bounds__(256) void vis_mask_kernel(int N, const float* __restrict__ radii, unsigned char* __restrict__ mask)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < N) mask[p] = radii[p] > 0.0f ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// data-parallel: the gated colour cotangent straight from the blend backward's accumulator (columns dr dg db of
// gradAcc16) and the gate bits the forward left in packed12 -- ready before the projection backward runs, so its
// all-gather overlaps with that kernel
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void color_cot_kernel(int N, const float* __restrict__ gradAcc16,
                                                        const float* __restrict__ packed12, float* __restrict__ out,
                                                        const uint32_t* __restrict__ ovf, float* __restrict__ rider)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && rider) *rider = *ovf ? 1.0f : 0.0f;      // this rank's word of the step's gate, gathered with the cotangents
    if (p >= N) return;
    const float* ga = gradAcc16 + (size_t)p * 16;
    const uint32_t gate = __float_as_uint(packed12[(size_t)p * 12 + 11]);
    float4 r0 = *reinterpret_cast<const float4*>(ga), r1 = *reinterpret_cast<const float4*>(ga + 4), r2 = *reinterpret_cast<const float4*>(ga + 8);
    drop_nonfinite_row(r0, r1, r2);        // (a row the blend backward left non-finite is dropped whole: proj_bwd_fused_kernel)
    const float col[3] = {r1.z, r1.w, r2.x};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t side = (gate >> (2 * ch)) & 3u;
        const float g = col[ch];
        out[(size_t)p * 3 + ch] = side == 2u ? g : (side == 1u ? 0.5f * g : 0.0f);      // d max(a, 0): tie -> 1/2
    }
}

// ---------------------------------------------------------------------------------------------
// data-parallel SH gradient: grad_shs[k] = sum over views r of basis_k(xyz - cam_r) * mg_r
// ---------------------------------------------------------------------------------------------
struct ViewCenters {
    float c[16][3];
    int n;
};

// ADAM: instead of writing the summed SH gradients, apply their Adam step to features_dc / features_rest in place
// (fdcParam / frestParam inside the parameter arena adam.pBase; lr[1], lr[2]; gscale = 1 / world).
template <bool ADAM>
__global__ __launch_bounds__(PROJ_FUSED_THREADS) void sh_grad_from_views_kernel(
    int N, int K, int degree, ViewCenters views, const float* __restrict__ xyz, const float* __restrict__ mgAll,
    long long mgStride, float* gFdc, float* gFrest, const float* fdcParam, const float* frestParam, AdamFuse adam)
{
    extern __shared__ float shLds[];
    // (looked at in front of the first store, proj_bwd_fused_kernel.)  With gathered words (round 5) this kernel is the
    // first to know the step's gate: it ORs the ranks' words for itself and leaves the result for the kernels behind it
    const uint32_t gateWord = (ADAM || adam.gwWords) ? adam_gate_word(adam) : 0u;
    adam_gate_publish(adam, gateWord);
    const int p = blockIdx.x * PROJ_FUSED_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = (K - 1) * 3;
    float* rest = shLds + wv * 64 * (L + 1) + lane * (L + 1);
    const int row0 = blockIdx.x * PROJ_FUSED_THREADS + wv * 64;
    const int rows = min(64, N - row0);
    if (p < N) {
        for (int i = 0; i < L; i++) rest[i] = 0.0f;
        float dc[3] = {0.f, 0.f, 0.f};
        const float m0 = xyz[3 * p], m1 = xyz[3 * p + 1], m2 = xyz[3 * p + 2];
        for (int r = 0; r < views.n; r++) {
            const float* mg = mgAll + (size_t)r * (size_t)mgStride + (size_t)p * 3;
            const float g0 = mg[0], g1 = mg[1], g2 = mg[2];
            if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) continue;
            sh_foreach(degree, m0 - views.c[r][0], m1 - views.c[r][1], m2 - views.c[r][2],
                       [&](int k, float b, float, float, float) {
                           if (k == 0) { dc[0] += b * g0; dc[1] += b * g1; dc[2] += b * g2; }
                           else { rest[(k - 1) * 3] += b * g0; rest[(k - 1) * 3 + 1] += b * g1; rest[(k - 1) * 3 + 2] += b * g2; }
                       });
        }
        if (ADAM && gateWord) {
            // the step's forward overflowed on some rank: no update
        } else if (ADAM) {
            const size_t off = (size_t)(fdcParam - adam.pBase) + 3 * (size_t)p;
            float pv[3], mv[3], vv[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) { pv[ch] = adam.pBase[off + ch]; mv[ch] = adam.mBase[off + ch]; vv[ch] = adam.vBase[off + ch]; }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) adam_step(adam, dc[ch], adam.lr[1], pv[ch], mv[ch], vv[ch]);
            // (one 12-byte store per arena instead of three 4-byte ones: proj_bwd_fused_kernel, small_moments)
            struct __attribute__((packed, aligned(4))) V3 { float x, y, z; };
            *reinterpret_cast<V3*>(const_cast<float*>(adam.pBase) + off) = V3{pv[0], pv[1], pv[2]};
            *reinterpret_cast<V3*>(adam.mBase + off) = V3{mv[0], mv[1], mv[2]};
            *reinterpret_cast<V3*>(adam.vBase + off) = V3{vv[0], vv[1], vv[2]};
        } else {
            gFdc[3 * p] = dc[0]; gFdc[3 * p + 1] = dc[1]; gFdc[3 * p + 2] = dc[2];
        }
    }
    if (rows > 0 && L > 0) {
        if (ADAM) { if (!gateWord) adam_rows(adam, frestParam, row0, rows, L, shLds + wv * 64 * (L + 1), lane, adam.lr[2]); }
        else sh_rows_out(shLds + wv * 64 * (L + 1), gFrest + (size_t)row0 * L, rows, L, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// data-parallel step, round 6: the SH rows are read ONCE per step.
//
// Rounds 2-5 split the fused projection backward + Adam of the single-device step into proj_bwd_fused_kernel<1> (the four
// geometry gradients; it staged every Gaussian's 288 B of SH rows through LDS only for the view-direction term of the xyz
// gradient, d_r = sum_k grad basis_k(xyz - cam_r) (SH_k . cc_r)) and sh_grad_from_views_kernel<true> (the SH gradients rebuilt
// from the gathered colour cotangents + their Adam step, which reads the same rows again): 46 + 93 us on one rank against 128
// for the fused kernel.  But d_r is, like the SH gradient itself, a function of replicated values (xyz, SH, camera centre)
// and of the view's gathered colour cotangent alone: every rank can rebuild sum_r d_r while it has the SH rows in hand
// for their Adam step.  So:
//   proj_bwd_geom_kernel       geometry only (56 + 64 B in, 44 + 12 B out per Gaussian; no LDS, no SH rows): the xyz gradient
//                              WITHOUT the view-direction term goes to the gradient arena (the all-reduce sums it) and, a
//                              copy, to xyzOwn -- the densify statistic needs this view's FULL xyz gradient;
//   sh_views_dir_adam_kernel   rows to registers + LDS once; pass 1 over the views: d_r from the OLD coefficients, their sum
//                              to xyzAdd, |xyzOwn_r + d_r| of this rank's own view(s) into the densify statistic; pass 2: the SH
//                              gradients into the same LDS rows; Adam from the kept registers (adam_rows_kept);
//   adam_kernel                the geometry slice after the all-reduce, gradient = reduced + xyzAdd on the xyz segment.
// Sum over views of (geometry_r + d_r) becomes (sum geometry_r) + (sum d_r): the same value up to float association.
// ---------------------------------------------------------------------------------------------
struct ViewCentersOwn {
    float c[16][3];
    const float* own[16];      // xyzOwn of the views THIS rank rendered (their full xyz gradient = own + d_r), else nullptr
    int n;
};

template <bool AA>       // (the anti-aliased mode: proj_bwd_fused_body's AA)
__global__ __launch_bounds__(256) void proj_bwd_geom_kernel(
    int N, CamParams cam, const float* __restrict__ xyz, const float* __restrict__ scalesRaw, const float* __restrict__ rotRaw,
    const float* __restrict__ opacityRaw, const float* __restrict__ gradAcc16, float* __restrict__ gXyz,
    float* __restrict__ gScales, float* __restrict__ gRot, float* __restrict__ gOpacity, float* __restrict__ xyzOwn,
    const float* __restrict__ packed12, float* __restrict__ ccOut, const uint32_t* __restrict__ ovf, float* __restrict__ rider)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    // ccOut != nullptr: color_cot_kernel's work rides here (the gated colour cotangents + this rank's word of the step's gate):
    // with the SH rows gone this kernel is ~10 us, too short for the all-gather to hide under -- one launch and one fork less
    if (ccOut && p == 0 && rider) *rider = *ovf ? 1.0f : 0.0f;
    if (p >= N) return;
    const float4* ga = reinterpret_cast<const float4*>(gradAcc16 + (size_t)p * 16);
    float4 g0 = ga[0], g1 = ga[1], g2 = ga[2];
    drop_nonfinite_row(g0, g1, g2);
    if (ccOut) {
        const uint32_t gate = __float_as_uint(packed12[(size_t)p * 12 + 11]);
        const float col[3] = {g1.z, g1.w, g2.x};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t side = (gate >> (2 * ch)) & 3u;
            ccOut[(size_t)p * 3 + ch] = side == 2u ? col[ch] : (side == 1u ? 0.5f * col[ch] : 0.0f);      // d max(a, 0): tie -> 1/2
        }
    }
    // row: dmx dmy dc00 dc01 | dc10 dc11 dr dg | db dop ddepth
    const float cm[2] = {g0.x, g0.y};
    const float ccon[4] = {g0.z, g0.w, g1.x, g1.y};
    const float cotOpacity = g2.y, cotDepth = g2.z;
    const float ccov[4] = {0.f, 0.f, 0.f, 0.f};   // cov2d is unused downstream (GaussianRenderer.swift:796-802)
    const float m[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
    const float sr[3] = {scalesRaw[3 * p], scalesRaw[3 * p + 1], scalesRaw[3 * p + 2]};
    const float s[3] = {expf(sr[0]), expf(sr[1]), expf(sr[2])};
    const float rr[4] = {rotRaw[4 * p], rotRaw[4 * p + 1], rotRaw[4 * p + 2], rotRaw[4 * p + 3]};
    const float n2 = rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3];
    const float nrm = sqrtf(n2);
    const float den = nrm + 1e-8f;
    const float q[4] = {rr[0] / den, rr[1] / den, rr[2] / den, rr[3] / den};
    GeomGrads g;
    float aaRho = 1.0f;
    const float aaSg = AA ? 1.0f / (1.0f + expf(-opacityRaw[p])) : 0.0f;
    project_geometry_bwd<false, AA>(m, s, q, cam, cm, cotDepth, ccov, ccon, g, nullptr, cotOpacity * aaSg, &aaRho);
    // (a Gaussian no pixel blended: the exact zero instead of the reference's 0 * inf, as proj_bwd_fused_kernel)
    if (g0.x == 0.f && g0.y == 0.f && g0.z == 0.f && g0.w == 0.f && g1.x == 0.f && g1.y == 0.f && g1.z == 0.f &&
        g1.w == 0.f && g2.x == 0.f && g2.y == 0.f && g2.z == 0.f) {
#pragma unroll
        for (int a = 0; a < 3; a++) { g.dm[a] = 0.f; g.ds[a] = 0.f; }
#pragma unroll
        for (int a = 0; a < 4; a++) g.dq[a] = 0.f;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        gXyz[3 * p + a] = g.dm[a];
        xyzOwn[3 * p + a] = g.dm[a];
        gScales[3 * p + a] = g.ds[a] * s[a];          // d exp
    }
    // rotation normalisation VJP: y = q / (|q| + 1e-8)
    const float dot = g.dq[0] * rr[0] + g.dq[1] * rr[1] + g.dq[2] * rr[2] + g.dq[3] * rr[3];
    const float dn = -dot / (den * den);
    const float dn2 = dn * 0.5f / nrm;
#pragma unroll
    for (int a = 0; a < 4; a++) gRot[4 * p + a] = g.dq[a] / den + 2.0f * rr[a] * dn2;
    const float sg = 1.0f / (1.0f + expf(-opacityRaw[p]));
    gOpacity[p] = (AA ? cotOpacity * aaRho : cotOpacity) * sg * (1.0f - sg);
}

__global__ __launch_bounds__(PROJ_FUSED_THREADS) void sh_views_dir_adam_kernel(
    int N, int K, int degree, ViewCentersOwn views, const float* __restrict__ xyz, const float* __restrict__ mgAll,
    long long mgStride, const float* fdcParam, const float* frestParam, float* __restrict__ xyzAdd,
    float* __restrict__ gradNormAccum, AdamFuse adam)
{
    extern __shared__ float shLds[];
    const uint32_t gateWord = adam_gate_word(adam);      // (the ranks' gathered words ORed; looked at in front of the first store)
    adam_gate_publish(adam, gateWord);
    const int p = blockIdx.x * PROJ_FUSED_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = (K - 1) * 3;
    float* myRows = shLds + wv * 64 * (L + 1);
    float* rest = myRows + lane * (L + 1);
    const int row0 = blockIdx.x * PROJ_FUSED_THREADS + wv * 64;
    const int rows = min(64, N - row0);
    // the wave's f_rest span: HBM -> registers (kept for the Adam update at the bottom) -> LDS rows (read per lane below)
    float4 keptRows[SH_ROWS_MAX4];
    const int total4 = (rows * L) >> 2;
    const bool kept = rows > 0 && L > 0 && (L & 3) == 0 && total4 <= 64 * SH_ROWS_MAX4 &&
                      (((size_t)(frestParam - adam.pBase) + (size_t)row0 * L) & 3) == 0;
    if (kept) {
        sh_rows_load4(frestParam + (size_t)row0 * L, total4, 0, lane, keptRows);
        sh_rows_to_lds4(myRows, total4, L, 0, lane, keptRows);
    } else if (rows > 0 && L > 0) sh_rows_in(myRows, frestParam + (size_t)row0 * L, rows, L, lane);
    if (p < N) {
        const float m0 = xyz[3 * p], m1 = xyz[3 * p + 1], m2 = xyz[3 * p + 2];
        // pass 1: the view-direction terms of the xyz gradient, from the coefficients as the forwards saw them
        float ds0 = 0.f, ds1 = 0.f, ds2 = 0.f, stat = 0.f;
        bool mine = false;
        for (int r = 0; r < views.n; r++) {
            const float* mg = mgAll + (size_t)r * (size_t)mgStride + (size_t)p * 3;
            const float g0 = mg[0], g1 = mg[1], g2 = mg[2];
            float dx = 0.f, dy = 0.f, dz = 0.f;
            if (!(g0 == 0.0f && g1 == 0.0f && g2 == 0.0f))
                sh_foreach(degree, m0 - views.c[r][0], m1 - views.c[r][1], m2 - views.c[r][2],
                           [&](int k, float, float gx, float gy, float gz) {
                               if (k == 0) return;          // (the constant basis function has no gradient)
                               const float w0 = rest[(k - 1) * 3] * g0, w1 = rest[(k - 1) * 3 + 1] * g1, w2 = rest[(k - 1) * 3 + 2] * g2;
                               dx += gx * w0; dy += gy * w0; dz += gz * w0;
                               dx += gx * w1; dy += gy * w1; dz += gz * w1;
                               dx += gx * w2; dy += gy * w2; dz += gz * w2;
                           });
            ds0 += dx; ds1 += dy; ds2 += dz;
            if (views.own[r]) {        // a view this rank rendered: its full xyz gradient, for accum_grad_norm (densify.hip), per VIEW
                const float* o = views.own[r] + (size_t)p * 3;
                const float gx = o[0] + dx, gy = o[1] + dy, gz = o[2] + dz;
                stat += sqrtf(gx * gx + gy * gy + gz * gz);
                mine = true;
            }
        }
        xyzAdd[3 * p] = ds0; xyzAdd[3 * p + 1] = ds1; xyzAdd[3 * p + 2] = ds2;
        if (gradNormAccum && mine && !gateWord) gradNormAccum[p] += stat;
        // pass 2: the SH gradients, summed over the views in view order, in place of the coefficients
        for (int i = 0; i < L; i++) rest[i] = 0.0f;
        float dc[3] = {0.f, 0.f, 0.f};
        for (int r = 0; r < views.n; r++) {
            const float* mg = mgAll + (size_t)r * (size_t)mgStride + (size_t)p * 3;
            const float g0 = mg[0], g1 = mg[1], g2 = mg[2];
            if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) continue;
            sh_foreach(degree, m0 - views.c[r][0], m1 - views.c[r][1], m2 - views.c[r][2],
                       [&](int k, float b, float, float, float) {
                           if (k == 0) { dc[0] += b * g0; dc[1] += b * g1; dc[2] += b * g2; }
                           else { rest[(k - 1) * 3] += b * g0; rest[(k - 1) * 3 + 1] += b * g1; rest[(k - 1) * 3 + 2] += b * g2; }
                       });
        }
        if (!gateWord) {
            const size_t off = (size_t)(fdcParam - adam.pBase) + 3 * (size_t)p;
            float pv[3], mv[3], vv[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) { pv[ch] = adam.pBase[off + ch]; mv[ch] = adam.mBase[off + ch]; vv[ch] = adam.vBase[off + ch]; }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) adam_step(adam, dc[ch], adam.lr[1], pv[ch], mv[ch], vv[ch]);
            struct __attribute__((packed, aligned(4))) V3 { float x, y, z; };
            *reinterpret_cast<V3*>(const_cast<float*>(adam.pBase) + off) = V3{pv[0], pv[1], pv[2]};
            *reinterpret_cast<V3*>(adam.mBase + off) = V3{mv[0], mv[1], mv[2]};
            *reinterpret_cast<V3*>(adam.vBase + off) = V3{vv[0], vv[1], vv[2]};
        }
    }
    if (rows > 0 && L > 0 && !gateWord) {
        if (kept) adam_rows_kept(adam, frestParam, row0, total4, L, myRows, lane, adam.lr[2], keptRows);
        else adam_rows(adam, frestParam, row0, rows, L, myRows, lane, adam.lr[2]);
    }
}

// ---------------------------------------------------------------------------------------------
// packing helpers
// ---------------------------------------------------------------------------------------------
__global__ void pack11_to_12_kernel(int N, const float* __restrict__ p11, float* __restrict__ p12)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 12) return;
    const int g = i / 12, k = i - g * 12;
    p12[i] = k < 11 ? p11[(size_t)g * 11 + k] : 0.0f;
}

__global__ void pack_gaussians_kernel(int N, const float* __restrict__ means2d, const float* __restrict__ conic,
                                      const float* __restrict__ color, const float* __restrict__ opacity,
                                      const float* __restrict__ depths, float* __restrict__ packed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float* o = packed + (size_t)i * 11;
    o[0] = means2d[2 * i]; o[1] = means2d[2 * i + 1];
#pragma unroll
    for (int k = 0; k < 4; k++) o[2 + k] = conic[4 * i + k];
#pragma unroll
    for (int k = 0; k < 3; k++) o[6 + k] = color[3 * i + k];
    o[9] = opacity[i];
    o[10] = depths[i];
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int launch_projection_forward(gs_ctx* c, int N, int K, const float* scales, const float* rot, const float* means3d,
                              const float* shs, const CamParams& cam, float* means2d, float* depths, float* color,
                              float* cov2d, float* conic, float* radii, float* rectMin, float* rectMax)
{
    if (N == 0) return GS_OK;
    if (c->modes.fisheye)
        hipLaunchKernelGGL(proj_fwd_op_fisheye_kernel, dim3(gs_div_up(N, PROJ_THREADS)), dim3(PROJ_THREADS), 0, c->stream, N, K,
                           c->modes.degree, cam, scales, rot, means3d, shs, means2d, depths, color, cov2d, conic, radii,
                           rectMin, rectMax);
    else
    hipLaunchKernelGGL(proj_fwd_op_kernel, dim3(gs_div_up(N, PROJ_THREADS)), dim3(PROJ_THREADS), 0, c->stream, N, K,
                       c->modes.degree, cam, scales, rot, means3d, shs, means2d, depths, color, cov2d, conic, radii,
                       rectMin, rectMax);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_projection_backward(gs_ctx* c, int N, int K, const float* scales, const float* rot, const float* means3d,
                               const float* shs, const CamParams& cam, const float* cotDepths,
                               const float* cotMeans2d, const float* cotCov2d, const float* cotColor,
                               const float* cotConic, float* gScales, float* gRot, float* gMeans, float* gShs,
                               float* gCam)
{
    if (N == 0) return GS_OK;
    if (c->modes.fisheye)
        hipLaunchKernelGGL(proj_bwd_op_fisheye_kernel, dim3(gs_div_up(N, PROJ_THREADS)), dim3(PROJ_THREADS), 0, c->stream, N, K,
                           c->modes.degree, cam, scales, rot, means3d, shs, cotDepths, cotMeans2d, cotCov2d, cotColor,
                           cotConic, gScales, gRot, gMeans, gShs, gCam);
    else
    hipLaunchKernelGGL(proj_bwd_op_kernel, dim3(gs_div_up(N, PROJ_THREADS)), dim3(PROJ_THREADS), 0, c->stream, N, K,
                       c->modes.degree, cam, scales, rot, means3d, shs, cotDepths, cotMeans2d, cotCov2d, cotColor,
                       cotConic, gScales, gRot, gMeans, gShs, gCam);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// Runtime flags as template parameters: f(std::bool_constant<flag>{}...), one per flag and in their order.  f is a generic lambda
// that guards its launch with `if constexpr (..._form_exists(...))`, so only the forms that exist are instantiated.
template <class F>
static int with_flags(F&& f) { return f(); }
template <class F, class... Rest>
static int with_flags(F&& f, bool flag, Rest... rest)
{
    if (flag) return with_flags([&](auto... r) { return f(std::true_type{}, r...); }, rest...);
    return with_flags([&](auto... r) { return f(std::false_type{}, r...); }, rest...);
}

int launch_projection_fused_forward(gs_ctx* c, int N, int K, const float* xyz, const float* fdc, const float* frest,
                                    const float* scales, const float* rot, const float* opacity,
                                    const CamParams& cam, float* radii)
{
    if (N == 0) return GS_OK;
    const int L = (K - 1) * 3;
    const bool twoPhase = (L % 8) == 0 && L >= 48 && L / 2 <= 4 * SH_HALF_MAX4;     // K = 25: two halves of 36 floats
    const size_t lds = sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * ((twoPhase ? L / 2 : L) + 1);
    // K = 25: geometry here, the colours as riders of the binning kernels behind this launch (gs_rider.h)
    // -- where those kernels have room for them: the three launches of the splitter depth sort and the tile sort's prefix
    // kernel (16385 .. 655 k Gaussians, not the context's first forward).  Elsewhere the split costs more than it hides
    // (measured): one projection kernel as before.  GS_TUNE_COLOUR_RIDERS = 2 forces the split (A/B).
    // pose refinement: the camera lives on the device, and only this kernel reads it -- no riders, no self-colour split
    const bool posed = c->modes.poseDelta != nullptr;
    c->rider.on = !posed && K == GS_RIDER_K && (c->colourRiders == 2 || (c->colourRiders == 1 && depth_sort_takes_splitters(c, N)));
    // where no rider travels (the LSD depth sort's and the one-workgroup sort's kernels are no hosts): geometry first, then
    // the wave's own colours with the rows of unseen Gaussians left out -- faster than the interleaved one-kernel form at
    // every size measured (2 M garden 0.168 -> 0.129 ms, 300 k 0.035 -> 0.031, 10 k 0.0116 -> 0.0098; same bits).
    // GS_TUNE_COLOUR_RIDERS = 3 forces this form, 0 the interleaved one
    const bool selfColour = !posed && K == GS_RIDER_K && !c->rider.on && (c->colourRiders == 3 || c->colourRiders == 1);
    // a view under depth cuts: its cuts in coarse form first (binning.hip), for the kernel to drop the Gaussians that lie beyond
    // all of theirs (block lists and 16 x 16 tiles alike: the context's grid is the grid the cuts are kept on)
    GsCutCoarse cc;
    c->dropBlocks = 0;
    if (c->fwd.cutsActive && c->fwd.cutStore && c->dropPerBlock) {
        const int src = launch_cut_super(c, c->fwd.cutStore);
        if (src) return src;
        cc.superCut = c->superCut; cc.superW = cut_super_width(c); cc.dropPerBlock = c->dropPerBlock;
        c->dropBlocks = gs_div_up(N, PROJ_FUSED_THREADS);
    }
    // the rects' row groups (rect_row_groups4) where the kernel trims: 16 x 16 tiles, no block lists, the knob on -- the expansion
    // of this forward then enumerates the groups (binning.hip, expand_kernel<.., true>)
    c->piecesValid = c->trimRects && c->rowGroups && !c->virt.nbx && c->tileW == 16 && c->tileH == 16 && c->tilePieces != nullptr;
    uint4* pieces = c->piecesValid ? c->tilePieces : nullptr;
    const int pflags = (gs_small_depth_sort(N) ? 1 : 0) | (c->trimRects ? 2 : 0);      // bit 0: no depth key for a Gaussian that touches
                                                                                      // no tile; bit 1: GS_TUNE_TRIM_RECTS
    ColourRider a = {};
    a.xyz = xyz; a.fdc = fdc; a.frest = frest; a.packed12 = c->packed12; a.tilesTouched = c->tilesTouched;
    a.cam[0] = cam.cam[0]; a.cam[1] = cam.cam[1]; a.cam[2] = cam.cam[2];
    a.N = N; a.degree = c->modes.degree; a.unit0 = 0; a.units = gs_div_up(N, 64);
    if (c->rider.on) {
        c->rider.args = a;
        c->rider.args.units = 0;
        c->rider.next = 0;
        c->rider.total = gs_div_up(N, 64);
    }
    // the form: geometry only under riders; the posed camera with the colours in the same kernel; geometry, then the wave's own
    // colours; else the colours in the same kernel -- in two phases where the rows allow it
    const bool colour = !c->rider.on && !selfColour;
    const size_t dynLds = c->rider.on ? 0 : colour ? lds : sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * GS_RIDER_ROW;
    const int rc = with_flags(
        [&](auto TWO_PHASE, auto COLOUR, auto SELF, auto AA, auto F3D, auto POSE, auto FISHEYE) {
            if constexpr (proj_fwd_form_exists(TWO_PHASE, COLOUR, SELF, POSE, F3D, FISHEYE)) {
                hipLaunchKernelGGL((proj_fwd_fused_kernel<TWO_PHASE, COLOUR, SELF, AA, F3D, POSE, FISHEYE>), dim3(gs_div_up(N, PROJ_FUSED_THREADS)),
                                   dim3(PROJ_FUSED_THREADS), dynLds, c->stream, N, K, c->modes.degree, cam, c->tileW, c->tileH,
                                   c->gridW, c->gridH, xyz, fdc, frest, scales, rot, opacity, c->packed12, radii, c->tileRect,
                                   c->tilesTouched, c->depthKey[0], c->depthVal[0], c->visPerBlock, c->counters, pflags, a, c->virt, cc,
                                   pieces, c->modes.filter3d, c->poseCam);
                return GS_OK;
            } else {      // unreachable: rider.on and selfColour each imply !posed and exclude one another, and api.hip refuses a
                          // fisheye forward under a pose correction or a 3-D filter, so the form exists;
                          // the branch is here for the lambda to compile for the combinations that have no kernel
                c->err = "fused projection forward: no kernel for this combination of settings";
                return GS_ERR_INVALID_ARG;
            }
        },
        !colour || twoPhase, colour, selfColour, c->modes.antialias, c->modes.filter3d != nullptr, posed, c->modes.fisheye);
    if (rc) return rc;
    c->visBlocks = gs_div_up(N, PROJ_FUSED_THREADS);
    GS_HIP_CHECK(c, hipGetLastError());
    if (c->sparseAdam) return launch_vis_mask(c, N, radii);      // (gs_render_forward hands a radii buffer of the context's in then)
    return GS_OK;
}

int launch_vis_mask(gs_ctx* c, int N, const float* radii)
{
    if (N == 0) return GS_OK;
    if (!radii || !c->visMask || N > c->visCap) { c->err = "sparse Adam: no visibility buffers for this forward"; return GS_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(vis_mask_kernel, dim3(gs_div_up(N, 256)), dim3(256), 0, c->stream, N, radii, c->visMask);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// the colour units no binning kernel has taken along (gs_rider.h): in front of the blend, on the whole chip
__global__ __launch_bounds__(GS_RIDER_WAVES * 64) void colour_rest_kernel(ColourRider r)
{
    colour_rider_block(r, (int)blockIdx.x);
}

int launch_colour_rest(gs_ctx* c)
{
    if (!c->rider.on) return GS_OK;
    c->rider.on = false;
    const int left = c->rider.total - c->rider.next;
    if (left <= 0) return GS_OK;
    ColourRider a = c->rider.args;
    a.unit0 = c->rider.next; a.units = left;
    c->rider.next = c->rider.total;
    hipLaunchKernelGGL(colour_rest_kernel, dim3(rider_blocks(left, GS_RIDER_WAVES * 64)), dim3(GS_RIDER_WAVES * 64), 0, c->stream, a);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// The fused backward of the context's forward (c->fwd), in the form its settings ask for.  mode: 0 gradients out, 1 the data-parallel
// variant (g.fdc receives mg[N,3]), 2 the fused Adam step (no gradient leaves the kernel).  The filter beats the MCMC step beats sparse
// Adam (api.hip lets no two of them be on together); a posed forward gets its pose gradient behind the kernel.
struct ProjBwdGrads { float *xyz, *fdc, *frest, *scales, *rot, *opacity; };
static int launch_proj_bwd_fused(gs_ctx* c, int mode, const ProjBwdGrads& g, const AdamFuse& adam)
{
    const int N = c->fwd.N, K = c->fwd.K;
    if (N == 0) return c->fwd.modes.poseDelta && mode != 1 ? launch_pose_grad(c, 0) : GS_OK;
    const bool f3d = c->fwd.modes.filter3d != nullptr;       // (the filter this backward's forward ran with; no data-parallel form: api.hip refuses)
    if (f3d && mode == 1) mode = 0;
    const bool pose = c->fwd.modes.poseDelta && mode != 1;
    const bool mcmc = mode == 2 && !f3d && c->mcmcOn;
    const bool sparse = mode == 2 && !f3d && !mcmc && c->sparseAdam;      // (api.hip has checked that the forward left its mask)
    ProjBwdArgs a = {};
    a.N = N; a.K = K; a.degree = c->fwd.modes.degree;      // (the degree this backward's forward ran with: gs_set_sh_degree)
    a.cam = c->fwd.cam; a.dcam = c->poseCam;
    a.xyz = c->fwd.xyz; a.fdc = c->fwd.fdc; a.frest = c->fwd.frest; a.scalesRaw = c->fwd.scales; a.rotRaw = c->fwd.rot;
    a.opacityRaw = c->fwd.opacity; a.gradAcc16 = c->gradAcc16;
    a.gXyz = g.xyz; a.gFdc = g.fdc; a.gFrest = g.frest; a.gScales = g.scales; a.gRot = g.rot; a.gOpacity = g.opacity;
    a.gradNormAccum = c->gradNormAccum;
    a.adam = adam;
    a.posePartials = c->posePartials;
    if (mcmc) a.mc = mcmc_fuse(c->mcmc, N, adam.lr[0]);
    a.filter3d = c->fwd.modes.filter3d;
    a.visMask = c->visMask;
    // the band-limited form: a plain fused Adam step below the degree K allows (GS_TUNE_SH_BAND_SKIP 0: the full-row form, whose
    // inactive columns meet exact zero gradients); at degree 0 it uses no LDS
    const bool bands = mode == 2 && !pose && !mcmc && !f3d && !sparse && c->shBandSkip && (a.degree + 2) * (a.degree + 2) <= K;
    const size_t lds = bands && a.degree == 0 ? 0 : sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * ((K - 1) * 3 + 1);
    const int rc = with_flags(
        [&](auto ADAM, auto EMIT_MG, auto POSE, auto AA, auto MCMC, auto F3D, auto SPARSE, auto FISHEYE, auto BANDS) {
            constexpr int MODE = ADAM ? 2 : EMIT_MG ? 1 : 0;
            if constexpr (!(ADAM && EMIT_MG) && proj_bwd_form_exists(MODE, POSE, MCMC, F3D, SPARSE, FISHEYE, BANDS)) {
                hipLaunchKernelGGL((proj_bwd_fused_kernel<MODE, POSE, AA, MCMC, F3D, SPARSE, FISHEYE, BANDS>), dim3(gs_div_up(N, PROJ_FUSED_THREADS)),
                                   dim3(PROJ_FUSED_THREADS), lds, c->stream, a);
                return GS_OK;
            } else {      // unreachable: f3d, mcmc and sparse are derived above to exclude one another and, like pose, mode 1;
                          // a fisheye forward ran without pose correction and filter (api.hip);
                          // the branch is here for the lambda to compile for the combinations that have no kernel
                c->err = "fused projection backward: no kernel for this combination of settings";
                return GS_ERR_INVALID_ARG;
            }
        },
        mode == 2, mode == 1, pose, c->fwd.modes.antialias, mcmc, f3d, sparse, c->fwd.modes.fisheye, bands);
    if (rc) return rc;
    GS_HIP_CHECK(c, hipGetLastError());
    return pose ? launch_pose_grad(c, N) : GS_OK;
}

int launch_projection_fused_backward(gs_ctx* c, float* gXyz, float* gFdc, float* gFrest, float* gScales, float* gRot, float* gOpacity,
                                     bool emitColorCot)
{
    AdamFuse none = {};
    if (!emitColorCot) { none.ovf = c->counters + GS_CNT_OVERFLOW; none.rider = c->overflowRider; }
    return launch_proj_bwd_fused(c, emitColorCot ? 1 : 0, ProjBwdGrads{gXyz, gFdc, gFrest, gScales, gRot, gOpacity}, none);
}

int launch_projection_fused_backward_adam(gs_ctx* c, const float* pBase, float* mBase, float* vBase, const float lr[6], float b1,
                                          float b2, float eps, float gscale)
{
    AdamFuse a = {};
    a.pBase = pBase; a.mBase = mBase; a.vBase = vBase;
    for (int i = 0; i < 6; i++) a.lr[i] = lr[i];
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = gscale;
    a.gate = c->adamGate;
    return launch_proj_bwd_fused(c, 2, ProjBwdGrads{}, a);
}

// gs_set_gathered_gate: the gathered colour cotangents come as `count` blocks of ccBlockFloats floats, every block's word
// [3 N] = that rank's overflow rider
static long long cc_block_floats(const gs_ctx* c, int N) { return c->ccBlockFloats > 0 ? c->ccBlockFloats : 3LL * N; }
static void fill_gathered_gate(const gs_ctx* c, int N, const float* mgAll, AdamFuse& a)
{
    a.seen = c->gateSeen;
    if (c->ccBlockFloats <= 0) return;
    a.gwWords = reinterpret_cast<const uint32_t*>(mgAll + 3LL * N);
    a.gwStride = c->ccBlockFloats; a.gwCount = c->ccBlockCount; a.gwOut = c->gatheredGateOut;
}

int launch_color_cot(gs_ctx* c, int N, float* out)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(color_cot_kernel, dim3(gs_div_up(N, 256)), dim3(256), 0, c->stream, N, c->gradAcc16, c->packed12,
                       out, c->counters + GS_CNT_OVERFLOW, c->overflowRider);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_sh_grad_from_views(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll,
                              const float* camCentersHost, float* gFdc, float* gFrest)
{
    if (N == 0) return GS_OK;
    ViewCenters v;
    v.n = R;
    for (int r = 0; r < R; r++) for (int k = 0; k < 3; k++) v.c[r][k] = camCentersHost[r * 3 + k];
    const size_t lds = sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * ((K - 1) * 3 + 1);
    AdamFuse none = {};
    fill_gathered_gate(c, N, mgAll, none);
    hipLaunchKernelGGL(sh_grad_from_views_kernel<false>, dim3(gs_div_up(N, PROJ_FUSED_THREADS)), dim3(PROJ_FUSED_THREADS),
                       lds, c->stream, N, K, c->modes.degree, v, xyz, mgAll, cc_block_floats(c, N), gFdc, gFrest, nullptr, nullptr, none);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_sh_grad_from_views_adam(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll,
                                   const float* camCentersHost, const float* fdcParam, const float* frestParam,
                                   const float* pBase, float* mBase, float* vBase, float lrDc, float lrRest, float b1,
                                   float b2, float eps, float gscale)
{
    if (N == 0) return GS_OK;
    ViewCenters v;
    v.n = R;
    for (int r = 0; r < R; r++) for (int k = 0; k < 3; k++) v.c[r][k] = camCentersHost[r * 3 + k];
    const size_t lds = sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * ((K - 1) * 3 + 1);
    AdamFuse a = {};
    a.pBase = pBase; a.mBase = mBase; a.vBase = vBase;
    a.lr[1] = lrDc; a.lr[2] = lrRest;
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = gscale;
    a.gate = c->adamGate;
    fill_gathered_gate(c, N, mgAll, a);
    hipLaunchKernelGGL(sh_grad_from_views_kernel<true>, dim3(gs_div_up(N, PROJ_FUSED_THREADS)), dim3(PROJ_FUSED_THREADS),
                       lds, c->stream, N, K, c->modes.degree, v, xyz, mgAll, cc_block_floats(c, N), nullptr, nullptr, fdcParam, frestParam, a);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_projection_geom_backward(gs_ctx* c, float* gXyz, float* gScales, float* gRot, float* gOpacity, float* xyzOwn, float* colorCot)
{
    const int N = c->fwd.N;
    if (N == 0) return GS_OK;
    with_flags(
        [&](auto AA) {
            hipLaunchKernelGGL(proj_bwd_geom_kernel<AA>, dim3(gs_div_up(N, 256)), dim3(256), 0, c->stream, N, c->fwd.cam, c->fwd.xyz,
                               c->fwd.scales, c->fwd.rot, c->fwd.opacity, c->gradAcc16, gXyz, gScales, gRot, gOpacity, xyzOwn,
                               c->packed12, colorCot, c->counters + GS_CNT_OVERFLOW, c->overflowRider);
            return GS_OK;
        },
        c->fwd.modes.antialias);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_sh_views_dir_adam(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll, const float* camCentersHost,
                             const float* const* ownXyzHost, const float* fdcParam, const float* frestParam, const float* pBase,
                             float* mBase, float* vBase, float lrDc, float lrRest, float b1, float b2, float eps, float gscale,
                             float* xyzAdd)
{
    if (N == 0) return GS_OK;
    ViewCentersOwn v;
    v.n = R;
    for (int r = 0; r < 16; r++) v.own[r] = nullptr;
    for (int r = 0; r < R; r++) {
        for (int k = 0; k < 3; k++) v.c[r][k] = camCentersHost[r * 3 + k];
        v.own[r] = ownXyzHost ? ownXyzHost[r] : nullptr;
    }
    const size_t lds = sizeof(float) * (PROJ_FUSED_THREADS / 64) * 64 * ((K - 1) * 3 + 1);
    AdamFuse a = {};
    a.pBase = pBase; a.mBase = mBase; a.vBase = vBase;
    a.lr[1] = lrDc; a.lr[2] = lrRest;
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = gscale;
    a.gate = c->adamGate;
    fill_gathered_gate(c, N, mgAll, a);
    hipLaunchKernelGGL(sh_views_dir_adam_kernel, dim3(gs_div_up(N, PROJ_FUSED_THREADS)), dim3(PROJ_FUSED_THREADS), lds, c->stream, N,
                       K, c->modes.degree, v, xyz, mgAll, cc_block_floats(c, N), fdcParam, frestParam, xyzAdd, c->gradNormAccum, a);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_pack11_to_12(gs_ctx* c, int N, const float* packed11)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(pack11_to_12_kernel, dim3(gs_div_up((long long)N * 12, 256)), dim3(256), 0, c->stream, N,
                       packed11, c->packed12);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_pack_gaussians(gs_ctx* c, int N, const float* means2d, const float* conic, const float* color,
                          const float* opacity, const float* depths, float* packed11)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(pack_gaussians_kernel, dim3(gs_div_up(N, 256)), dim3(256), 0, c->stream, N, means2d, conic,
                       color, opacity, depths, packed11);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}


// ---------------------------------------------------------------------------------------------
// pose refinement (gs_set_pose_correction; DESIGN.md "Pose refinement")
// ---------------------------------------------------------------------------------------------
// R(w) = I + A K + B K^2, K = [w]x, t = |w|: A = sin t / t, B = (1 - cos t) / t^2; the Jacobian needs C = A'(t) / t =
// (t cos t - sin t) / t^3 and D = B'(t) / t = (t sin t - 2 (1 - cos t)) / t^4.  Taylor series below t^2 = 1e-3 (the first
// omitted terms are under 1e-12 there), so that R(0) is exactly I; 1 - cos t as 2 sin^2(t / 2) above it.
__device__ void rodrigues_coeffs(double t2, double& A, double& B, double& C, double& D)
{
    if (t2 < 1e-3) {
        A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
        B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
        C = -1.0 / 3.0 + t2 / 30.0 - t2 * t2 / 840.0;
        D = -1.0 / 12.0 + t2 / 180.0 - t2 * t2 / 6720.0;
    } else {
        const double t = sqrt(t2), s = sin(t), h = sin(0.5 * t), omc = 2.0 * h * h;
        A = s / t;
        B = omc / t2;
        C = (t * cos(t) - s) / (t2 * t);
        D = (t * s - 2.0 * omc) / (t2 * t2);
    }
}

__device__ void skew(const double w[3], double K[3][3])
{
    K[0][0] = 0.0;   K[0][1] = -w[2]; K[0][2] = w[1];
    K[1][0] = w[2];  K[1][1] = 0.0;   K[1][2] = -w[0];
    K[2][0] = -w[1]; K[2][1] = w[0];  K[2][2] = 0.0;
}

__device__ void matmul3(const double X[3][3], const double Y[3][3], double Z[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Z[i][j] = X[i][0] * Y[0][j] + X[i][1] * Y[1][j] + X[i][2] * Y[2][j];
}

__device__ void rodrigues(const double w[3], double R[3][3])
{
    double A, B, C, D, K[3][3], K2[3][3];
    rodrigues_coeffs(w[0] * w[0] + w[1] * w[1] + w[2] * w[2], A, B, C, D);
    skew(w, K);
    matmul3(K, K, K2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = (i == j ? 1.0 : 0.0) + A * K[i][j] + B * K2[i][j];
}

// The corrected camera: c2w' = c2w [[R, tau], [0, 1]], so w2c' = [[R^T Rw, R^T (tw - tau)], [0, 1]] with w2c = [[Rw, tw], [0, 1]]
// = V^T (p_view = [p, 1] V), and cam' = cam + Rw^T tau.  A delta of six zero words copies the host camera bit for bit.
__global__ __launch_bounds__(64) void pose_camera_kernel(CamParams host, const float* __restrict__ delta, CamParams* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    CamParams o = host;
    bool zero = true;
    for (int i = 0; i < 6; i++) zero = zero && __float_as_uint(delta[i]) == 0u;
    if (!zero) {
        const double w[3] = {delta[0], delta[1], delta[2]}, tau[3] = {delta[3], delta[4], delta[5]};
        double R[3][3];
        rodrigues(w, R);
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 4; k++) {
                double acc = 0.0;
                for (int j = 0; j < 3; j++) acc += R[j][a] * ((double)host.V[4 * k + j] - (k == 3 ? tau[j] : 0.0));
                o.V[4 * k + a] = (float)acc;
            }
        for (int i = 0; i < 3; i++) {
            double acc = host.cam[i];
            for (int j = 0; j < 3; j++) acc += (double)host.V[4 * i + j] * tau[j];
            o.cam[i] = (float)acc;
        }
    }
    *out = o;
}

// dL/d delta from the wave partials of proj_bwd_fused_kernel's POSE forms: one workgroup, sums in a fixed order (no atomics), the
// chain rule in float64.  G[k][a] = dL/dV'[k][a] = part [3 k + a] (k < 4, a < 3), gc = dL/dcam' = parts [12 .. 14].  With dA = G^T (dL/d w2c'[:3, :4]),
// B = [Rw | tw - tau]:  dL/dtau = -(R dA)[:, 3] + Rw gc,  dL/dw_i = sum_ja (B dA^T)[j][a] dR[j][a]/dw_i,
// dR/dw_i = C w_i K + A E_i + D w_i K^2 + B (E_i K + K E_i), E_i = [e_i]x.
__global__ __launch_bounds__(256) void pose_grad_kernel(int nParts, const float* __restrict__ parts, CamParams host,
                                                        const float* __restrict__ delta, float* __restrict__ gradDelta)
{
    // thread (g, q): columns 4 q .. 4 q + 3 of rows g, g + 64, g + 128, ...; eight rows' loads in flight at a time, added in
    // row order; then the 64 groups pairwise in a fixed tree.  Column 15 is a zero pad.
    __shared__ double acc[64][16];
    const int q = threadIdx.x & 3, grp = threadIdx.x >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(parts);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    constexpr int B = 8;
    for (int r0 = grp; r0 < nParts; r0 += 64 * B) {
        float4 v[B];
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int r = r0 + 64 * b;
            v[b] = r < nParts ? p4[4 * (size_t)r + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int b = 0; b < B; b++) { s0 += v[b].x; s1 += v[b].y; s2 += v[b].z; s3 += v[b].w; }
    }
    acc[grp][4 * q] = s0; acc[grp][4 * q + 1] = s1; acc[grp][4 * q + 2] = s2; acc[grp][4 * q + 3] = s3;
    for (int h = 32; h > 0; h >>= 1) {
        __syncthreads();
        if (grp < h)
            for (int k = 0; k < 4; k++) acc[grp][4 * q + k] += acc[grp + h][4 * q + k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[15];
    for (int k = 0; k < 15; k++) tot[k] = acc[0][k];
    const double w[3] = {delta[0], delta[1], delta[2]}, tau[3] = {delta[3], delta[4], delta[5]};
    double A, Bc, C, D, K[3][3], K2[3][3], R[3][3];
    rodrigues_coeffs(w[0] * w[0] + w[1] * w[1] + w[2] * w[2], A, Bc, C, D);
    skew(w, K);
    matmul3(K, K, K2);
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) R[i][k] = (i == k ? 1.0 : 0.0) + A * K[i][k] + Bc * K2[i][k];
    double dA[3][4], Bm[3][4];
    for (int a = 0; a < 3; a++)
        for (int k = 0; k < 4; k++) {
            dA[a][k] = tot[3 * k + a];
            Bm[a][k] = (double)host.V[4 * k + a] - (k == 3 ? tau[a] : 0.0);
        }
    double g[6];
    for (int r = 0; r < 3; r++) {
        double t = 0.0;
        for (int a = 0; a < 3; a++) t -= R[r][a] * dA[a][3];
        for (int i = 0; i < 3; i++) t += (double)host.V[4 * i + r] * tot[12 + i];
        g[3 + r] = t;
    }
    double Gam[3][3];
    for (int jj = 0; jj < 3; jj++)
        for (int a = 0; a < 3; a++) {
            double t = 0.0;
            for (int k = 0; k < 4; k++) t += Bm[jj][k] * dA[a][k];
            Gam[jj][a] = t;
        }
    for (int i = 0; i < 3; i++) {
        double e[3] = {0.0, 0.0, 0.0}, E[3][3], EK[3][3], KE[3][3];
        e[i] = 1.0;
        skew(e, E);
        matmul3(E, K, EK);
        matmul3(K, E, KE);
        double t = 0.0;
        for (int jj = 0; jj < 3; jj++)
            for (int a = 0; a < 3; a++)
                t += Gam[jj][a] * (C * w[i] * K[jj][a] + A * E[jj][a] + D * w[i] * K2[jj][a] + Bc * (EK[jj][a] + KE[jj][a]));
        g[i] = t;
    }
    for (int q = 0; q < 6; q++) gradDelta[q] = (float)g[q];
}

int launch_pose_camera(gs_ctx* c, const CamParams& host, const float* delta)
{
    hipLaunchKernelGGL(pose_camera_kernel, dim3(1), dim3(64), 0, c->stream, host, delta, c->poseCam);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// floats of the backward's pose partials: a row of 16 per wave of proj_bwd_fused_kernel's POSE forms
long long pose_partials_floats(int N)
{
    return 16LL * gs_div_up(N, PROJ_FUSED_THREADS) * (PROJ_FUSED_THREADS / 64);
}

int launch_pose_grad(gs_ctx* c, int N)
{
    const int parts = (int)(pose_partials_floats(N) / 16);
    hipLaunchKernelGGL(pose_grad_kernel, dim3(1), dim3(256), 0, c->stream, N > 0 ? parts : 0, c->posePartials, c->fwd.cam,
                       c->fwd.modes.poseDelta, c->fwd.modes.poseGrad);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
