// api.hip -- C ABI (include/gsplat.h): context, workspace, argument checks, launch sequencing.
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include "gs_ctx.h"
#include <vector>

using namespace gs;

namespace {

int fail(gs_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

// what a regrow of the per-Gaussian workspace replaces
void free_gaussian_ws(gs_ctx* c)
{
    ctx_free(c, c->packed12); ctx_free(c, c->gradAcc16);
    for (int i = 0; i < 2; i++) { ctx_free(c, c->depthKey[i]); ctx_free(c, c->depthVal[i]); }
    ctx_free(c, c->tilesTouched); ctx_free(c, c->tileRect); ctx_free(c, c->tilePieces); ctx_free(c, c->waveSeg);
    ctx_free(c, c->scanPrefix); ctx_free(c, c->scanTmp); ctx_free(c, c->blockSums);
    ctx_free(c, c->visPerBlock); ctx_free(c, c->dropPerBlock);
    ctx_free(c, c->bucketId);
    ctx_free(c, c->densifyTiles);
    c->densifyInts = 0;
}

// ... and of the per-pair workspace (the checkpoint arena, segState, is not part of it: ensure_arena)
void free_pair_ws(gs_ctx* c)
{
    for (int i = 0; i < 2; i++) { ctx_free(c, c->pairKey[i]); ctx_free(c, c->pairVal[i]); }
    ctx_free(c, c->segSlot); ctx_free(c, c->itemBlock); ctx_free(c, c->itemRow);
}

// The checkpoint arena of the fused blend (blend_v2.hip): slots are taken as they are written, so the arena is sized
// from what forwards use, not from every list being swept to its end.  Reserved capacity: one 8x8-quadrant slot per 80
// reserved pairs (the bench scene writes one per ~100 pairs binned, the 100 k / 800x800 config one per ~30, against
// reserves of 3x and 5x their pairs; gs_ctx_reserve regrows to 1.5x the need after an overflow).  Without a reserve nothing may overflow silently between two host checks, so the arena holds the full bound.
int ensure_arena(gs_ctx* c)
{
    if (!c->fast16 || c->capM <= 0) return GS_OK;
    long long want = (c->pairsReserved || c->reserving) ? c->capM / 80 : c->segCap * 4;
    if (want < 65536) want = 65536;
    if (want > c->segCap * 4) want = c->segCap * 4;
    if (want < c->qslotWanted) want = c->qslotWanted;
    if (want <= c->qslotCap) return GS_OK;
    if (const int rc = ctx_grow(c, &c->segState, &c->qslotCap, want, 5 * 64)) return rc;
    c->fwd.valid = false;
    return GS_OK;
}

// grows the workspace to hold N Gaussians and M pairs; synchronises only when it has to reallocate
int ensure_capacity(gs_ctx* c, int N, long long M)
{
    bool grewN = false, grewM = false;
    if (N > c->capN) {
        GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        free_gaussian_ws(c);
        const size_t n = (size_t)N;
        int rc;
        if ((rc = ctx_alloc(c, &c->packed12, n * 12))) return rc;
        if ((rc = ctx_alloc(c, &c->gradAcc16, n * 16))) return rc;
        for (int i = 0; i < 2; i++) {
            if ((rc = ctx_alloc(c, &c->depthKey[i], n))) return rc;
            if ((rc = ctx_alloc(c, &c->depthVal[i], n))) return rc;
        }
        if ((rc = ctx_alloc(c, &c->tilesTouched, n))) return rc;
        if ((rc = ctx_alloc(c, &c->tileRect, n))) return rc;
        if ((rc = ctx_alloc(c, &c->tilePieces, n))) return rc;
        if ((rc = ctx_alloc(c, &c->waveSeg, (n / 64 + 8) * GS_EXPAND_SLICES))) return rc;
        if ((rc = ctx_alloc(c, &c->scanPrefix, (n / 64 + 16) * GS_EXPAND_SLICES))) return rc;
        if ((rc = ctx_alloc(c, &c->scanTmp, (n / 64 + 16) * GS_EXPAND_SLICES / 1024 + 8))) return rc;
        const size_t nb = n / GS_SCAN_BLOCK + 2;
        if ((rc = ctx_alloc(c, &c->blockSums, nb))) return rc;
        if ((rc = ctx_alloc(c, &c->visPerBlock, n / 128 + 2))) return rc;
        if ((rc = ctx_alloc(c, &c->dropPerBlock, n / 128 + 2))) return rc;
        if ((rc = ctx_alloc(c, &c->bucketId, n + 16))) return rc;
        c->capN = N;
        grewN = true;
    }
    if (M > c->capM) {
        GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        free_pair_ws(c);
        int rc;
        for (int i = 0; i < 2; i++) {
            if ((rc = ctx_alloc(c, &c->pairKey[i], (size_t)M))) return rc;
            if ((rc = ctx_alloc(c, &c->pairVal[i], (size_t)M))) return rc;
        }
        if (c->fast16) {
            // saved-state slots: sum over pixel blocks of ceil(list/SEG)-1 <= (pairs seen by pixel blocks)/SEG
            const long long blocksPerTile = (long long)(c->tileW / 16) * (c->tileH / 16);
            c->segCap = M / GS_SEG_LEN * blocksPerTile + 16;
            c->itemCap = c->segCap + c->numPixBlocks;
            if ((rc = ctx_alloc(c, &c->segSlot, (size_t)c->segCap * 4))) return rc;
            // (entries are only ever read where this forward wrote them; zeroed once so that a backward run on a
            // forward that overflowed -- host errors off -- reads slot 0, never an address out of bounds)
            GS_HIP_CHECK(c, hipMemset(c->segSlot, 0, (size_t)c->segCap * 4 * sizeof(uint32_t)));
            if ((rc = ctx_alloc(c, &c->itemBlock, (size_t)c->itemCap))) return rc;
            if ((rc = ctx_alloc(c, &c->itemRow, (size_t)c->itemCap))) return rc;
        }
        c->capM = M;
        grewM = true;
    }
    if (grewN || grewM) {
        const long long big = c->capM > c->capN ? c->capM : c->capN;
        const int nb = gs_div_up(big, GS_SORT_TILE) + 1;
        if (nb > c->nbCap) {
            ctx_free(c, c->hist); ctx_free(c, c->wideCnt); ctx_free(c, c->wideChunk);
            int rc = ctx_alloc(c, &c->hist, (size_t)256 * nb);
            if (rc) return rc;
            if (c->T <= GS_WIDE_BINS) {      // the one-pass tile sort's count tables (binning.hip)
                if ((rc = ctx_alloc(c, &c->wideCnt, (size_t)GS_WIDE_BINS * nb))) return rc;
                if ((rc = ctx_alloc(c, &c->wideChunk, (size_t)GS_WIDE_BINS * (nb / GS_WIDE_CHUNK + 2)))) return rc;
            }
            c->nbCap = nb;
        }
        c->binValid = false;
        c->fwd.valid = false;
    }
    return ensure_arena(c);
}

long long default_pair_capacity(const gs_ctx* c, int N)
{
    long long m = (long long)N * 12 + 4LL * c->T + 65536;
    return m;
}

int zero_counters(gs_ctx* c)
{
    GS_HIP_CHECK(c, hipMemsetAsync(c->counters, 0, sizeof(uint32_t) * GS_CNT_COUNT, c->stream));
    return GS_OK;
}

// [sync] pulls the counters to the host
int read_counters(gs_ctx* c)
{
    GS_HIP_CHECK(c, hipMemcpyAsync(c->countersHost, c->counters, sizeof(uint32_t) * GS_CNT_COUNT,
                                   hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int overflow_error(gs_ctx* c, uint32_t need)
{
    char buf[260];
    if (c->missHost && c->missHost[4] == 2u) {
        snprintf(buf, sizeof buf, "the fused forward ran out of checkpoint slots (%lld held): its image is complete, but no "
                 "backward can be taken from it and no optimizer step was; call gs_ctx_reserve (it regrows the arena)", c->qslotCap);
        c->err = buf;
        return GS_ERR_WORKSPACE_OVERFLOW;
    }
    snprintf(buf, sizeof buf, "tile-splat pairs M=%u exceed the reserved capacity %lld: that forward rendered nothing and "
             "no optimizer step was taken from it; call gs_ctx_reserve", need, c->capM);
    c->err = buf;
    return GS_ERR_WORKSPACE_OVERFLOW;
}
int overflow_error(gs_ctx* c) { return overflow_error(c, c->countersHost[GS_CNT_MREQ]); }

// Deferred overflow of a forward under reserved capacity (no host check of M per call): the expansion kernel raises
// two words in mapped host memory.  Looked at -- without waiting -- by every entry point that continues a training
// step, so the error surfaces at the first call after the device got there; the device-side gate (adamGate) has kept
// the parameters untouched meanwhile.  Stays raised until gs_sync has reported it or gs_ctx_reserve has fixed it.
int deferred_overflow(gs_ctx* c)
{
    if (c->hostOverflowErrors && c->missHost && c->missHost[4]) return overflow_error(c, c->missHost[5]);
    return GS_OK;
}

// runs the binning pipeline; in auto-capacity mode it checks M on the host and regrows once
template <class Prep>
int bin_with_capacity(gs_ctx* c, int N, bool reserved, bool wantPlain, Prep&& prep)
{
    int rc;
    if ((rc = ensure_capacity(c, N, c->capM > 0 ? c->capM : default_pair_capacity(c, N)))) return rc;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (N == 0 && (rc = zero_counters(c))) return rc;      // otherwise the prep kernel's first block clears them
        {
            GsStageTimer t(c, GS_STAGE_PROJ_FWD);
            if ((rc = prep())) return rc;
        }
        {
            GsStageTimer t(c, GS_STAGE_BIN);
            if ((rc = launch_binning(c, N, wantPlain))) return rc;
        }
        if (reserved) break;
        if ((rc = read_counters(c))) return rc;
        if (!c->countersHost[GS_CNT_OVERFLOW]) break;
        if (attempt == 1) return overflow_error(c);
        c->missHost[4] = 0;      // handled here (the wait above is behind the kernel that raised it): regrow and repeat
        const long long need = (long long)c->countersHost[GS_CNT_MREQ];
        if ((rc = ensure_capacity(c, N, need + need / 2 + 1024))) return rc;
    }
    c->binValid = true;
    c->binN = N;
    return GS_OK;
}

// waits for a forward that ran under depth cuts and records whether it missed (the wait is behind the forward only)
int settle_cut_forward(gs_ctx* c)
{
    if (!c->fwd.cutsActive || c->fwd.missChecked) return GS_OK;
    // busy-wait: the answer unblocks the launches of the rest of the step, and a blocking wait wakes up too late
    // (~0.1 ms) to keep the queue behind the loss kernel filled
    for (;;) {
        const hipError_t q = hipEventQuery(c->fwdDone);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) GS_HIP_CHECK(c, q);
    }
    c->fwd.missChecked = true;
    c->fwd.missed = c->missHost[0] != 0u;
    return GS_OK;
}

// what every backward entry point asks first: a usable forward (not consumed, not overflowed, and -- under depth
// cuts -- one that did not miss; a caller that never asked gs_forward_missed is answered here)
int backward_preflight(gs_ctx* c, const char* who, bool wantsDepth)
{
    if (!c->fwd.valid || c->fwd.consumed) {
        c->err = std::string(who) + ": no gs_render_forward on this context";
        return GS_ERR_NO_FORWARD;
    }
    int rc = deferred_overflow(c);
    if (rc) return rc;
    if (c->fwd.arenaOverflow) {
        c->err = std::string(who) + ": the forward ran out of checkpoint slots (reported by gs_sync): call gs_ctx_reserve and "
                 "repeat it";
        return GS_ERR_WORKSPACE_OVERFLOW;
    }
    if ((rc = settle_cut_forward(c))) return rc;
    if (c->fast16 && c->fwd.statePlanes == 0) {
        c->err = std::string(who) + ": the forward ran render-only (GS_TUNE_RENDER_ONLY): it kept nothing a backward could start from";
        return GS_ERR_NO_FORWARD;
    }
    if (wantsDepth && (!c->fwd.outDepth || (c->fast16 && c->fwd.statePlanes != 5))) {
        c->err = std::string(who) + ": cot_depth given, but the forward took no depth image (out_depth NULL) or ran with "
                 "GS_TUNE_DEPTH_GRADIENT off (no depth checkpoints)";
        return GS_ERR_INVALID_ARG;
    }
    if (c->fwd.missed) {
        c->err = std::string(who) + ": the forward ran under depth cuts and missed (gs_forward_missed): repeat it "
                 "with gs_set_depth_cuts(ctx, 0) first";
        return GS_ERR_NO_FORWARD;
    }
    return GS_OK;
}

// the armed distortion term's backward into the context's own accumulator rows (gs_arm_distortion): between the blend backward
// that fills them and their readers (a stage of its own, inside the blend-backward stage's interval)
int distortion_backward_of_forward(gs_ctx* c)
{
    GsStageTimer t(c, GS_STAGE_DISTORTION_BWD);
    return launch_blend_distortion_backward(c, c->distortion.params, c->distortion.cot, c->distortion.totals, c->gradAcc16);
}

// the blend backward of the last fused forward: the first stage of every backward entry point
// absgrad (gs_set_absgrad; gs_render_backward and gs_render_backward_adam only): the ABSGRAD instantiation, which leaves (Ax, Ay)
// in columns 12 and 13 of gradAcc16, and behind it the AbsGS statistic into the grad-norm accumulator (gate: the overflow word
// the fused Adam tests, null without it)
int blend_backward_of_forward(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                              bool absgrad = false, const uint32_t* gate = nullptr)
{
    if (c->adcGradSum && !c->fwd.radii)      // (before anything is launched: the forward stays usable)
        return fail(c, GS_ERR_NO_FORWARD, "the ADC statistic is set, but the forward kept no radii (gs_set_adc_stats comes before "
                                          "gs_render_forward)");
    GsStageTimer t(c, GS_STAGE_BLEND_BWD);
    c->absgradN = -1;
    if (!c->fast16) {
        const int rc = launch_blend_backward(c, c->fwd.modes.bg, c->fwd.N, cot_color, cot_depth, cot_alpha, c->fwd.outAlpha, c->lastContrib);
        return rc || !c->distortion.armed ? rc : distortion_backward_of_forward(c);
    }
    if (const int rc = launch_blend_backward_v2(c, c->fwd.N, cot_color, cot_depth, cot_alpha, c->fwd.outColor, c->fwd.outDepth,
                                                c->fwd.outAlpha, absgrad))
        return rc;
    // the distortion term (gs_arm_distortion) adds its cotangents to the rows the blend backward has filled, in front of
    // everything that reads them: the ADC statistic below sees the term in columns 0 and 1
    if (c->distortion.armed) {
        if (const int rc = distortion_backward_of_forward(c)) return rc;
    }
    // the ADC statistic (gs_set_adc_stats), from the signed mean gradient in columns 0 and 1 -- the absolute sums under absgrad
    if (c->adcGradSum) {
        if (const int rc = launch_adc_accum(c, c->fwd.N, c->gradAcc16, c->fwd.radii, absgrad, gate, c->adcGradSum, c->adcCount,
                                            c->adcMaxRadius))
            return rc;
    }
    if (!absgrad) return GS_OK;
    c->absgradN = c->fwd.N;
    return c->gradNormAccum ? launch_absgrad_accum(c, c->fwd.N, gate, c->gradNormAccum) : GS_OK;
}

// the projection backward of an absgrad step adds nothing to the grad-norm accumulator: it sees none
struct AbsgradScope {
    gs_ctx* c;
    float* saved;
    explicit AbsgradScope(gs_ctx* ctx) : c(ctx), saved(ctx->gradNormAccum) { if (c->absgrad) c->gradNormAccum = nullptr; }
    ~AbsgradScope() { c->gradNormAccum = saved; }
};

// the gs_sh_grad_from_views* family's common arguments; own_bad / own_null: what the entry point's own arguments add to the
// first and to the null-buffer check
int sh_views_args(gs_ctx* c, const char* who, int N, int K, int R, const float* xyz, const float* color_cot_all,
                  const float* cam_centers, const float* dc, const float* rest, bool own_bad, bool own_null)
{
    if (N < 0 || K < 1 || R < 1 || R > 16 || !cam_centers || own_bad)
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": bad N/K/R");
    if ((c->modes.degree + 1) * (c->modes.degree + 1) > K) return fail(c, GS_ERR_SIZE_MISMATCH, "K smaller than (degree+1)^2");
    if (N > 0 && (!xyz || !color_cot_all || !dc || (K > 1 && !rest) || own_null))
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    return GS_OK;
}

// ... and their last check: the gathered blocks' layout, where gs_set_gathered_gate has described one
int sh_views_gate_layout(gs_ctx* c, const char* who, int N, int R)
{
    if (c->ccBlockFloats > 0 && (R != c->ccBlockCount || c->ccBlockFloats < 3LL * N + 1))
        return fail(c, GS_ERR_SIZE_MISMATCH, std::string(who) + ": R / N do not match the gs_set_gathered_gate layout");
    return GS_OK;
}

// the kernels move a wave's f_rest span as float4 when its row length L = 3 (K - 1) is a multiple of four (sh_rows_in /
// sh_rows_out / the kept registers): the tensor must then start on a 16-byte boundary.  Other row lengths go element by element
// (or through adam_rows' scalar head and tail) and may lie anywhere.  bases: the arenas the Adam forms address by one offset
int sh_rest_alignment(gs_ctx* c, const char* who, int N, int K, const float* rest, const float* params_base = nullptr,
                      const float* m_base = nullptr, const float* v_base = nullptr)
{
    if (((uintptr_t)params_base | (uintptr_t)m_base | (uintptr_t)v_base) & 15)
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": the parameter and moment arenas must be 16-byte aligned");
    if (N > 0 && K > 1 && ((3 * (K - 1)) & 3) == 0 && ((uintptr_t)rest & 15))
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": with 3 (K - 1) a multiple of four the f_rest tensor must be 16-byte aligned");
    return GS_OK;
}

// the SH tensors of a fused SH rebuild + Adam lie in [params_base, params_base + n_arena)
int sh_in_arena(gs_ctx* c, const char* who, int N, int K, const float* dc, const float* rest, const float* params_base,
                long long n_arena)
{
    const float* lo = params_base;
    const float* hi = params_base + n_arena;
    if (N > 0 && (dc < lo || dc + 3LL * N > hi || (K > 1 && (rest < lo || rest + 3LL * (K - 1) * N > hi))))
        return fail(c, GS_ERR_SIZE_MISMATCH, std::string(who) + ": the SH tensors do not lie in the arena");
    return GS_OK;
}

// the scratch image the loss reads under a per-view colour correction ([H, W, 3]): allocated once per ctx, by the
// correction's setter -- a step never allocates
int ensure_corrected_image(gs_ctx* c)
{
    return c->correctedImage ? GS_OK : ctx_alloc(c, &c->correctedImage, (size_t)3 * c->H * c->W);
}

// gs_copy_overflow_flag: a one-thread kernel, not hipMemcpyAsync -- the runtime's device-to-device copy is a blit kernel
// between two barrier packets (5.6 us + ~7 us of idle in front of the blend backward of every data-parallel step of the
// torch exchange, tools/trace_gaps.py)
__global__ void copy_word_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) { *dst = *src; }

// The op-level entry points see the caller's tile grid; under block lists (gs_ctx.h) the context's own fields describe the
// fused path's block grid, so they are swapped for the duration of the call.
struct RealGeomScope {
    gs_ctx* c;
    GsRealGeom saved;
    GsVirtGeom virt;
    explicit RealGeomScope(gs_ctx* ctx) : c(ctx)
    {
        if (!c || !c->virt.nbx) { c = nullptr; return; }
        saved.tileW = c->tileW; saved.tileH = c->tileH; saved.gridW = c->gridW; saved.gridH = c->gridH; saved.T = c->T;
        saved.tileBits = c->tileBits; saved.fast16 = c->fast16;
        virt = c->virt;
        c->tileW = c->real.tileW; c->tileH = c->real.tileH; c->gridW = c->real.gridW; c->gridH = c->real.gridH; c->T = c->real.T;
        c->tileBits = c->real.tileBits; c->fast16 = c->real.fast16;
        c->virt = GsVirtGeom();
    }
    ~RealGeomScope()
    {
        if (!c) return;
        c->tileW = saved.tileW; c->tileH = saved.tileH; c->gridW = saved.gridW; c->gridH = saved.gridH; c->T = saved.T;
        c->tileBits = saved.tileBits; c->fast16 = saved.fast16;
        c->virt = virt;
    }
};

}  // namespace

// the context's allocator (gs_mem.h): the one place the library's own buffers reach HIP's
static int hip_device_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
static int hip_device_free(void* p) { return (int)hipFree(p); }
static int hip_pinned_alloc(void** p, size_t bytes, unsigned flags) { return (int)hipHostMalloc(p, bytes, flags); }
static int hip_pinned_free(void* p) { return (int)hipHostFree(p); }
const GsMemBackend* gs_hip_mem_backend()
{
    static const GsMemBackend hip = {hip_device_alloc, hip_device_free, hip_pinned_alloc, hip_pinned_free};
    return &hip;
}

namespace gs {

int refuse_modes(gs_ctx* c, const char* who, std::initializer_list<GsMode> unserved)
{
    const GsRenderModes &now = c->modes, &ran = c->fwd.modes;
    const bool fwd = c->fwd.valid;
    for (const GsMode m : unserved) {
        const char* why = nullptr;
        switch (m) {
        case GS_MODE_POSE:
            if (now.poseDelta || ran.poseDelta) why = ": a pose correction is set (single-device steps only)";
            break;
        case GS_MODE_FILTER3D:
            if (now.filter3d || (fwd && ran.filter3d)) why = ": a 3-D filter is set (single-device steps only)";
            break;
        case GS_MODE_FISHEYE:
            if (now.fisheye || (fwd && ran.fisheye)) why = ": the fisheye camera model is set (gs_set_camera_model; pinhole cameras only)";
            break;
        case GS_MODE_ABSGRAD:
            if (c->absgrad) why = ": absgrad is on (gs_set_absgrad): only gs_render_backward and gs_render_backward_adam accumulate the "
                                  "absolute sums";
            break;
        case GS_MODE_SPARSE_ADAM:
            if (c->sparseAdam) why = ": sparse Adam is on (gs_set_sparse_adam): single-device steps through gs_render_backward_adam or "
                                     "gs_adam_step_visible only";
            break;
        case GS_MODE_ADC_STATS:
            if (c->adcGradSum) why = ": the ADC statistic is set (gs_set_adc_stats): only gs_render_backward and gs_render_backward_adam "
                                     "accumulate it";
            break;
        case GS_MODE_DISTORTION:
            if (c->distortion.armed) why = ": the distortion term is armed (gs_arm_distortion): only gs_render_backward and "
                                           "gs_render_backward_adam run its backward (single-device steps only)";
            break;
        }
        if (why) return fail(c, GS_ERR_INVALID_ARG, std::string(who) + why);
    }
    return GS_OK;
}

int forward_in_arena(gs_ctx* c, const char* who, const float* params_base, long long n_arena)
{
    const int N = c->fwd.N, K = c->fwd.K;
    const float* lo = params_base;
    const float* hi = params_base + n_arena;
    auto inside = [&](const float* p, long long n) { return n == 0 || (p >= lo && p + n <= hi); };
    if (inside(c->fwd.xyz, 3LL * N) && inside(c->fwd.fdc, 3LL * N) && inside(c->fwd.frest, 3LL * (K - 1) * N) &&
        inside(c->fwd.scales, 3LL * N) && inside(c->fwd.rot, 4LL * N) && inside(c->fwd.opacity, N))
        return GS_OK;
    return fail(c, GS_ERR_SIZE_MISMATCH, std::string(who) + ": the forward's tensors do not lie in the arena");
}

}  // namespace gs

#pragma GCC visibility push(default)
extern "C" {

int gs_abi_version(void) { return GSPLAT_ABI_VERSION; }

int gs_ctx_create(int device, int W, int H, int tile_w, int tile_h, int sh_degree, int white_bg, gs_ctx** out)
{
    if (!out) return GS_ERR_INVALID_ARG;
    *out = nullptr;
    if (W <= 0 || H <= 0 || tile_w <= 0 || tile_h <= 0 || sh_degree < 0 || sh_degree > 4) return GS_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return GS_ERR_NO_DEVICE;
    gs_ctx* c = new gs_ctx();
    c->mem.backend = gs_hip_mem_backend();
    c->device = device;
    c->W = W; c->H = H; c->tileW = tile_w; c->tileH = tile_h;
    c->gridW = (W + tile_w - 1) / tile_w; c->gridH = (H + tile_h - 1) / tile_h;
    c->T = c->gridW * c->gridH;
    c->modes.degree = c->maxDegree = sh_degree; c->whiteBg = white_bg ? 1 : 0;
    c->modes.bg.mode = c->whiteBg ? GS_BG_WHITE : GS_BG_BLACK;
    c->fast16 = (tile_w % 16 == 0) && (tile_h % 16 == 0);
    c->blocksX = gs_div_up(W, 16); c->blocksY = gs_div_up(H, 16);
    c->real.tileW = tile_w; c->real.tileH = tile_h; c->real.gridW = c->gridW; c->real.gridH = c->gridH; c->real.T = c->T;
    c->real.fast16 = c->fast16;
    {
        // Block lists (gs_ctx.h, GsVirtGeom): for a tile size that is not a multiple of 16 the fused path works on the grid
        // of 16 x 16 blocks enumerated per tile.  GSPLAT_BLOCK_LISTS=0 keeps round 3's form (tile lists + the generic blend
        // kernels that scan a tile's list per block) for A/B runs.
        const char* e = getenv("GSPLAT_BLOCK_LISTS");
        const int nbx = gs_div_up(tile_w, 16), nby = gs_div_up(tile_h, 16);
        if (!c->fast16 && !(e && atoi(e) == 0) && (long long)c->gridW * nbx <= 65535 && (long long)c->gridH * nby <= 65535) {
            c->virt.nbx = nbx; c->virt.nby = nby; c->virt.tw = tile_w; c->virt.th = tile_h;
            c->tileW = 16; c->tileH = 16;
            c->gridW *= nbx; c->gridH *= nby;
            c->T = c->gridW * c->gridH;
            c->fast16 = true;
            c->blocksX = c->gridW; c->blocksY = c->gridH;
        }
    }
    if (const char* e = getenv("GSPLAT_COLOUR_RIDERS")) c->colourRiders = atoi(e);      // tuning experiments (tools/rider_ab.py)
    if (const char* e = getenv("GSPLAT_FWD_WIDE")) c->fwdWide = atoi(e) < 0 ? -1 : atoi(e) != 0;
    if (const char* e = getenv("GSPLAT_FWD_QUEUES")) { const int q = atoi(e); if (q >= 1 && q <= (int)GS_QUEUES && !(q & (q - 1))) c->fwdQueues = q; }
    if (const char* e = getenv("GSPLAT_RIDER_SHARES")) {      // tuning experiments: permille of the colour units per host kernel
        // exactly GS_RIDE_HOSTS comma-separated values, in the enum's order (ss_hist, ss_scatter, wide_tile); anything else
        // is refused loudly -- a sweep that passes four values would measure other splits than the ones it prints
        int vals[GS_RIDE_HOSTS + 1], n = 0;
        for (const char* q = e; *q && n <= GS_RIDE_HOSTS; n++) {
            vals[n] = atoi(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        if (n == GS_RIDE_HOSTS) for (int i = 0; i < GS_RIDE_HOSTS; i++) c->riderShare[i] = vals[i];
        else fprintf(stderr, "gsplat: GSPLAT_RIDER_SHARES needs %d comma-separated values (got %s): ignored\n", GS_RIDE_HOSTS, e);
    }
    if (c->gridW > 65535 || c->gridH > 65535) { delete c; return GS_ERR_INVALID_ARG; }
    int bits = 1;
    while ((1LL << bits) < c->T) bits++;
    c->tileBits = bits;
    for (bits = 1; (1LL << bits) < c->real.T; bits++) {}
    c->real.tileBits = bits;
    auto bail = [&](int code) { gs_ctx_destroy(c); return code; };
    if (hipSetDevice(device) != hipSuccess) return bail(GS_ERR_HIP);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(GS_ERR_HIP);
    c->stream = c->own_stream;
    const size_t P = (size_t)W * H;
    c->numPixBlocks = c->blocksX * c->blocksY;
    c->opBlocks = c->real.fast16 ? c->numPixBlocks : c->real.T * gs_div_up(tile_w, 16) * gs_div_up(tile_h, 16);
    const size_t maxBlocks = (size_t)(c->opBlocks > c->numPixBlocks ? c->opBlocks : c->numPixBlocks);
    if (ctx_alloc(c, &c->blockWorkOwn, maxBlocks) || ctx_alloc(c, &c->blockOrder, maxBlocks + 8) || ctx_alloc(c, &c->fwdQueue, GS_QUEUES * GS_QUEUE_STRIDE) || ctx_alloc(c, &c->bwdQueue, GS_QUEUES * GS_QUEUE_STRIDE) ||
        ctx_alloc(c, &c->segBase, (size_t)c->numPixBlocks) || ctx_alloc(c, &c->finalT, P))
        return bail(GS_ERR_HIP);
    c->blockWork = c->blockWorkOwn;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            c->numCUs = prop.multiProcessorCount;
    }
    if (ctx_alloc(c, &c->superCut, (size_t)c->T + 16) || ctx_alloc(c, &c->tileRanges, (size_t)c->T * 2) || ctx_alloc(c, &c->tileCounts, (size_t)c->T) ||
        ctx_alloc(c, &c->lastContrib, P) ||
        ctx_alloc(c, &c->lossPartials, (size_t)(c->lossPartialBlocks = gs_div_up(W, 16) * gs_div_up(H, 16) * 3) * 4 + 16) || ctx_alloc(c, &c->windowDev, 121) ||
        ctx_alloc(c, &c->counters, GS_CNT_COUNT) || ctx_alloc(c, &c->rowTotal, 256) ||
        ctx_alloc(c, &c->sortBits, GS_SMALL_SORT_BLOCKS) || ctx_alloc(c, &c->wideTotal, GS_WIDE_BINS) ||
        ctx_alloc(c, &c->bucketStart, 520) || ctx_alloc(c, &c->sortSplit[0], 256) || ctx_alloc(c, &c->sortSplit[1], 256))
        return bail(GS_ERR_HIP);
    if (ctx_alloc_pinned(c, &c->countersHost, GS_CNT_COUNT)) return bail(GS_ERR_HIP);
    // the depth cuts' miss word: host memory the forward kernel writes directly, read after the fwdDone event
    if (ctx_alloc_pinned(c, &c->missHost, 16, hipHostMallocMapped)) return bail(GS_ERR_HIP);
    for (int i = 0; i < 16; i++) c->missHost[i] = 0;
    if (hipHostGetDevicePointer((void**)&c->missDev, c->missHost, 0) != hipSuccess) return bail(GS_ERR_HIP);
    if (hipEventCreateWithFlags(&c->fwdDone, hipEventDisableTiming) != hipSuccess) return bail(GS_ERR_HIP);
    float win[121];
    gs_ssim_window(11, 1.5f, win);
    if (hipMemcpy(c->windowDev, win, sizeof win, hipMemcpyHostToDevice) != hipSuccess) return bail(GS_ERR_HIP);
    if (hipMemset(c->counters, 0, sizeof(uint32_t) * GS_CNT_COUNT) != hipSuccess) return bail(GS_ERR_HIP);
    if (hipMemset(c->tileRanges, 0, sizeof(uint32_t) * 2 * c->T) != hipSuccess) return bail(GS_ERR_HIP);
    c->adamGate = c->counters + GS_CNT_OVERFLOW;
    *out = c;
    return GS_OK;
}

int gs_ctx_destroy(gs_ctx* c)
{
    if (!c) return GS_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)gs_dp_shutdown(c);
    c->mem.freeAll();      // every device and pinned buffer the context still owns
    for (auto& e : c->profPool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (c->fwdDone) (void)hipEventDestroy(c->fwdDone);
    if (c->densifyDone) (void)hipEventDestroy(c->densifyDone);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return GS_OK;
}

int gs_ctx_set_stream(gs_ctx* c, void* hip_stream)
{
    if (!c) return GS_ERR_INVALID_ARG;
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)hip_stream;
    return GS_OK;
}

int gs_ctx_reserve(gs_ctx* c, int max_gaussians, long long max_pairs)
{
    if (!c || max_gaussians < 0 || max_pairs < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_reserve: negative size");
    (void)hipSetDevice(c->device);
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));      // a pending overflow report lands before it is cleared
    if (c->missHost[4] == 2u || c->arenaRegrowPending) {
        // the last forward ran out of checkpoint slots: its waves kept counting, so static part + counter is the need
        uint32_t parts[8], used = 0;
        GS_HIP_CHECK(c, hipMemcpy(parts, c->counters + GS_CNT_QSLOTS, sizeof parts, hipMemcpyDeviceToHost));
        // (what the waves drew from the eight parts together.  A draw that does not fit its part is given back (atomicSub),
        // and once every part is empty a wave keeps counting on its own part what it would have drawn, so the sum is what
        // was drawn + what was wanted and not had.  Between a failed draw's add and its sub another wave can see the
        // counter inflated and take a part that still has room for empty -- for good: partsEmpty is sticky per wave.  The
        // cost is a regrow a little early on an arena that is nearly full, never a wrong result; accepted.)
        for (uint32_t x : parts) used += x;
        // (counted in slots of that forward's planes; the arena is sized in five-plane slots)
        const long long need5 = (((long long)used + c->fwd.qslotStatic) * c->fwd.statePlanes + 4) / 5;
        c->qslotWanted = need5 + need5 / 2 + 4096;
        // the counters are the LAST forward's, which need not be the one that ran out (a report may be several forwards
        // old by the time the host acts on it): a pending regrow always grows the arena, by half at least
        const long long half = c->qslotCap + c->qslotCap / 2;
        if (c->qslotWanted < half) c->qslotWanted = half;
    }
    c->reserving = max_pairs > 0;      // (sizes the checkpoint arena for a reserve, ensure_arena)
    int rc = ensure_capacity(c, max_gaussians, max_pairs);
    if (rc == GS_OK) rc = ensure_arena(c);
    c->reserving = false;
    if (rc == GS_OK) {
        // (only now: a ctx whose allocation failed must not believe in a reserve it does not hold)
        if (max_pairs > 0) c->pairsReserved = true;
        c->missHost[4] = 0; c->arenaRegrowPending = false;
    }
    return rc;
}

size_t gs_workspace_bytes(const gs_ctx* c) { return c ? c->mem.deviceBytes : 0; }

int gs_sync(gs_ctx* c)
{
    if (!c) return GS_ERR_INVALID_ARG;
    const int rc = read_counters(c);
    if (rc) return rc;
    if (c->missHost[4]) {            // an earlier forward's overflow nobody has been told about yet
        const uint32_t need = c->missHost[5];
        const int orc = overflow_error(c, need);
        if (c->missHost[4] == 2u) { c->arenaRegrowPending = true; c->fwd.arenaOverflow = true; }
        c->missHost[4] = 0;
        return orc;
    }
    if (c->countersHost[GS_CNT_OVERFLOW]) return overflow_error(c);
    return GS_OK;
}

int gs_overflow_pending(gs_ctx* c, uint32_t out[2])
{
    if (!c || !out) return GS_ERR_INVALID_ARG;
    out[0] = c->missHost ? c->missHost[4] : 0u;
    out[1] = c->missHost ? c->missHost[5] : 0u;
    if (out[0] == 0u && c->arenaRegrowPending) out[0] = 2u;
    return GS_OK;
}

int gs_wait(gs_ctx* c)
{
    if (!c) return GS_ERR_INVALID_ARG;
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

const char* gs_last_error(const gs_ctx* c) { return c ? c->err.c_str() : "null context"; }

// ---- projection -------------------------------------------------------------------------------
int gs_projection_forward(gs_ctx* c, int N, int K, const float* scales, const float* rotations, const float* means3d,
                          const float* shs, const gs_camera* cam, float* means2d, float* depths, float* color,
                          float* cov2d, float* conic, float* radii, float* rect_min, float* rect_max)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || K < 1 || !cam) return fail(c, GS_ERR_INVALID_ARG, "gs_projection_forward: bad N/K/cam");
    if ((c->modes.degree + 1) * (c->modes.degree + 1) > K) return fail(c, GS_ERR_SIZE_MISMATCH, "K smaller than (degree+1)^2");
    if (N > 0 && (!scales || !rotations || !means3d || !shs || !means2d || !depths || !color || !cov2d || !conic ||
                  !radii || !rect_min || !rect_max))
        return fail(c, GS_ERR_INVALID_ARG, "gs_projection_forward: null buffer");
    return launch_projection_forward(c, N, K, scales, rotations, means3d, shs, make_cam(cam, c->W, c->H), means2d,
                                     depths, color, cov2d, conic, radii, rect_min, rect_max);
}

int gs_projection_backward(gs_ctx* c, int N, int K, const float* scales, const float* rotations,
                           const float* means3d, const float* shs, const gs_camera* cam, const float* cot_depths,
                           const float* cot_means2d, const float* cot_cov2d, const float* cot_color,
                           const float* cot_conic, float* grad_scales, float* grad_rotations, float* grad_means3d,
                           float* grad_shs, float* grad_cam_center_point)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || K < 1 || !cam) return fail(c, GS_ERR_INVALID_ARG, "gs_projection_backward: bad N/K/cam");
    if ((c->modes.degree + 1) * (c->modes.degree + 1) > K) return fail(c, GS_ERR_SIZE_MISMATCH, "K smaller than (degree+1)^2");
    if (N > 0 && (!scales || !rotations || !means3d || !shs || !cot_depths || !cot_means2d || !cot_cov2d ||
                  !cot_color || !cot_conic || !grad_scales || !grad_rotations || !grad_means3d || !grad_shs ||
                  !grad_cam_center_point))
        return fail(c, GS_ERR_INVALID_ARG, "gs_projection_backward: null buffer");
    return launch_projection_backward(c, N, K, scales, rotations, means3d, shs, make_cam(cam, c->W, c->H), cot_depths,
                                      cot_means2d, cot_cov2d, cot_color, cot_conic, grad_scales, grad_rotations,
                                      grad_means3d, grad_shs, grad_cam_center_point);
}

// ---- binning ------------------------------------------------------------------------------------
int gs_tile_bin(gs_ctx* c, int N, const float* rect_min, const float* rect_max, const float* radii,
                const float* depths)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!rect_min || !rect_max || !radii || !depths)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_tile_bin: bad arguments");
    return gs_tile_bin_cut(c, N, rect_min, rect_max, radii, depths, nullptr);
}

int gs_tile_bin_cut(gs_ctx* c, int N, const float* rect_min, const float* rect_max, const float* radii,
                    const float* depths, const uint32_t* tile_cuts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!rect_min || !rect_max || !radii || !depths)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_tile_bin: bad arguments");
    RealGeomScope real(c);
    c->binIsBlockLists = false;
    c->dropBlocks = 0; c->superCutReady = false;      // (no fused projection in front of this binning)
    c->fwd.valid = false;
    c->fwd.cutsActive = false;          // a fused forward's cuts never leak into an op-level binning
    c->fwd.bwdPrepared = false;
    c->opCuts = N > 0 ? tile_cuts : nullptr;
    const bool reserved = c->pairsReserved && c->capN >= N;
    const int rc = bin_with_capacity(c, N, reserved, true, [&]() { return launch_bin_prep(c, N, rect_min, rect_max, radii, depths); });
    c->opCuts = nullptr;
    return rc;
}

int gs_tile_bin_info(gs_ctx* c, uint32_t* M, uint32_t* B)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_info: no binning on this context");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_info: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    int rc = launch_tile_counts(c);
    if (rc) return rc;
    if ((rc = read_counters(c))) return rc;
    if (c->countersHost[GS_CNT_OVERFLOW]) return overflow_error(c);
    if (M) *M = c->countersHost[GS_CNT_M];
    if (B) *B = c->countersHost[GS_CNT_B];
    return GS_OK;
}

int gs_tile_bin_views(gs_ctx* c, const uint32_t** sorted_gauss_idx, const uint32_t** tile_ranges,
                      const uint32_t** tile_counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_views: no binning on this context");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_views: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    if (tile_counts) {
        const int rc = launch_tile_counts(c);
        if (rc) return rc;
        *tile_counts = c->tileCounts;
    }
    if (sorted_gauss_idx) {
        const int rc = ensure_plain_sorted(c);
        if (rc) return rc;
        *sorted_gauss_idx = c->sortedIdx;
    }
    if (tile_ranges) *tile_ranges = c->tileRanges;
    return GS_OK;
}

int gs_tile_bin_export(gs_ctx* c, uint32_t* sorted_gauss_idx, uint32_t* tile_ranges, uint32_t* tile_counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_export: no binning on this context");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_tile_bin_export: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    int rc;
    if ((rc = launch_tile_counts(c))) return rc;
    if (sorted_gauss_idx && (rc = ensure_plain_sorted(c))) return rc;
    if ((rc = read_counters(c))) return rc;
    if (c->countersHost[GS_CNT_OVERFLOW]) return overflow_error(c);
    const size_t M = c->countersHost[GS_CNT_M];
    if (sorted_gauss_idx && M)
        GS_HIP_CHECK(c, hipMemcpyAsync(sorted_gauss_idx, c->sortedIdx, M * 4, hipMemcpyDeviceToDevice, c->stream));
    if (tile_ranges)
        GS_HIP_CHECK(c, hipMemcpyAsync(tile_ranges, c->tileRanges, (size_t)c->T * 8, hipMemcpyDeviceToDevice, c->stream));
    if (tile_counts)
        GS_HIP_CHECK(c, hipMemcpyAsync(tile_counts, c->tileCounts, (size_t)c->T * 4, hipMemcpyDeviceToDevice, c->stream));
    return GS_OK;
}

int gs_build_packed_tile_indices(gs_ctx* c, uint32_t B, int32_t* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_build_packed_tile_indices: no binning on this context");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_build_packed_tile_indices: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    if (B > 0 && !out) return fail(c, GS_ERR_INVALID_ARG, "gs_build_packed_tile_indices: null output");
    const int rc = ensure_plain_sorted(c);
    if (rc) return rc;
    return launch_build_packed_tile_indices(c, B, out);
}

// ---- packing / blending ---------------------------------------------------------------------------
int gs_pack_gaussians(gs_ctx* c, int N, const float* means2d, const float* conic, const float* color,
                      const float* opacity, const float* depths, float* packed)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!means2d || !conic || !color || !opacity || !depths || !packed)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_pack_gaussians: bad arguments");
    return launch_pack_gaussians(c, N, means2d, conic, color, opacity, depths, packed);
}

int gs_blend_forward(gs_ctx* c, int N, const float* packed, float* out_color, float* out_depth, float* out_alpha,
                     uint32_t* last_contrib)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_forward: call gs_tile_bin first");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_forward: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    if (N != c->binN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_blend_forward: N differs from the binned N");
    if (!out_color || !out_depth || !out_alpha || !last_contrib || (N > 0 && !packed))
        return fail(c, GS_ERR_INVALID_ARG, "gs_blend_forward: null buffer");
    // the op-level blend overwrites the ctx's packed records (and, backward, its accumulator): whatever a fused forward
    // saved on this ctx -- incl. a backward preparation the loss kernel carried along -- is gone
    c->fwd.valid = false; c->fwd.bwdPrepared = false;
    int rc = launch_pack11_to_12(c, N, packed);
    if (rc) return rc;
    return launch_blend_forward(c, c->modes.bg, out_color, out_depth, out_alpha, last_contrib);
}

int gs_blend_backward(gs_ctx* c, int N, const float* packed, const float* cot_color, const float* cot_depth,
                      const float* cot_alpha, const float* out_color, const float* out_depth, const float* out_alpha,
                      const uint32_t* last_contrib, float* grad_packed)
{
    (void)out_color; (void)out_depth;   // undone by the reference but never read back
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_backward: call gs_tile_bin first");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_backward: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    if (N != c->binN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_blend_backward: N differs from the binned N");
    if (!cot_color || !out_alpha || !last_contrib || (N > 0 && (!packed || !grad_packed)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_blend_backward: null buffer");
    c->fwd.valid = false; c->fwd.bwdPrepared = false;      // as gs_blend_forward
    c->absgradN = -1;                                       // (the accumulator's rows are rewritten)
    int rc = launch_pack11_to_12(c, N, packed);
    if (rc) return rc;
    if ((rc = launch_blend_backward(c, c->modes.bg, N, cot_color, cot_depth, cot_alpha, out_alpha, last_contrib))) return rc;
    return launch_gradacc_to_packed11(c, N, grad_packed);
}

int gs_blend_contrib(gs_ctx* c, int N, const float* packed, float* max_w, float* sum_w)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_contrib: call gs_tile_bin first");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, "gs_blend_contrib: the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    RealGeomScope real(c);
    if (N != c->binN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_blend_contrib: N differs from the binned N");
    if ((!max_w && !sum_w) || (N > 0 && !packed)) return fail(c, GS_ERR_INVALID_ARG, "gs_blend_contrib: null buffer (one of max_w, sum_w at least)");
    c->fwd.valid = false; c->fwd.bwdPrepared = false;      // as gs_blend_forward: the ctx's packed records are overwritten
    int rc = launch_pack11_to_12(c, N, packed);
    if (rc) return rc;
    return launch_blend_contrib(c, max_w, sum_w);
}

// the op-level feature pair's preconditions: gs_blend_contrib's, and a channel count in range
static int blend_features_preflight(gs_ctx* c, const char* who, int N, int C, const float* packed, const void* in, const void* out)
{
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, std::string(who) + ": call gs_tile_bin first");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, std::string(who) + ": the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    if (N != c->binN) return fail(c, GS_ERR_SIZE_MISMATCH, std::string(who) + ": N differs from the binned N");
    if (C < 1 || C > GS_MAX_FEATURE_CHANNELS) return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": C must be in [1, GS_MAX_FEATURE_CHANNELS]");
    if (!in || !out || (N > 0 && !packed)) return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    return GS_OK;
}

int gs_blend_features(gs_ctx* c, int N, int C, const float* packed, const float* features, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int prc = blend_features_preflight(c, "gs_blend_features", N, C, packed, features, out)) return prc;
    RealGeomScope real(c);
    c->fwd.valid = false; c->fwd.bwdPrepared = false;      // as gs_blend_forward: the ctx's packed records are overwritten
    if (const int rc = launch_pack11_to_12(c, N, packed)) return rc;
    return launch_blend_features(c, C, features, out);
}

int gs_blend_features_backward(gs_ctx* c, int N, int C, const float* packed, const float* cot, float* grad_features)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int prc = blend_features_preflight(c, "gs_blend_features_backward", N, C, packed, cot, grad_features)) return prc;
    RealGeomScope real(c);
    c->fwd.valid = false; c->fwd.bwdPrepared = false;
    if (const int rc = launch_pack11_to_12(c, N, packed)) return rc;
    return launch_blend_features_backward(c, C, cot, grad_features);
}

int gs_feature_channel_group(void) { return feature_channel_group(); }

// ---- depth distortion loss (include/gsplat.h gs_blend_distortion ..; distortion.hip) -----------------------------------------
// what every distortion entry point asks of its params
static int distortion_params_check(gs_ctx* c, const char* who, const gs_distortion_params* p)
{
    if (!p) return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": null params");
    if (p->map != GS_DISTORTION_NDC && p->map != GS_DISTORTION_LINEAR)
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": map is GS_DISTORTION_NDC or GS_DISTORTION_LINEAR");
    if (p->map == GS_DISTORTION_NDC && !(isfinite(p->near) && isfinite(p->far) && p->near > 0.0f && p->far > p->near))
        return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": near and far are finite with 0 < near < far");
    return GS_OK;
}

// the op-level pair's preconditions: gs_blend_contrib's
static int blend_distortion_preflight(gs_ctx* c, const char* who, int N, const float* packed, const gs_distortion_params* p)
{
    if (!c->binValid) return fail(c, GS_ERR_NO_FORWARD, std::string(who) + ": call gs_tile_bin first");
    if (c->binIsBlockLists) return fail(c, GS_ERR_NO_FORWARD, std::string(who) + ": the last binning on this context was a fused forward's block lists (tile size not a multiple of 16); call gs_tile_bin");
    if (N != c->binN) return fail(c, GS_ERR_SIZE_MISMATCH, std::string(who) + ": N differs from the binned N");
    if (N > 0 && !packed) return fail(c, GS_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    return distortion_params_check(c, who, p);
}

int gs_blend_distortion(gs_ctx* c, int N, const float* packed, const gs_distortion_params* params, float* out_distort,
                        float* out_totals)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int prc = blend_distortion_preflight(c, "gs_blend_distortion", N, packed, params)) return prc;
    if (!out_distort || !out_totals) return fail(c, GS_ERR_INVALID_ARG, "gs_blend_distortion: null buffer");
    RealGeomScope real(c);
    c->fwd.valid = false; c->fwd.bwdPrepared = false;      // as gs_blend_forward: the ctx's packed records are overwritten
    if (const int rc = launch_pack11_to_12(c, N, packed)) return rc;
    return launch_blend_distortion(c, *params, out_distort, out_totals);
}

int gs_blend_distortion_backward(gs_ctx* c, int N, const float* packed, const gs_distortion_params* params, const float* cot,
                                 const float* totals, float* rows16)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int prc = blend_distortion_preflight(c, "gs_blend_distortion_backward", N, packed, params)) return prc;
    if (!cot || !totals || (N > 0 && !rows16)) return fail(c, GS_ERR_INVALID_ARG, "gs_blend_distortion_backward: null buffer");
    RealGeomScope real(c);
    c->fwd.valid = false; c->fwd.bwdPrepared = false;
    if (const int rc = launch_pack11_to_12(c, N, packed)) return rc;
    return launch_blend_distortion_backward(c, *params, cot, totals, rows16);
}

int gs_distortion_loss(gs_ctx* c, float weight, long long n_pixels, const float* distort, const unsigned char* mask, float* loss,
                       float* cot_out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n_pixels < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_distortion_loss: negative n_pixels");
    if (!isfinite(weight)) return fail(c, GS_ERR_INVALID_ARG, "gs_distortion_loss: weight is finite");
    if (!distort || !loss || !cot_out) return fail(c, GS_ERR_INVALID_ARG, "gs_distortion_loss: null buffer");
    if (!c->distortionWs) {      // the first call: a step never allocates after it
        GS_HIP_CHECK(c, hipSetDevice(c->device));
        if (const int rc = ctx_alloc(c, &c->distortionWs, (size_t)distortion_loss_ws_doubles())) return rc;
    }
    GsStageTimer t(c, GS_STAGE_LOSS);
    return launch_distortion_loss(c, weight, n_pixels, distort, mask, loss, cot_out);
}

// ---- SSIM -----------------------------------------------------------------------------------------
int gs_ssim_window(int K, float sigma, float* window)
{
    if (K <= 0 || K > 32 || !window) return GS_ERR_INVALID_ARG;
    float g[32];
    const float center = (float)K / 2.0f;    // 5.5 for K = 11: the reference's off-centre window
    float sum = 0.0f;
    for (int x = 0; x < K; x++) {
        const float d = (float)x - center;
        g[x] = expf(-(d * d) / (2.0f * (sigma * sigma)));
        sum += g[x];
    }
    for (int x = 0; x < K; x++) g[x] = g[x] / sum;
    for (int i = 0; i < K; i++)
        for (int j = 0; j < K; j++) window[i * K + j] = g[i] * g[j];
    return GS_OK;
}

int gs_ssim_forward(gs_ctx* c, int H, int W, int C, int K, const float* img1, const float* img2, const float* window,
                    float* out_ssim, float* out_mu1, float* out_mu2, float* out_sigma1, float* out_sigma2,
                    float* out_sigma12)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (H < 0 || W < 0 || C < 0 || K <= 0 || K > 32) return fail(c, GS_ERR_INVALID_ARG, "gs_ssim_forward: bad shape");
    if (C > 65535) return fail(c, GS_ERR_INVALID_ARG, "gs_ssim_forward: too many channels");
    if ((size_t)H * W * C > 0 && (!img1 || !img2 || !window || !out_ssim || !out_mu1 || !out_mu2 || !out_sigma1 ||
                                  !out_sigma2 || !out_sigma12))
        return fail(c, GS_ERR_INVALID_ARG, "gs_ssim_forward: null buffer");
    return launch_ssim_forward(c, H, W, C, K, img1, img2, window, out_ssim, out_mu1, out_mu2, out_sigma1, out_sigma2,
                               out_sigma12);
}

int gs_ssim_backward(gs_ctx* c, int H, int W, int C, int K, const float* grad_out, const float* img1,
                     const float* img2, const float* window, const float* mu1, const float* mu2, const float* sigma1,
                     const float* sigma2, const float* sigma12, float* grad_img1, float* grad_img2)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (H < 0 || W < 0 || C < 0 || K <= 0 || K > 32) return fail(c, GS_ERR_INVALID_ARG, "gs_ssim_backward: bad shape");
    if ((size_t)H * W * C > 0 && (!grad_out || !img1 || !img2 || !window || !mu1 || !mu2 || !sigma1 || !sigma2 ||
                                  !sigma12 || !grad_img1 || !grad_img2))
        return fail(c, GS_ERR_INVALID_ARG, "gs_ssim_backward: null buffer");
    return launch_ssim_backward(c, H, W, C, K, grad_out, 0.0f, img1, img2, window, mu1, mu2, sigma1, sigma2, sigma12,
                                grad_img1, grad_img2, 0.0f);
}

// ---- fused path -------------------------------------------------------------------------------------
int gs_render_forward(gs_ctx* c, int N, int K, const float* xyz, const float* features_dc,
                      const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                      const gs_camera* cam, float* out_color, float* out_depth, float* out_alpha, float* radii)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || K < 1 || !cam) return fail(c, GS_ERR_INVALID_ARG, "gs_render_forward: bad N/K/cam");
    if ((c->modes.degree + 1) * (c->modes.degree + 1) > K) return fail(c, GS_ERR_SIZE_MISMATCH, "K smaller than (degree+1)^2");
    // (out_depth may be NULL: no depth image is computed, and the backward of this forward takes no depth cotangent)
    if (!out_color || !out_alpha) return fail(c, GS_ERR_INVALID_ARG, "gs_render_forward: null output");
    if (N > 0 && (!xyz || !features_dc || (K > 1 && !features_rest) || !scales || !rotation || !opacity))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_forward: null parameter tensor");
    if (c->modes.fisheye && c->modes.poseDelta)
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_forward: the fisheye camera model has no pose refinement (gs_set_pose_correction is set)");
    if (c->modes.fisheye && c->modes.filter3d)
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_forward: the fisheye camera model has no 3-D filter (gs_set_filter3d is set)");
    c->fwd.valid = false;
    c->visN = -1;
    c->distortion.armed = false;         // (gs_arm_distortion arms the term for one forward)
    const bool keepRadii = c->sparseAdam || c->adcGradSum != nullptr;      // (the ADC statistic reads the radii in the backward)
    if (keepRadii && N > c->visCap) {           // sparse Adam's mask and radii: grown by the first forward that needs more rows
        if (const int arc = ctx_grow_pair(c, &c->visMask, &c->visRadii, &c->visCap, N > c->capN ? N : c->capN)) return arc;
    }
    if (keepRadii && !radii) radii = c->visRadii;          // (the mask is taken from the radii the projection writes)
    c->binIsBlockLists = c->virt.nbx != 0;
    const bool reserved = c->pairsReserved && c->capN >= N;
    if (reserved) { const int orc = deferred_overflow(c); if (orc) return orc; }
    // a forward under depth cuts that nobody asked about: let its miss word settle before it is reused
    if (c->fwd.cutsActive && !c->fwd.missChecked) GS_HIP_CHECK(c, hipEventSynchronize(c->fwdDone));
    c->fwd.missed = false;
    c->fwd.bwdPrepared = false;
    c->fwd.arenaOverflow = false;
    c->fwd.cutStore = c->cutStore;
    c->fwd.cutsActive = c->cutStore != nullptr && c->allowCuts && N > 0;
    c->fwd.missChecked = !c->fwd.cutsActive;
    if (c->fwd.cutsActive) c->missHost[0] = 0;
    const CamParams cp = make_cam(cam, c->W, c->H);
    if (c->modes.poseDelta) {         // pose refinement: the corrected camera, composed on the device, for every kernel of this step
        if (const int arc = ctx_grow(c, &c->posePartials, &c->posePartialsCap, pose_partials_floats(N))) return arc;
        if (const int prc = launch_pose_camera(c, cp, c->modes.poseDelta)) return prc;
    }
    c->segBaseWanted = c->fast16 && N > 0;
    c->segBaseDone = false;
    c->fwdPairNow = c->fast16 && blend_forward_v2_pair_decide(c);
    int rc = bin_with_capacity(c, N, reserved, !c->fast16, [&]() {
        return launch_projection_fused_forward(c, N, K, xyz, features_dc, features_rest, scales, rotation, opacity, cp,
                                               radii);
    });
    c->segBaseWanted = false;
    if (rc) { c->rider.on = false; return rc; }
    if (c->rider.on && c->rider.next < c->rider.total) {
        GsStageTimer t(c, GS_STAGE_PROJ_FWD, true);      // the colour units still outstanding belong to the projection
        if ((rc = launch_colour_rest(c))) return rc;
    }
    c->rider.on = false;
    {
        GsStageTimer t(c, GS_STAGE_BLEND_FWD);
        rc = c->fast16 ? launch_blend_forward_v2(c, out_color, out_depth, out_alpha)
                       : launch_blend_forward(c, c->modes.bg, out_color, out_depth, out_alpha, c->lastContrib);
        if (rc) return rc;
    }
    if (c->fwd.cutsActive) GS_HIP_CHECK(c, hipEventRecord(c->fwdDone, c->stream));
    c->fwd.valid = true;
    c->absgradN = -1;                   // (the next loss or backward clears the rows gs_get_absgrad would read)
    c->fwd.blendBackwardDone = false;
    c->fwd.consumed = false;
    c->fwd.blockWork = c->blockWork;
    c->fwd.N = N; c->fwd.K = K;
    c->fwd.xyz = xyz; c->fwd.fdc = features_dc; c->fwd.frest = features_rest; c->fwd.scales = scales;
    c->fwd.rot = rotation; c->fwd.opacity = opacity;
    c->fwd.outColor = out_color; c->fwd.outDepth = out_depth; c->fwd.outAlpha = out_alpha;
    c->fwd.cam = cp;
    c->fwd.modes = c->modes;      // whole: what this forward ran under is what its backward runs under
    c->fwd.radii = keepRadii ? radii : nullptr;      // (a caller's buffer is remembered only where a backward will read it)
    if (c->sparseAdam) c->visN = N;
    return GS_OK;
}

// ---- sparse Adam (include/gsplat.h gs_set_sparse_adam; projection.hip proj_bwd_fused_*sparse_kernel, optim.hip) -------------
int gs_set_sparse_adam(gs_ctx* c, int enable)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (enable != 0 && enable != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_set_sparse_adam: enable is 0 or 1");
    if (enable && c->mcmcOn)
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_sparse_adam: the MCMC strategy is set (its noise and regularisers act on every Gaussian)");
    if (enable && c->modes.filter3d) return fail(c, GS_ERR_INVALID_ARG, "gs_set_sparse_adam: a 3-D filter is set (gs_set_filter3d)");
    // (the mask of the last forward made under the setting stays readable when the setting goes off: every forward drops it first)
    c->sparseAdam = enable == 1;
    return GS_OK;
}

int gs_get_visibility(gs_ctx* c, int N, unsigned char* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (c->visN < 0)
        return fail(c, GS_ERR_NO_FORWARD, "gs_get_visibility: the last gs_render_forward was not made with sparse Adam on (gs_set_sparse_adam)");
    if (N != c->visN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_get_visibility: N differs from the forward's N");
    if (N > 0 && !out) return fail(c, GS_ERR_INVALID_ARG, "gs_get_visibility: null buffer");
    if (N > 0) GS_HIP_CHECK(c, hipMemcpyAsync(out, c->visMask, (size_t)N, hipMemcpyDeviceToDevice, c->stream));
    return GS_OK;
}

int gs_set_absgrad(gs_ctx* c, int enable)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (enable != 0 && enable != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_set_absgrad: enable is 0 or 1");
    if (enable && !c->fast16)
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_absgrad: this context's tile size is served by the generic blend kernels, which "
                                           "have no absolute sums");
    if ((enable == 1) != c->absgrad) c->absgradN = -1;
    c->absgrad = enable == 1;
    return GS_OK;
}

int gs_get_absgrad(gs_ctx* c, int N, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->absgrad || c->absgradN < 0)
        return fail(c, GS_ERR_NO_FORWARD, "gs_get_absgrad: no gs_render_backward / gs_render_backward_adam with absgrad on since "
                                          "gs_set_absgrad (or another forward or backward has run since)");
    if (N != c->absgradN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_get_absgrad: N differs from the backward's N");
    if (N > 0 && !out) return fail(c, GS_ERR_INVALID_ARG, "gs_get_absgrad: null buffer");
    return launch_absgrad_copy(c, N, out);
}

// ---- adaptive density control (include/gsplat.h gs_set_adc_stats; adc.hip) ---------------------------------------------------
int gs_set_adc_stats(gs_ctx* c, float* grad_sum, float* count, float* max_radius)
{
    if (!c) return GS_ERR_INVALID_ARG;
    const int given = (grad_sum != nullptr) + (count != nullptr) + (max_radius != nullptr);
    if (given != 0 && given != 3) return fail(c, GS_ERR_INVALID_ARG, "gs_set_adc_stats: all three accumulators, or all three NULL");
    if (given && !c->fast16)
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_adc_stats: this context's tile size is served by the generic blend kernels, whose "
                                           "backward leaves no gradient rows");
    c->adcGradSum = grad_sum;
    c->adcCount = count;
    c->adcMaxRadius = max_radius;
    return GS_OK;
}

int gs_adc_accumulate(gs_ctx* c, int N, const float* rows16, const float* radii, int use_abs, float* grad_sum, float* count,
                      float* max_radius)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (use_abs != 0 && use_abs != 1)) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_accumulate: bad N / use_abs");
    if (N > 0 && (!rows16 || !radii || !grad_sum || !count || !max_radius))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_accumulate: null buffer");
    if ((uintptr_t)rows16 & 7) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_accumulate: rows16 must be 8-byte aligned");
    return launch_adc_accum(c, N, rows16, radii, use_abs == 1, nullptr, grad_sum, count, max_radius);
}

int gs_adc_classify(gs_ctx* c, int N, const float* grad_sum, const float* count, const float* max_radius, const float* scales,
                    int scale_stride, const float* opacity, const gs_adc_params* params, int allow_densify, int size_prune,
                    int* actions, int* output_counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || scale_stride < 3 || !params) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_classify: bad N / scale_stride / params");
    if (N > 0 && (!grad_sum || !count || !max_radius || !scales || !opacity || !actions || !output_counts))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_classify: null buffer");
    const gs_adc_params& p = *params;
    if (!(p.grad_threshold >= 0.0f) || !(p.percent_dense >= 0.0f) || !(p.prune_world >= 0.0f) || !(p.scene_extent > 0.0f) ||
        !isfinite(p.scene_extent) || !(p.min_opacity >= 0.0f) || p.max_screen_size != p.max_screen_size)
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_classify: thresholds must be >= 0 (scene_extent > 0 and finite; max_screen_size "
                                           "any number, <= 0 for no screen test)");
    return launch_adc_classify(c, N, grad_sum, count, max_radius, scales, scale_stride, opacity, p.grad_threshold,
                               p.percent_dense * p.scene_extent, p.min_opacity, p.max_screen_size, p.prune_world * p.scene_extent,
                               allow_densify != 0, size_prune != 0, actions, output_counts);
}

int gs_adc_gather(gs_ctx* c, int total, int K, const float* xyz, const float* features_dc, const float* features_rest,
                  const float* scales, const float* rotation, const float* opacity, const int* gather_indices, const int* noise_mode,
                  const float* noise, int revised_opacity, float* out_xyz, float* out_features_dc, float* out_features_rest,
                  float* out_scales, float* out_rotation, float* out_opacity)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (total < 0 || K < 1 || (revised_opacity != 0 && revised_opacity != 1))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather: bad total / K / revised_opacity");
    if (total > 0 && (!xyz || !features_dc || !scales || !rotation || !opacity || !gather_indices || !noise_mode || !noise ||
                      !out_xyz || !out_features_dc || !out_scales || !out_rotation || !out_opacity ||
                      (K > 1 && (!features_rest || !out_features_rest))))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather: null buffer");
    return launch_adc_gather(c, total, K, xyz, features_dc, features_rest, scales, rotation, opacity, gather_indices, noise_mode,
                             noise, revised_opacity, out_xyz, out_features_dc, out_features_rest, out_scales, out_rotation,
                             out_opacity);
}

int gs_adc_gather_moments(gs_ctx* c, int total, int K, const int* gather_indices, const int* noise_mode, const int* actions,
                          const float* const in[6], float* const out[6])
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (total < 0 || K < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather_moments: bad total / K");
    if (!in || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather_moments: null tensor table");
    if (total > 0) {
        if (!gather_indices || !noise_mode || !actions) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather_moments: null buffer");
        for (int t = 0; t < 6; t++)
            if ((t != 2 || K > 1) && (!in[t] || !out[t])) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_gather_moments: null buffer");
    }
    return launch_adc_gather_moments(c, total, K, gather_indices, noise_mode, actions, in, out);
}

int gs_adc_reset_opacity(gs_ctx* c, int N, float* opacity, float* m_opacity, float* v_opacity, float reset_value)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || !(reset_value > 0.0f && reset_value < 1.0f))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adc_reset_opacity: bad N, or reset_value not in (0, 1)");
    if (N > 0 && (!opacity || !m_opacity || !v_opacity)) return fail(c, GS_ERR_INVALID_ARG, "gs_adc_reset_opacity: null buffer");
    const double rv = (double)reset_value;
    return launch_adc_reset_opacity(c, N, opacity, m_opacity, v_opacity, (float)log(rv / (1.0 - rv)));
}

int gs_set_antialiasing(gs_ctx* c, int enable)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (enable != 0 && enable != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_set_antialiasing: enable is 0 or 1");
    c->modes.antialias = enable == 1;
    return GS_OK;
}

// ---- active SH degree (include/gsplat.h gs_set_sh_degree; projection.hip proj_bwd_fused_kernel's BANDS forms) -----------------
int gs_set_sh_degree(gs_ctx* c, int degree)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (degree < 0 || degree > c->maxDegree)
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_sh_degree: degree is 0 .. the sh_degree the context was created with");
    c->modes.degree = degree;
    return GS_OK;
}

int gs_get_sh_degree(gs_ctx* c, int* degree)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!degree) return fail(c, GS_ERR_INVALID_ARG, "gs_get_sh_degree: null pointer");
    *degree = c->modes.degree;
    return GS_OK;
}

// ---- camera model (include/gsplat.h gs_set_camera_model; gs_math.h fisheye_map) ---------------------------------------------
int gs_set_camera_model(gs_ctx* c, int model)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (model != GS_CAMERA_PINHOLE && model != GS_CAMERA_FISHEYE)
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_camera_model: model is GS_CAMERA_PINHOLE or GS_CAMERA_FISHEYE");
    c->modes.fisheye = model == GS_CAMERA_FISHEYE;
    return GS_OK;
}

int gs_get_camera_model(gs_ctx* c, int* model)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!model) return fail(c, GS_ERR_INVALID_ARG, "gs_get_camera_model: null pointer");
    *model = c->modes.fisheye ? GS_CAMERA_FISHEYE : GS_CAMERA_PINHOLE;
    return GS_OK;
}

// ---- background colour (include/gsplat.h gs_set_background; gs_ctx.h GsBackground, background.hip) -------------------------
int gs_set_background(gs_ctx* c, const float* rgb)
{
    if (!c) return GS_ERR_INVALID_ARG;
    GsBackground bg;
    bg.mode = c->whiteBg ? GS_BG_WHITE : GS_BG_BLACK;
    if (rgb) {
        if (!isfinite(rgb[0]) || !isfinite(rgb[1]) || !isfinite(rgb[2]))
            return fail(c, GS_ERR_INVALID_ARG, "gs_set_background: the three values must be finite");
        bg.mode = GS_BG_COLOUR; bg.r = rgb[0]; bg.g = rgb[1]; bg.b = rgb[2];
    }
    c->modes.bg = bg;
    return GS_OK;
}

int gs_get_background(gs_ctx* c, float rgb[3])
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!rgb) return fail(c, GS_ERR_INVALID_ARG, "gs_get_background: null buffer");
    if (c->modes.bg.mode == GS_BG_COLOUR) { rgb[0] = c->modes.bg.r; rgb[1] = c->modes.bg.g; rgb[2] = c->modes.bg.b; }
    else rgb[0] = rgb[1] = rgb[2] = c->modes.bg.mode == GS_BG_WHITE ? 1.0f : 0.0f;
    return GS_OK;
}

int gs_composite_target(gs_ctx* c, long long n_pixels, const float* rgb, const float* alpha, const float* bg, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n_pixels < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_composite_target: negative n_pixels");
    if (!rgb || !alpha || !bg || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_composite_target: null pointer");
    return launch_composite_target(c, n_pixels, rgb, alpha, bg, out);
}

// ---- the 3-D smoothing filter (include/gsplat.h gs_set_filter3d; filter3d.hip, gs_math.h filter3d_activate) -----------------
int gs_set_filter3d_cameras(gs_ctx* c, int V, const gs_camera* cams)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (V < 0 || (V > 0 && !cams)) return fail(c, GS_ERR_INVALID_ARG, "gs_set_filter3d_cameras: V >= 0 and V cameras");
    if (V > 0) { if (const int rc = refuse_modes(c, "gs_set_filter3d_cameras", {GS_MODE_FISHEYE})) return rc; }
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    if (V == 0) {
        GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));      // (a width kernel may still be reading the table)
        ctx_free(c, c->f3dCams);
        c->f3dCamCount = c->f3dCamCap = 0;
        return GS_OK;
    }
    for (int v = 0; v < V; v++)
        if (!(cams[v].focal_x > 0.0f) || !(cams[v].fov_x > 0.0f) || !(cams[v].fov_y > 0.0f))
            return fail(c, GS_ERR_INVALID_ARG, "gs_set_filter3d_cameras: focal_x, fov_x and fov_y are > 0");
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (!c->f3dMax) { if (const int rc = ctx_alloc(c, &c->f3dMax, 1)) return rc; }
    if (V > c->f3dCamCap) {      // (the capacity counts cameras, the buffer rows of GS_F3D_CAM_FLOATS)
        c->f3dCamCount = 0;
        if (const int rc = ctx_grow(c, &c->f3dCams, &c->f3dCamCap, V, GS_F3D_CAM_FLOATS)) return rc;
    }
    std::vector<float> rows((size_t)V * GS_F3D_CAM_FLOATS, 0.0f);
    for (int v = 0; v < V; v++) {
        float* r = rows.data() + (size_t)v * GS_F3D_CAM_FLOATS;
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 4; k++) r[4 * a + k] = cams[v].view[4 * k + a];      // p_a = [x, 1] . view[:, a]
        r[12] = tanf(cams[v].fov_x * 0.5f) * 1.3f;      // (make_cam's limX / limY: the EWA clamp's constant)
        r[13] = tanf(cams[v].fov_y * 0.5f) * 1.3f;
        r[14] = cams[v].focal_x;
        // an off-centre principal point: |p.x / z + ox| <= limX is |(p.x + ox z) / z| <= limX, so the
        // offset goes into the row and the kernel is unchanged; a zero offset leaves the row's bits
        const float* P = cams[v].proj;
        if (P[8] != 0.0f && P[0] != 0.0f) {
            const float ox = P[8] / P[0];
            for (int k = 0; k < 4; k++) r[k] += ox * cams[v].view[4 * k + 2];
        }
        if (P[9] != 0.0f && P[5] != 0.0f) {
            const float oy = P[9] / P[5];
            for (int k = 0; k < 4; k++) r[4 + k] += oy * cams[v].view[4 * k + 2];
        }
    }
    GS_HIP_CHECK(c, hipMemcpy(c->f3dCams, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    c->f3dCamCount = V;
    return GS_OK;
}

int gs_compute_filter3d(gs_ctx* c, int N, const float* xyz, float* filter)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (c->f3dCamCount < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_compute_filter3d: no cameras (gs_set_filter3d_cameras)");
    if (N < 0 || (N > 0 && (!xyz || !filter))) return fail(c, GS_ERR_INVALID_ARG, "gs_compute_filter3d: N >= 0 and non-null buffers");
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    return launch_filter3d_width(c, N, xyz, filter);
}

int gs_set_filter3d(gs_ctx* c, const float* filter)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (filter && c->mcmcOn) return fail(c, GS_ERR_INVALID_ARG, "gs_set_filter3d: the MCMC strategy is set (the reference strategy only)");
    if (filter) { if (const int rc = refuse_modes(c, "gs_set_filter3d", {GS_MODE_SPARSE_ADAM})) return rc; }
    c->modes.filter3d = filter;
    return GS_OK;
}

int gs_filter3d_bake(gs_ctx* c, int N, const float* scales_raw, const float* opacity_raw, const float* filter,
                     float* out_scales_raw, float* out_opacity_raw)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!scales_raw || !opacity_raw || !filter || !out_scales_raw || !out_opacity_raw)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_filter3d_bake: N >= 0 and non-null buffers");
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    return launch_filter3d_bake(c, N, scales_raw, opacity_raw, filter, out_scales_raw, out_opacity_raw);
}

// ---- the MCMC strategy (include/gsplat.h gs_set_mcmc; mcmc.hip, projection.hip proj_bwd_fused_*mcmc_kernel) ----------------
static const char* mcmc_params_error(const gs_mcmc_params* p)
{
    if (!p) return "null gs_mcmc_params";
    auto fin = [](double v) { return v - v == 0.0; };
    if (!fin(p->noise_lr) || p->noise_lr < 0 || !fin(p->opacity_reg) || p->opacity_reg < 0 || !fin(p->scale_reg) || p->scale_reg < 0)
        return "noise_lr, opacity_reg and scale_reg are finite and >= 0";
    if (!(p->min_opacity > 0.0 && p->min_opacity < 1.0)) return "min_opacity is in (0, 1)";
    if (!(p->grow_rate >= 0.0 && p->grow_rate <= 1.0)) return "grow_rate is in [0, 1]";
    if (p->n_max < 1 || p->n_max > 51) return "n_max is in 1 .. 51";
    if (p->cap_max < 1 || p->cap_max > 0x7fffffffLL) return "cap_max is in 1 .. 2^31 - 1";
    if (p->iteration < 0) return "iteration >= 0";
    return nullptr;
}

int gs_set_mcmc(gs_ctx* c, const gs_mcmc_params* params)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!params) { c->mcmcOn = false; return GS_OK; }
    if (c->modes.filter3d) return fail(c, GS_ERR_INVALID_ARG, "gs_set_mcmc: a 3-D filter is set (gs_set_filter3d: the reference strategy only)");
    if (const int rc = refuse_modes(c, "gs_set_mcmc", {GS_MODE_SPARSE_ADAM})) return rc;
    if (const char* e = mcmc_params_error(params)) return fail(c, GS_ERR_INVALID_ARG, e);
    c->mcmc = *params;
    c->mcmcOn = true;
    return GS_OK;
}

int gs_mcmc_regularizer_grad(gs_ctx* c, int N, const float* scales, const float* opacity, float* grad_scales, float* grad_opacity,
                             const gs_mcmc_params* params)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const char* e = mcmc_params_error(params)) return fail(c, GS_ERR_INVALID_ARG, e);
    if (N < 0 || (N > 0 && (!scales || !opacity || !grad_scales || !grad_opacity)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_mcmc_regularizer_grad: bad arguments");
    return launch_mcmc_regularizer(c, N, scales, opacity, grad_scales, grad_opacity, *params);
}

int gs_mcmc_inject_noise(gs_ctx* c, int N, float* xyz, const float* scales, const float* rotation, const float* opacity,
                         float lr_xyz, const gs_mcmc_params* params)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const char* e = mcmc_params_error(params)) return fail(c, GS_ERR_INVALID_ARG, e);
    if (N < 0 || (N > 0 && (!xyz || !scales || !rotation || !opacity)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_mcmc_inject_noise: bad arguments");
    return launch_mcmc_noise(c, N, xyz, scales, rotation, opacity, lr_xyz, *params);
}

int gs_mcmc_random(gs_ctx* c, unsigned long long seed, int iteration, int stream, int n, uint32_t* words, float* normals,
                   double* uniforms)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n < 0 || iteration < 0 || stream < 0 || stream > 2) return fail(c, GS_ERR_INVALID_ARG, "gs_mcmc_random: bad arguments");
    return launch_mcmc_random(c, seed, iteration, stream, n, words, normals, uniforms);
}

static int mcmc_rows(gs_ctx* c, const char* who, int N, int K, float* xyz, float* fdc, float* frest, float* scales, float* rot,
                     float* opacity, const float* pBase, float* m, float* v, const gs_mcmc_params* params, McmcRows& rows)
{
    if (const char* e = mcmc_params_error(params)) return fail(c, GS_ERR_INVALID_ARG, e);
    if (N < 0 || K < 1 || K > 25) return fail(c, GS_ERR_INVALID_ARG, who);
    if (N > 0 && (!xyz || !fdc || (K > 1 && !frest) || !scales || !rot || !opacity || !pBase || !m || !v))
        return fail(c, GS_ERR_INVALID_ARG, who);
    float* t[6] = {xyz, fdc, K > 1 ? frest : fdc, scales, rot, opacity};
    for (int k = 0; k < 6; k++) {
        if (N > 0 && t[k] < pBase) return fail(c, GS_ERR_INVALID_ARG, who);
        rows.t[k] = t[k];
    }
    rows.pBase = pBase; rows.mBase = m; rows.vBase = v;
    return GS_OK;
}

int gs_mcmc_relocate(gs_ctx* c, int N, int K, float* xyz, float* features_dc, float* features_rest, float* scales, float* rotation,
                     float* opacity, const float* param_base, float* exp_avg, float* exp_avg_sq, const gs_mcmc_params* params,
                     long long stats[4])
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!stats) return fail(c, GS_ERR_INVALID_ARG, "gs_mcmc_relocate: null stats");
    McmcRows rows;
    const int rc = mcmc_rows(c, "gs_mcmc_relocate: bad arguments", N, K, xyz, features_dc, features_rest, scales, rotation,
                             opacity, param_base, exp_avg, exp_avg_sq, params, rows);
    if (rc) return rc;
    return mcmc_relocate(c, N, K, rows, *params, stats);
}

int gs_mcmc_grow(gs_ctx* c, int N, int capacity, int K, float* xyz, float* features_dc, float* features_rest, float* scales,
                 float* rotation, float* opacity, const float* param_base, float* exp_avg, float* exp_avg_sq,
                 const gs_mcmc_params* params, int* N_out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!N_out || capacity < N) return fail(c, GS_ERR_INVALID_ARG, "gs_mcmc_grow: bad arguments");
    McmcRows rows;
    const int rc = mcmc_rows(c, "gs_mcmc_grow: bad arguments", N, K, xyz, features_dc, features_rest, scales, rotation, opacity,
                             param_base, exp_avg, exp_avg_sq, params, rows);
    if (rc) return rc;
    return mcmc_grow(c, N, capacity, K, rows, *params, N_out);
}

int gs_set_pose_correction(gs_ctx* c, const float* delta, float* grad_delta)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!delta != !grad_delta) return fail(c, GS_ERR_INVALID_ARG, "gs_set_pose_correction: delta and grad_delta are both set or both NULL");
    if (delta && !c->poseCam) { const int arc = ctx_alloc(c, &c->poseCam, 1); if (arc) return arc; }
    c->modes.poseDelta = delta;
    c->modes.poseGrad = grad_delta;
    return GS_OK;
}

int gs_set_exposure(gs_ctx* c, const float* M, float* grad)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!M != !grad) return fail(c, GS_ERR_INVALID_ARG, "gs_set_exposure: M and grad are both set or both NULL");
    if (M && c->bgGrid) return fail(c, GS_ERR_INVALID_ARG, "gs_set_exposure: a bilateral grid is set (the two corrections are exclusive)");
    // (once per ctx, here: a step never allocates)
    if (M && !c->expoPartials) { const int arc = ctx_alloc(c, &c->expoPartials, (size_t)exposure_partials_doubles()); if (arc) return arc; }
    if (M) { const int arc = ensure_corrected_image(c); if (arc) return arc; }
    c->expoM = M;
    c->expoGrad = grad;
    return GS_OK;
}

int gs_apply_exposure(gs_ctx* c, long long n_pixels, const float* M, const float* in, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n_pixels < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_apply_exposure: negative n_pixels");
    if (n_pixels > 0 && (!M || !in || !out)) return fail(c, GS_ERR_INVALID_ARG, "gs_apply_exposure: null buffer");
    return launch_exposure_apply(c, n_pixels, M, in, out);
}

// ---- lens undistortion (include/gsplat.h gs_undistort; lens.hip) ----------------------------------------------------------------
int gs_undistort(gs_ctx* c, const gs_lens* lens, int src_w, int src_h, int dst_w, int dst_h, int channels, int mode,
                 const void* src, void* dst, unsigned char* valid)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!lens || !src || !dst) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: null pointer");
    if (mode < 0 || mode > 2) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: mode is 0 (colour), 1 (mask) or 2 (depth)");
    if (channels < 1 || channels > 4) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: channels in 1 .. 4");
    if (mode != 0 && channels != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: mask and depth images have one channel");
    if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: sizes are positive");
    if (dst_h > 4 * 65535) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: at most 262140 destination rows");
    const float focal[4] = {lens->fx, lens->fy, lens->dst_fx, lens->dst_fy};
    for (float f : focal)
        if (!(f > 0.0f) || !isfinite(f)) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: focal lengths are finite and > 0");
    const float rest[8] = {lens->cx, lens->cy, lens->k1, lens->k2, lens->p1, lens->p2, lens->dst_cx, lens->dst_cy};
    for (float f : rest)
        if (!isfinite(f)) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort: principal points and coefficients are finite");
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    return launch_undistort(c, *lens, src_w, src_h, dst_w, dst_h, channels, mode, src, dst, valid);
}

int gs_undistort_fisheye(gs_ctx* c, const gs_fisheye_lens* lens, int src_w, int src_h, int dst_w, int dst_h, int channels, int mode,
                         const void* src, void* dst, unsigned char* valid)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!lens || !src || !dst) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: null pointer");
    if (mode < 0 || mode > 2) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: mode is 0 (colour), 1 (mask) or 2 (depth)");
    if (channels < 1 || channels > 4) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: channels in 1 .. 4");
    if (mode != 0 && channels != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: mask and depth images have one channel");
    if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: sizes are positive");
    if (dst_h > 4 * 65535) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: at most 262140 destination rows");
    const float focal[4] = {lens->fx, lens->fy, lens->dst_fx, lens->dst_fy};
    for (float f : focal)
        if (!(f > 0.0f) || !isfinite(f)) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: focal lengths are finite and > 0");
    const float rest[8] = {lens->cx, lens->cy, lens->k1, lens->k2, lens->k3, lens->k4, lens->dst_cx, lens->dst_cy};
    for (float f : rest)
        if (!isfinite(f)) return fail(c, GS_ERR_INVALID_ARG, "gs_undistort_fisheye: principal points and coefficients are finite");
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    return launch_undistort_fisheye(c, *lens, src_w, src_h, dst_w, dst_h, channels, mode, src, dst, valid);
}

int gs_set_bilateral_grid(gs_ctx* c, const float* grid, float* grad, int grid_w, int grid_h, int grid_l, float tv_weight)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!grid != !grad) return fail(c, GS_ERR_INVALID_ARG, "gs_set_bilateral_grid: grid and grad are both set or both NULL");
    if (grid) {
        if (c->expoM) return fail(c, GS_ERR_INVALID_ARG, "gs_set_bilateral_grid: an exposure is set (the two corrections are exclusive)");
        if (!bilateral_shape_ok(grid_w, grid_h, grid_l))
            return fail(c, GS_ERR_INVALID_ARG, "gs_set_bilateral_grid: grid_w, grid_h in [2, 64] and grid_l in [2, 32]");
        if (!(tv_weight >= 0.0f) || !isfinite(tv_weight))
            return fail(c, GS_ERR_INVALID_ARG, "gs_set_bilateral_grid: tv_weight must be finite and >= 0");
        // (here and only here: a step never allocates; a trainer that sets the same shape every step allocates once)
        if (grid_w != c->bgChunksW || grid_h != c->bgChunksH) {
            c->bgChunks = bilateral_chunks(c->W, c->H, grid_w, grid_h);
            c->bgChunksW = grid_w;
            c->bgChunksH = grid_h;
        }
        const long long need = bilateral_partials_floats(grid_w, grid_h, grid_l, c->bgChunks);
        if (const int arc = ctx_grow(c, &c->bgPartials, &c->bgPartialsCap, need)) return arc;
        if (const int arc = ensure_corrected_image(c)) return arc;
    }
    c->bgGrid = grid;
    c->bgGrad = grad;
    c->bgW = grid_w;
    c->bgH = grid_h;
    c->bgL = grid_l;
    c->bgTv = tv_weight;
    return GS_OK;
}

int gs_apply_bilateral_grid(gs_ctx* c, int W, int H, const float* grid, int grid_w, int grid_h, int grid_l, const float* in,
                            float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (W < 0 || H < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_apply_bilateral_grid: negative image size");
    if (!bilateral_shape_ok(grid_w, grid_h, grid_l))
        return fail(c, GS_ERR_INVALID_ARG, "gs_apply_bilateral_grid: grid_w, grid_h in [2, 64] and grid_l in [2, 32]");
    if ((long long)W * H > 0 && (!grid || !in || !out)) return fail(c, GS_ERR_INVALID_ARG, "gs_apply_bilateral_grid: null buffer");
    return launch_bilateral_apply(c, W, H, grid, grid_w, grid_h, grid_l, in, out);
}

int gs_render_backward(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                       float* grad_xyz, float* grad_features_dc, float* grad_features_rest, float* grad_scales,
                       float* grad_rotation, float* grad_opacity)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_backward", cot_depth != nullptr); if (prc) return prc; }
    const int N = c->fwd.N, K = c->fwd.K;
    if (!cot_color) return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward: null cot_color");
    if (N > 0 && (!grad_xyz || !grad_features_dc || (K > 1 && !grad_features_rest) || !grad_scales || !grad_rotation ||
                  !grad_opacity))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward: null gradient buffer");
    if (const int rc = blend_backward_of_forward(c, cot_color, cot_depth, cot_alpha, c->absgrad, nullptr)) return rc;
    AbsgradScope noNorm(c);
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_projection_fused_backward(c, grad_xyz, grad_features_dc, grad_features_rest, grad_scales, grad_rotation, grad_opacity);
}

int gs_render_contrib(gs_ctx* c, float* max_w, float* sum_w)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_contrib", false); if (prc) return prc; }
    if (!max_w && !sum_w) return fail(c, GS_ERR_INVALID_ARG, "gs_render_contrib: null buffer (one of max_w, sum_w at least)");
    // reads the forward's records and lists, writes nothing of the context's: a backward may still follow
    return launch_blend_contrib(c, max_w, sum_w);
}

// reads the forward's records and lists, writes nothing of the context's: a backward and further feature calls may follow
int gs_render_features(gs_ctx* c, int C, const float* features, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_features", false); if (prc) return prc; }
    if (C < 1 || C > GS_MAX_FEATURE_CHANNELS) return fail(c, GS_ERR_INVALID_ARG, "gs_render_features: C must be in [1, GS_MAX_FEATURE_CHANNELS]");
    if (!features || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_render_features: null buffer");
    return launch_blend_features(c, C, features, out);
}

int gs_render_features_backward(gs_ctx* c, int C, const float* cot, float* grad_features)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_features_backward", false); if (prc) return prc; }
    if (C < 1 || C > GS_MAX_FEATURE_CHANNELS) return fail(c, GS_ERR_INVALID_ARG, "gs_render_features_backward: C must be in [1, GS_MAX_FEATURE_CHANNELS]");
    if (!cot || !grad_features) return fail(c, GS_ERR_INVALID_ARG, "gs_render_features_backward: null buffer");
    return launch_blend_features_backward(c, C, cot, grad_features);
}

// read the forward's records and lists, write nothing of the context's: a backward and further calls may follow
int gs_render_distortion(gs_ctx* c, const gs_distortion_params* params, float* out_distort, float* out_totals)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_distortion", false); if (prc) return prc; }
    if (const int rc = distortion_params_check(c, "gs_render_distortion", params)) return rc;
    if (!out_distort || !out_totals) return fail(c, GS_ERR_INVALID_ARG, "gs_render_distortion: null buffer");
    return launch_blend_distortion(c, *params, out_distort, out_totals);
}

int gs_render_distortion_backward(gs_ctx* c, const gs_distortion_params* params, const float* cot, const float* totals, float* rows16)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_distortion_backward", false); if (prc) return prc; }
    if (const int rc = distortion_params_check(c, "gs_render_distortion_backward", params)) return rc;
    if (!cot || !totals || (c->fwd.N > 0 && !rows16)) return fail(c, GS_ERR_INVALID_ARG, "gs_render_distortion_backward: null buffer");
    return launch_blend_distortion_backward(c, *params, cot, totals, rows16);
}

int gs_arm_distortion(gs_ctx* c, const gs_distortion_params* params, const float* cot, const float* totals)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!params && !cot && !totals) { c->distortion.armed = false; return GS_OK; }
    { const int prc = backward_preflight(c, "gs_arm_distortion", false); if (prc) return prc; }
    if (const int rc = distortion_params_check(c, "gs_arm_distortion", params)) return rc;
    if (!cot || !totals) return fail(c, GS_ERR_INVALID_ARG, "gs_arm_distortion: null buffer (all three NULL disarms)");
    c->distortion.armed = true;
    c->distortion.params = *params;
    c->distortion.cot = cot;
    c->distortion.totals = totals;
    return GS_OK;
}

int gs_contrib_actions(gs_ctx* c, int N, const float* score, float threshold, int* actions, int* output_counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || !(threshold == threshold) || (N > 0 && (!score || !actions || !output_counts)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_contrib_actions: bad arguments");
    return launch_contrib_actions(c, N, score, threshold, actions, output_counts);
}

int gs_render_backward_adam(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                            float* params_base, float* m_base, float* v_base, long long n_arena, const float lr[6],
                            float beta1, float beta2, float eps, float grad_scale)
{
    if (!c) return GS_ERR_INVALID_ARG;
    { const int prc = backward_preflight(c, "gs_render_backward_adam", cot_depth != nullptr); if (prc) return prc; }
    const int N = c->fwd.N, K = c->fwd.K;
    if (!cot_color || !lr || n_arena < 0 || (N > 0 && (!params_base || !m_base || !v_base)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward_adam: null buffer");
    if (const int rc = forward_in_arena(c, "gs_render_backward_adam", params_base, n_arena)) return rc;
    if (c->sparseAdam && (c->visN != N || c->fwd.modes.filter3d))
        return fail(c, GS_ERR_NO_FORWARD, "gs_render_backward_adam: sparse Adam is on, but the forward was not made under it "
                                          "(gs_set_sparse_adam comes before gs_render_forward)");
    if (const int rc = blend_backward_of_forward(c, cot_color, cot_depth, cot_alpha, c->absgrad, c->adamGate)) return rc;
    c->fwd.consumed = true;     // the parameters the forward saw are gone after this call
    AbsgradScope noNorm(c);
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_projection_fused_backward_adam(c, params_base, m_base, v_base, lr, beta1, beta2, eps, grad_scale);
}

int gs_render_backward_dp_begin(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                                float* color_cot)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int rc = refuse_modes(c, "gs_render_backward_dp_begin", {GS_MODE_POSE, GS_MODE_FILTER3D, GS_MODE_FISHEYE, GS_MODE_SPARSE_ADAM,
                                                                   GS_MODE_ABSGRAD, GS_MODE_ADC_STATS, GS_MODE_DISTORTION}))
        return rc;
    { const int prc = backward_preflight(c, "gs_render_backward_dp_begin", cot_depth != nullptr); if (prc) return prc; }
    const int N = c->fwd.N;
    if (!cot_color || (N > 0 && !color_cot)) return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward_dp_begin: null buffer");
    if (const int rc = blend_backward_of_forward(c, cot_color, cot_depth, cot_alpha)) return rc;
    c->fwd.blendBackwardDone = true;
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_color_cot(c, N, color_cot);
}

int gs_render_backward_dp_finish(gs_ctx* c, float* grad_xyz, float* grad_scales, float* grad_rotation, float* grad_opacity)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int rc = refuse_modes(c, "gs_render_backward_dp_finish", {GS_MODE_POSE, GS_MODE_FILTER3D, GS_MODE_FISHEYE, GS_MODE_SPARSE_ADAM})) return rc;
    if (!c->fwd.valid || !c->fwd.blendBackwardDone)
        return fail(c, GS_ERR_NO_FORWARD, "gs_render_backward_dp_finish: no gs_render_backward_dp_begin on this context");
    const int N = c->fwd.N, K = c->fwd.K;
    if (N > 0 && (!grad_xyz || !grad_scales || !grad_rotation || !grad_opacity))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward_dp_finish: null gradient buffer");
    c->fwd.blendBackwardDone = false;
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_projection_fused_backward(c, grad_xyz, nullptr, nullptr, grad_scales, grad_rotation, grad_opacity, true);
}

int gs_render_backward_dp_finish_geom(gs_ctx* c, float* grad_xyz, float* grad_scales, float* grad_rotation, float* grad_opacity,
                                      float* xyz_own)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int rc = refuse_modes(c, "gs_render_backward_dp_finish_geom", {GS_MODE_POSE, GS_MODE_FILTER3D, GS_MODE_FISHEYE, GS_MODE_SPARSE_ADAM})) return rc;
    if (!c->fwd.valid || !c->fwd.blendBackwardDone)
        return fail(c, GS_ERR_NO_FORWARD, "gs_render_backward_dp_finish_geom: no gs_render_backward_dp_begin on this context");
    const int N = c->fwd.N;
    if (N > 0 && (!grad_xyz || !grad_scales || !grad_rotation || !grad_opacity || !xyz_own))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward_dp_finish_geom: null buffer");
    c->fwd.blendBackwardDone = false;
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_projection_geom_backward(c, grad_xyz, grad_scales, grad_rotation, grad_opacity, xyz_own);
}

int gs_render_backward_dp_geom(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha, float* color_cot,
                               float* grad_xyz, float* grad_scales, float* grad_rotation, float* grad_opacity, float* xyz_own)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (const int rc = refuse_modes(c, "gs_render_backward_dp_geom", {GS_MODE_POSE, GS_MODE_FILTER3D, GS_MODE_FISHEYE, GS_MODE_SPARSE_ADAM,
                                                                  GS_MODE_ABSGRAD, GS_MODE_ADC_STATS, GS_MODE_DISTORTION}))
        return rc;
    { const int prc = backward_preflight(c, "gs_render_backward_dp_geom", cot_depth != nullptr); if (prc) return prc; }
    const int N = c->fwd.N;
    if (!cot_color || (N > 0 && (!color_cot || !grad_xyz || !grad_scales || !grad_rotation || !grad_opacity || !xyz_own)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_render_backward_dp_geom: null buffer");
    if (const int rc = blend_backward_of_forward(c, cot_color, cot_depth, cot_alpha)) return rc;
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_projection_geom_backward(c, grad_xyz, grad_scales, grad_rotation, grad_opacity, xyz_own, color_cot);
}

int gs_sh_grad_from_views_adam_dir(gs_ctx* c, int N, int K, int R, const float* xyz, const float* color_cot_all,
                                   const float* cam_centers, const float* const* own_xyz, float* features_dc, float* features_rest,
                                   float* params_base, float* m_base, float* v_base, long long n_arena, float lr_dc, float lr_rest,
                                   float beta1, float beta2, float eps, float grad_scale, float* xyz_add)
{
    if (!c) return GS_ERR_INVALID_ARG;
    const char* who = "gs_sh_grad_from_views_adam_dir";
    if (const int rc = refuse_modes(c, who, {GS_MODE_SPARSE_ADAM})) return rc;
    if (const int rc = sh_views_args(c, who, N, K, R, xyz, color_cot_all, cam_centers, features_dc, features_rest, n_arena < 0,
                                     !params_base || !m_base || !v_base || !xyz_add))
        return rc;
    if ((uintptr_t)xyz_add & 15) return fail(c, GS_ERR_INVALID_ARG, "gs_sh_grad_from_views_adam_dir: xyz_add must be 16-byte aligned");
    if (const int rc = sh_in_arena(c, who, N, K, features_dc, features_rest, params_base, n_arena)) return rc;
    if (const int rc = sh_rest_alignment(c, who, N, K, features_rest, params_base, m_base, v_base)) return rc;
    if (const int rc = sh_views_gate_layout(c, who, N, R)) return rc;
    GsStageTimer t(c, GS_STAGE_ADAM);
    return launch_sh_views_dir_adam(c, N, K, R, xyz, color_cot_all, cam_centers, own_xyz, features_dc, features_rest, params_base,
                                    m_base, v_base, lr_dc, lr_rest, beta1, beta2, eps, grad_scale, xyz_add);
}

int gs_render_backward_dp(gs_ctx* c, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                          float* grad_xyz, float* grad_scales, float* grad_rotation, float* grad_opacity, float* color_cot)
{
    const int rc = gs_render_backward_dp_begin(c, cot_color, cot_depth, cot_alpha, color_cot);
    if (rc) return rc;
    return gs_render_backward_dp_finish(c, grad_xyz, grad_scales, grad_rotation, grad_opacity);
}

int gs_sh_grad_from_views(gs_ctx* c, int N, int K, int R, const float* xyz, const float* color_cot_all,
                          const float* cam_centers, float* grad_features_dc, float* grad_features_rest)
{
    if (!c) return GS_ERR_INVALID_ARG;
    const char* who = "gs_sh_grad_from_views";
    if (const int rc = sh_views_args(c, who, N, K, R, xyz, color_cot_all, cam_centers, grad_features_dc, grad_features_rest, false,
                                     false))
        return rc;
    if (const int rc = sh_rest_alignment(c, who, N, K, grad_features_rest)) return rc;
    if (const int rc = sh_views_gate_layout(c, who, N, R)) return rc;
    GsStageTimer t(c, GS_STAGE_PROJ_BWD);
    return launch_sh_grad_from_views(c, N, K, R, xyz, color_cot_all, cam_centers, grad_features_dc, grad_features_rest);
}

int gs_sh_grad_from_views_adam(gs_ctx* c, int N, int K, int R, const float* xyz, const float* color_cot_all,
                               const float* cam_centers, float* features_dc, float* features_rest, float* params_base,
                               float* m_base, float* v_base, long long n_arena, float lr_dc, float lr_rest, float beta1,
                               float beta2, float eps, float grad_scale)
{
    if (!c) return GS_ERR_INVALID_ARG;
    const char* who = "gs_sh_grad_from_views_adam";
    if (const int rc = refuse_modes(c, who, {GS_MODE_SPARSE_ADAM})) return rc;
    if (const int rc = sh_views_args(c, who, N, K, R, xyz, color_cot_all, cam_centers, features_dc, features_rest, n_arena < 0,
                                     !params_base || !m_base || !v_base))
        return rc;
    if (const int rc = sh_in_arena(c, who, N, K, features_dc, features_rest, params_base, n_arena)) return rc;
    if (const int rc = sh_rest_alignment(c, who, N, K, features_rest, params_base, m_base, v_base)) return rc;
    if (const int rc = sh_views_gate_layout(c, who, N, R)) return rc;
    GsStageTimer t(c, GS_STAGE_ADAM);
    return launch_sh_grad_from_views_adam(c, N, K, R, xyz, color_cot_all, cam_centers, features_dc, features_rest,
                                          params_base, m_base, v_base, lr_dc, lr_rest, beta1, beta2, eps, grad_scale);
}

int gs_loss_forward_backward(gs_ctx* c, const float* render, const float* target, const float* render_depth,
                             const float* target_depth, const unsigned char* depth_mask, float lambda_dssim,
                             float lambda_depth, float* loss_out, float* cot_color, float* cot_depth)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!render || !target || !loss_out || !cot_color)
        return fail(c, GS_ERR_INVALID_ARG, "gs_loss_forward_backward: null buffer");
    if (lambda_depth != 0.0f && (!render_depth || !target_depth || !depth_mask || !cot_depth))
        return fail(c, GS_ERR_INVALID_ARG, "gs_loss_forward_backward: depth loss needs depth buffers");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    GsStageTimer t(c, GS_STAGE_LOSS);
    if (!c->bgGrid && !c->expoM)
        return launch_loss(c, render, target, render_depth, target_depth, depth_mask, lambda_dssim, lambda_depth, loss_out,
                           cot_color, cot_depth);
    // (a loss mask, gs_set_loss_mask, is launch_loss's business: the correction's backward below gets the weighted cotangent)
    // A per-view colour correction is bound -- a bilateral grid (the sliced transform) or an exposure (A r + b), never both:
    // the loss of the corrected image (the ctx's scratch image; the render itself is left alone), then the correction's
    // backward: cot_color <- dL/d render, grad <- dL/dG or dL/dM
    const bool grid = c->bgGrid != nullptr;
    const long long np = (long long)c->H * c->W;
    int rc = grid ? launch_bilateral_apply(c, c->W, c->H, c->bgGrid, c->bgW, c->bgH, c->bgL, render, c->correctedImage)
                  : launch_exposure_apply(c, np, c->expoM, render, c->correctedImage);
    if (rc) return rc;
    if ((rc = launch_loss(c, c->correctedImage, target, render_depth, target_depth, depth_mask, lambda_dssim, lambda_depth, loss_out,
                          cot_color, cot_depth)))
        return rc;
    return grid ? launch_bilateral_backward(c, c->W, c->H, c->bgGrid, c->bgW, c->bgH, c->bgL, c->bgChunks, c->bgTv, render,
                                            cot_color, c->bgPartials, c->bgGrad)
                : launch_exposure_backward(c, np, c->expoM, render, cot_color, c->expoPartials, c->expoGrad);
}

// ---- depth supervision (include/gsplat.h gs_depth_loss; depth_loss.hip) ---------------------------------------------------
int gs_depth_loss(gs_ctx* c, const gs_depth_loss_params* p, const float* render_depth, const float* render_alpha,
                  const float* target, const unsigned char* mask, float* loss, float* cot_depth, float* cot_alpha)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!p) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: null params");
    if (p->mode != GS_DEPTH_ACCUMULATED && p->mode != GS_DEPTH_EXPECTED && p->mode != GS_DEPTH_DISPARITY)
        return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: mode is GS_DEPTH_ACCUMULATED, GS_DEPTH_EXPECTED or GS_DEPTH_DISPARITY");
    if (!(p->alpha_min >= 0.0f) || !isfinite(p->alpha_min))
        return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: alpha_min is finite and >= 0");
    if (!isfinite(p->lambda) || !isfinite(p->scale) || !isfinite(p->offset))
        return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: lambda, scale and offset are finite");
    if (!render_depth || !target || !loss || !cot_depth) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: null buffer");
    if (p->mode != GS_DEPTH_ACCUMULATED && (!render_alpha || !cot_alpha))
        return fail(c, GS_ERR_INVALID_ARG, "gs_depth_loss: the expected and disparity modes need render_alpha and cot_alpha");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    if (!c->depthLossWs) {      // the first call: a step never allocates after it
        GS_HIP_CHECK(c, hipSetDevice(c->device));
        if (const int rc = ctx_alloc(c, &c->depthLossWs, (size_t)depth_loss_ws_doubles())) return rc;
    }
    GsStageTimer t(c, GS_STAGE_LOSS);
    return launch_depth_loss(c, p->mode, p->lambda, p->alpha_min, p->scale, p->offset, render_depth, render_alpha, target, mask,
                             loss, cot_depth, cot_alpha);
}

int gs_depth_normalize(gs_ctx* c, long long n_pixels, const float* depth, const float* alpha, float alpha_min, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n_pixels < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_normalize: negative n_pixels");
    if (!(alpha_min >= 0.0f) || !isfinite(alpha_min)) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_normalize: alpha_min is finite and >= 0");
    if (!depth || !alpha || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_normalize: null pointer");
    return launch_depth_normalize(c, n_pixels, depth, alpha, alpha_min, out);
}

// ---- normal regularisation (include/gsplat.h gs_normal_loss / gs_depth_normals; normal_loss.hip) ---------------------------
namespace {
bool nonneg_finite(float x) { return x >= 0.0f && isfinite(x); }

// what both entry points ask of the camera, the size and the two thresholds; NULL when all is well
const char* normal_geometry_error(const gs_normal_loss_params& p)
{
    if (!(p.fx > 0.0f) || !(p.fy > 0.0f) || !isfinite(p.fx) || !isfinite(p.fy)) return "fx and fy are positive and finite";
    if (!isfinite(p.cx) || !isfinite(p.cy)) return "cx and cy are finite";
    if (p.H <= 0 || p.W <= 0) return "H and W are positive";
    if (!nonneg_finite(p.alpha_min)) return "alpha_min is finite and >= 0";
    if (!nonneg_finite(p.max_jump)) return "max_jump is finite and >= 0";
    return nullptr;
}
}  // namespace

int gs_depth_normals(gs_ctx* c, const float* intrinsics, int H, int W, const float* depth, const float* alpha, float alpha_min,
                     float max_jump, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!intrinsics || !depth || !alpha || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_depth_normals: null pointer");
    gs_normal_loss_params p = {};
    p.fx = intrinsics[0]; p.fy = intrinsics[1]; p.cx = intrinsics[2]; p.cy = intrinsics[3];
    p.H = H; p.W = W; p.alpha_min = alpha_min; p.max_jump = max_jump;
    if (const char* why = normal_geometry_error(p)) return fail(c, GS_ERR_INVALID_ARG, std::string("gs_depth_normals: ") + why);
    return launch_depth_normals(c, p, depth, alpha, out);
}

int gs_normal_loss(gs_ctx* c, const gs_normal_loss_params* p, const float* render_depth, const float* render_alpha,
                   const float* target_normals, const unsigned char* mask, const float* edge_image, float* loss, float* normal_out,
                   float* cot_depth, float* cot_alpha)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!p) return fail(c, GS_ERR_INVALID_ARG, "gs_normal_loss: null params");
    if (const char* why = normal_geometry_error(*p)) return fail(c, GS_ERR_INVALID_ARG, std::string("gs_normal_loss: ") + why);
    if (!nonneg_finite(p->lambda_l1) || !nonneg_finite(p->lambda_cos) || !nonneg_finite(p->lambda_smooth))
        return fail(c, GS_ERR_INVALID_ARG, "gs_normal_loss: lambda_l1, lambda_cos and lambda_smooth are finite and >= 0");
    if (!nonneg_finite(p->edge_gamma)) return fail(c, GS_ERR_INVALID_ARG, "gs_normal_loss: edge_gamma is finite and >= 0");
    if (p->accumulate != 0 && p->accumulate != 1) return fail(c, GS_ERR_INVALID_ARG, "gs_normal_loss: accumulate is 0 or 1");
    if (!render_depth || !render_alpha || !loss || !normal_out || !cot_depth || !cot_alpha)
        return fail(c, GS_ERR_INVALID_ARG, "gs_normal_loss: null buffer");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    const long long want = normal_loss_ws_floats((long long)p->H * p->W);
    if (want > c->normalWsFloats || !c->normalPartials) {      // the first call, or a larger image: a step never allocates after it
        GS_HIP_CHECK(c, hipSetDevice(c->device));
        if (const int rc = ctx_grow(c, &c->normalWs, &c->normalWsFloats, want)) return rc;
        if (!c->normalPartials)
            if (const int rc = ctx_alloc(c, &c->normalPartials, (size_t)normal_loss_ws_doubles())) return rc;
    }
    GsStageTimer t(c, GS_STAGE_LOSS);
    return launch_normal_loss(c, *p, render_depth, render_alpha, target_normals, mask, edge_image, loss, normal_out, cot_depth,
                              cot_alpha, c->normalWs, c->normalPartials);
}

// ---- held-out evaluation (include/gsplat.h gs_image_metrics / gs_colour_moments; metrics.hip) ------------------------------
namespace {
// the partials of both entry points: allocated at the first call, regrown only when a larger image needs more
int ensure_metrics_ws(gs_ctx* c, int H, int W)
{
    const long long want = metrics_ws_doubles(H, W);
    if (want <= c->metricsWsDoubles) return GS_OK;
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    return ctx_grow(c, &c->metricsWs, &c->metricsWsDoubles, want);
}
}  // namespace

int gs_image_metrics(gs_ctx* c, int H, int W, const float* render, const float* target, const unsigned char* mask, double* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (H < 0 || W < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_image_metrics: negative H or W");
    if (!render || !target || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_image_metrics: null render, target or out");
    if (H > 0 && W > 0)
        if (const int rc = ensure_metrics_ws(c, H, W)) return rc;
    return launch_image_metrics(c, H, W, render, target, mask, out);
}

int gs_colour_moments(gs_ctx* c, long long n_pixels, const float* render, const float* target, const unsigned char* mask,
                      double* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n_pixels < 0) return fail(c, GS_ERR_INVALID_ARG, "gs_colour_moments: negative n_pixels");
    if (!render || !target || !out) return fail(c, GS_ERR_INVALID_ARG, "gs_colour_moments: null render, target or out");
    if (n_pixels > 0)
        if (const int rc = ensure_metrics_ws(c, 1, 1)) return rc;      // (its 512 x 22 partials are the workspace's least size)
    return launch_colour_moments(c, n_pixels, render, target, mask, out);
}

int gs_loss_target_cache_floats(gs_ctx* c, long long* n)
{
    if (!c || !n) return GS_ERR_INVALID_ARG;
    *n = 2LL * 3LL * c->H * c->W;
    return GS_OK;
}

int gs_set_loss_target_cache(gs_ctx* c, float* cache, int filled)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->lossTargetCache = cache;
    c->lossTargetCacheFilled = cache != nullptr && filled != 0;
    return GS_OK;
}

int gs_set_loss_mask(gs_ctx* c, const unsigned char* mask)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->lossMask = mask;      // read by launch_loss (ssim.hip) only
    return GS_OK;
}

int gs_set_block_work_buffer(gs_ctx* c, uint32_t* buf)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->blockWork = buf ? buf : c->blockWorkOwn;
    c->workHint = buf;
    c->cutStore = nullptr;
    return GS_OK;
}

int gs_view_hint_words(gs_ctx* c, int* n)
{
    if (!c || !n) return GS_ERR_INVALID_ARG;
    *n = c->numPixBlocks + c->T;
    return GS_OK;
}

int gs_set_view_hints(gs_ctx* c, uint32_t* buf, int words)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (buf && words < c->numPixBlocks + c->T) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_set_view_hints: buffer too small (gs_view_hint_words)");
    c->blockWork = buf ? buf : c->blockWorkOwn;
    c->workHint = buf;
    // cuts are per tile and renewed per 16x16 block: kept only where the two coincide
    c->cutStore = (buf && c->fast16 && c->tileW == 16 && c->tileH == 16) ? buf + c->numPixBlocks : nullptr;
    return GS_OK;
}

int gs_clear_depth_cuts(gs_ctx* c, uint32_t* buf, int words)
{
    if (!c || !buf) return GS_ERR_INVALID_ARG;
    if (words < c->numPixBlocks + c->T) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_clear_depth_cuts: buffer too small (gs_view_hint_words)");
    GS_HIP_CHECK(c, hipMemsetAsync(buf + c->numPixBlocks, 0, sizeof(uint32_t) * (size_t)c->T, c->stream));
    return GS_OK;
}

int gs_set_depth_cuts(gs_ctx* c, int enable)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->allowCuts = enable != 0;
    return GS_OK;
}

int gs_forward_missed(gs_ctx* c, int* missed)
{
    if (!c || !missed) return GS_ERR_INVALID_ARG;
    *missed = 0;
    if (!c->fwd.valid) return fail(c, GS_ERR_NO_FORWARD, "gs_forward_missed: no gs_render_forward on this context");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    if (!c->fwd.cutsActive) return GS_OK;
    const int rc = settle_cut_forward(c);
    if (rc) return rc;
    *missed = c->fwd.missed ? 1 : 0;
    return deferred_overflow(c);      // the wait was behind the forward: its overflow word, if any, has landed
}

int gs_cut_stats(gs_ctx* c, uint32_t out[2])
{
    if (!c || !out) return GS_ERR_INVALID_ARG;
    out[0] = out[1] = 0;
    if (!c->fwd.valid || !c->fwd.cutsActive) return GS_OK;
    if (!c->fwd.missChecked) return fail(c, GS_ERR_INVALID_ARG, "gs_cut_stats: ask gs_forward_missed first");
    out[0] = c->missHost[1]; out[1] = c->missHost[2];
    return GS_OK;
}

int gs_ctx_set_tuning(gs_ctx* c, int knob, long long value)
{
    if (!c) return GS_ERR_INVALID_ARG;
    switch (knob) {
    case GS_TUNE_FWD_WAVES_PER_SIMD:
        if (value < 1 || value > 16) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: forward waves per SIMD must be 1..16");
        c->fwdWavesPerSimd = (int)value; return GS_OK;
    case GS_TUNE_BWD_WAVES_PER_CU:
        if (value < 1 || value > 64) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: backward waves per CU must be 1..64");
        c->bwdWavesPerCu = (int)value; return GS_OK;
    case GS_TUNE_FWD_QUADRANTS:
        c->fwdQuadrants = value != 0; return GS_OK;
    case GS_TUNE_FWD_QUEUES:
        if (value < 1 || value > (long long)GS_QUEUES || (value & (value - 1))) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: forward queues must be 1, 2, 4 or 8");
        c->fwdQueues = (int)value; return GS_OK;
    case GS_TUNE_FWD_FOUR_WAVES:
        c->fwdWide = value < 0 ? -1 : (value != 0); return GS_OK;
    case GS_TUNE_OP_FWD_PPL:
    case GS_TUNE_OP_BWD_PPL:
        if (value != 1 && value != 2 && value != 4) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: pixels per lane must be 1, 2 or 4");
        (knob == GS_TUNE_OP_FWD_PPL ? c->opFwdPpl : c->opBwdPpl) = (int)value; return GS_OK;
    case GS_TUNE_WIDE_TILE_SORT:
        c->wideTileSort = value != 0; return GS_OK;
    case GS_TUNE_DEPTH_GRADIENT:
        c->depthGradient = value != 0; return GS_OK;
    case GS_TUNE_HOST_OVERFLOW_ERRORS:
        c->hostOverflowErrors = value != 0; return GS_OK;
    case GS_TUNE_SPLITTER_DEPTH_SORT:
        c->splitterSort = value > 0; c->haveSplitters = false; return GS_OK;      // (2, once a second form, is 1)
    case GS_TUNE_COLOUR_RIDERS:
        c->colourRiders = (int)value; return GS_OK;
    case GS_TUNE_FWD_FOLD_TEST_SCALE:
        if (value < 1 || value > 1000) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: fold test scale is in permille, 1..1000");
        c->fwdFoldScale = (float)value / 1000.0f; return GS_OK;
    case GS_TUNE_POISON_CHECKPOINTS:
        c->poisonCheckpoints = value != 0; return GS_OK;
    case GS_TUNE_RENDER_ONLY:
        c->renderOnly = value != 0; return GS_OK;
    case GS_TUNE_FWD_SLOW_SLOT:
        if (value < 1 || value > 16) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: the first slow wave slot must be 1..16 (16 = none)");
        c->fwdSlowSlot = (int)value; return GS_OK;
    case GS_TUNE_FWD_PAIR:
        if (value < -1 || value > 16) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: forward pair workgroups per CU must be -1 (by list depth), 0..16");
        c->fwdPair = (int)value; return GS_OK;
    case GS_TUNE_TRIM_RECTS:
        if (value < 0 || value > 2) return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: trim rects is 0 (the reference's squares), 1 (cut by the ellipse's box) or 2 (and into four row groups)");
        c->trimRects = value != 0; c->rowGroups = value == 2; return GS_OK;
    case GS_TUNE_SH_BAND_SKIP:
        c->shBandSkip = value != 0; return GS_OK;
    case GS_TUNE_FWD_TRACE_BUFFER:
        c->fwdTrace = reinterpret_cast<unsigned long long*>((uintptr_t)value); return GS_OK;
    default:
        return fail(c, GS_ERR_INVALID_ARG, "gs_ctx_set_tuning: unknown knob");
    }
}

int gs_copy_overflow_flag(gs_ctx* c, uint32_t* out)
{
    if (!c || !out) return GS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(copy_word_kernel, dim3(1), dim3(1), 0, c->stream, c->counters + GS_CNT_OVERFLOW, out);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int gs_set_update_gate(gs_ctx* c, const uint32_t* gate)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->adamGate = gate ? gate : c->counters + GS_CNT_OVERFLOW;
    return GS_OK;
}

int gs_set_overflow_rider(gs_ctx* c, float* dst)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->overflowRider = dst;
    return GS_OK;
}

int gs_set_gathered_gate(gs_ctx* c, long long block_floats, int count, uint32_t* reduced_out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (block_floats < 0 || (block_floats > 0 && (count < 1 || count > 16)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_set_gathered_gate: bad block size / count (1..16 blocks)");
    c->ccBlockFloats = block_floats;
    c->ccBlockCount = block_floats > 0 ? count : 0;
    c->gatheredGateOut = block_floats > 0 ? reduced_out : nullptr;
    return GS_OK;
}

int gs_set_gate_seen(gs_ctx* c, uint32_t* seen)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->gateSeen = seen;
    return GS_OK;
}

int gs_set_grad_norm_accum(gs_ctx* c, float* accum)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->gradNormAccum = accum;
    return GS_OK;
}

int gs_block_count(gs_ctx* c, int* n)
{
    if (!c || !n) return GS_ERR_INVALID_ARG;
    *n = c->numPixBlocks;
    return GS_OK;
}

int gs_copy_block_work(gs_ctx* c, uint32_t* out)
{
    if (!c || !out) return GS_ERR_INVALID_ARG;
    if (!c->fwd.valid) return fail(c, GS_ERR_NO_FORWARD, "gs_copy_block_work: no gs_render_forward on this context");
    if (!c->fast16) return fail(c, GS_ERR_INVALID_ARG, "gs_copy_block_work: only for tile sizes served by the fused kernels");
    GS_HIP_CHECK(c, hipMemcpyAsync(out, c->fwd.blockWork, sizeof(uint32_t) * (size_t)c->numPixBlocks, hipMemcpyDeviceToDevice,
                                   c->stream));
    return GS_OK;
}

int gs_copy_last_contrib(gs_ctx* c, uint32_t* out)
{
    if (!c || !out) return GS_ERR_INVALID_ARG;
    if (!c->fwd.valid) return fail(c, GS_ERR_NO_FORWARD, "gs_copy_last_contrib: no gs_render_forward on this context");
    GS_HIP_CHECK(c, hipMemcpyAsync(out, c->lastContrib, sizeof(uint32_t) * (size_t)c->W * c->H, hipMemcpyDeviceToDevice,
                                   c->stream));
    return GS_OK;
}

int gs_adam_step(gs_ctx* c, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                 const long long* seg_end, const float* seg_lr, float beta1, float beta2, float eps, float grad_scale)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n < 0 || nseg < 1 || nseg > 8 || !seg_end || !seg_lr) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step: bad segments");
    if (n > 0 && (!params || !grads || !m || !v)) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step: null buffer");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v) & 15)
        return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step: arenas must be 16-byte aligned");
    long long prev = 0;
    for (int i = 0; i < nseg; i++) {
        if (seg_end[i] < prev || seg_end[i] > n) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step: segments not ascending");
        prev = seg_end[i];
    }
    if (prev != n) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_adam_step: segments do not cover the arena");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    return launch_adam(c, n, params, grads, m, v, nseg, seg_end, seg_lr, beta1, beta2, eps, grad_scale);
}

int gs_adam_step_visible(gs_ctx* c, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                         const long long* seg_end, const float* seg_lr, const int* seg_row_floats, float beta1, float beta2,
                         float eps, float grad_scale, int N, const unsigned char* visible)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (n < 0 || nseg < 1 || nseg > 8 || !seg_end || !seg_lr || !seg_row_floats || N < 0)
        return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_visible: bad segments");
    if (n > 0 && (!params || !grads || !m || !v)) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_visible: null buffer");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v) & 15)
        return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_visible: arenas must be 16-byte aligned");
    long long prev = 0;
    for (int i = 0; i < nseg; i++) {
        if (seg_end[i] < prev || seg_end[i] > n) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_visible: segments not ascending");
        if (seg_row_floats[i] < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_visible: seg_row_floats are >= 1");
        prev = seg_end[i];
    }
    if (prev != n) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_adam_step_visible: segments do not cover the arena");
    if (!visible) {
        if (c->visN < 0)
            return fail(c, GS_ERR_NO_FORWARD, "gs_adam_step_visible: visible is NULL and the last gs_render_forward was not made with "
                                              "sparse Adam on (gs_set_sparse_adam)");
        if (N != c->visN) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_adam_step_visible: N differs from the forward's N");
        visible = c->visMask;
    }
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    if (N == 0) return GS_OK;      // (no row below N: nothing moves)
    return launch_adam_visible(c, n, params, grads, m, v, nseg, seg_end, seg_lr, seg_row_floats, beta1, beta2, eps, grad_scale, N,
                               visible);
}

int gs_adam_step_add(gs_ctx* c, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                     const long long* seg_end, const float* seg_lr, float beta1, float beta2, float eps, float grad_scale,
                     const float* add, long long add_n)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (add_n < 0 || add_n > n || (add_n > 0 && !add) || ((uintptr_t)add & 15))
        return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_add: add must be 16-byte aligned and cover at most the arena");
    if (n < 0 || nseg < 1 || nseg > 8 || !seg_end || !seg_lr) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_add: bad segments");
    if (n > 0 && (!params || !grads || !m || !v)) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_add: null buffer");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v) & 15)
        return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_add: arenas must be 16-byte aligned");
    long long prev = 0;
    for (int i = 0; i < nseg; i++) {
        if (seg_end[i] < prev || seg_end[i] > n) return fail(c, GS_ERR_INVALID_ARG, "gs_adam_step_add: segments not ascending");
        prev = seg_end[i];
    }
    if (prev != n) return fail(c, GS_ERR_SIZE_MISMATCH, "gs_adam_step_add: segments do not cover the arena");
    { const int orc = deferred_overflow(c); if (orc) return orc; }
    return launch_adam(c, n, params, grads, m, v, nseg, seg_end, seg_lr, beta1, beta2, eps, grad_scale, add_n > 0 ? add : nullptr, add_n);
}

int gs_accum_grad_norm(gs_ctx* c, int N, const float* xyz_grad, const float* accum_in, float* accum_out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!xyz_grad || !accum_out))) return fail(c, GS_ERR_INVALID_ARG, "gs_accum_grad_norm: bad arguments");
    return launch_accum_grad_norm(c, N, xyz_grad, accum_in, accum_out);
}

int gs_classify_gaussians(gs_ctx* c, int N, const float* grad_accum, float denom, const float* scales,
                          int scale_stride, const float* opacity, float grad_threshold, float max_scale_thresh,
                          float min_opacity_thresh, int allow_densify, int* actions, int* output_counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || scale_stride < 3) return fail(c, GS_ERR_INVALID_ARG, "gs_classify_gaussians: bad N / scale_stride");
    if (N > 0 && (!grad_accum || !scales || !opacity || !actions || !output_counts))
        return fail(c, GS_ERR_INVALID_ARG, "gs_classify_gaussians: null buffer");
    return launch_classify(c, N, grad_accum, denom, scales, scale_stride, opacity, grad_threshold, max_scale_thresh,
                           min_opacity_thresh, allow_densify, actions, output_counts);
}

int gs_densify_offsets(gs_ctx* c, int N, const int* actions, const int* output_counts, int* offsets, long long stats[5])
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || !stats || (N > 0 && (!actions || !output_counts || !offsets)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_densify_offsets: bad arguments");
    return launch_densify_offsets(c, N, actions, output_counts, offsets, stats);
}

int gs_build_densify_output_map(gs_ctx* c, int N, const int* actions, const int* offsets, int total,
                                int* gather_indices, int* noise_mode)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || total < 0 || (N > 0 && (!actions || !offsets)) || (total > 0 && (!gather_indices || !noise_mode)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_build_densify_output_map: bad arguments");
    return launch_build_densify_map(c, N, actions, offsets, total, gather_indices, noise_mode);
}

int gs_densify_gather(gs_ctx* c, int total, int K, const float* xyz, const float* features_dc,
                      const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                      const int* gather_indices, const int* noise_mode, const float* base_noise, float* out_xyz,
                      float* out_features_dc, float* out_features_rest, float* out_scales, float* out_rotation,
                      float* out_opacity)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (total < 0 || K < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather: bad total / K");
    if (total > 0 && (!xyz || !features_dc || !scales || !rotation || !opacity || !gather_indices || !noise_mode ||
                      !out_xyz || !out_features_dc || !out_scales || !out_rotation || !out_opacity ||
                      (K > 1 && (!features_rest || !out_features_rest))))
        return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather: null buffer");
    return launch_densify_gather(c, total, K, xyz, features_dc, features_rest, scales, rotation, opacity,
                                 gather_indices, noise_mode, base_noise, out_xyz, out_features_dc, out_features_rest,
                                 out_scales, out_rotation, out_opacity);
}

int gs_densify_plan(gs_ctx* c, int N, const int* actions, const int* output_counts, int* offsets)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || (N > 0 && (!actions || !output_counts || !offsets)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_densify_plan: bad arguments");
    return launch_densify_plan(c, N, actions, output_counts, offsets);
}

int gs_densify_plan_read(gs_ctx* c, int wait, long long plan[8], int* ready)
{
    if (!c || !plan || !ready) return GS_ERR_INVALID_ARG;
    return densify_plan_read(c, wait, plan, ready);
}

int gs_build_densify_output_map_planned(gs_ctx* c, int N, const int* actions, const int* offsets, int capacity,
                                        int* gather_indices, int* noise_mode)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->densifyPlanned) return fail(c, GS_ERR_NO_FORWARD, "gs_build_densify_output_map_planned: no gs_densify_plan on this context");
    if (N < 0 || capacity < 0 || (N > 0 && (!actions || !offsets)) || (capacity > 0 && (!gather_indices || !noise_mode)))
        return fail(c, GS_ERR_INVALID_ARG, "gs_build_densify_output_map_planned: bad arguments");
    return launch_build_densify_map_planned(c, N, actions, offsets, capacity, gather_indices, noise_mode);
}

int gs_densify_gather_planned(gs_ctx* c, int capacity, int K, const float* xyz, const float* features_dc,
                              const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                              const int* gather_indices, const int* noise_mode, unsigned long long noise_seed, float* out_xyz,
                              float* out_features_dc, float* out_features_rest, float* out_scales, float* out_rotation,
                              float* out_opacity)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->densifyPlanned) return fail(c, GS_ERR_NO_FORWARD, "gs_densify_gather_planned: no gs_densify_plan on this context");
    if (capacity < 0 || K < 1) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned: bad capacity / K");
    if (capacity > 0 && (!xyz || !features_dc || !scales || !rotation || !opacity || !gather_indices || !noise_mode ||
                         !out_xyz || !out_features_dc || !out_scales || !out_rotation || !out_opacity ||
                         (K > 1 && (!features_rest || !out_features_rest))))
        return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned: null buffer");
    return launch_densify_gather_planned(c, capacity, K, xyz, features_dc, features_rest, scales, rotation, opacity,
                                         gather_indices, noise_mode, noise_seed, out_xyz, out_features_dc, out_features_rest,
                                         out_scales, out_rotation, out_opacity);
}

int gs_densify_gather_planned_packed(gs_ctx* c, int capacity, int K, const float* xyz, const float* features_dc,
                                     const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                                     const int* gather_indices, const int* noise_mode, unsigned long long noise_seed,
                                     float* out_base, const int arena_order[6])
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->densifyPlanned) return fail(c, GS_ERR_NO_FORWARD, "gs_densify_gather_planned_packed: no gs_densify_plan on this context");
    if (capacity < 0 || K < 1 || !arena_order) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned_packed: bad capacity / K / order");
    int seen = 0;
    for (int i = 0; i < 6; i++) if (arena_order[i] >= 0 && arena_order[i] < 6) seen |= 1 << arena_order[i];
    if (seen != 63) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned_packed: arena_order must be a permutation of 0..5");
    if (capacity > 0 && (!xyz || !features_dc || (K > 1 && !features_rest) || !scales || !rotation || !opacity || !gather_indices ||
                         !noise_mode || !out_base))
        return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned_packed: null buffer");
    if ((uintptr_t)out_base & 15) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_gather_planned_packed: out_base must be 16-byte aligned");
    return launch_densify_gather_planned_packed(c, capacity, K, xyz, features_dc, features_rest, scales, rotation, opacity,
                                                gather_indices, noise_mode, noise_seed, out_base, arena_order);
}

int gs_densify_noise(gs_ctx* c, unsigned long long seed, int rows, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (rows < 0 || (rows > 0 && !out)) return fail(c, GS_ERR_INVALID_ARG, "gs_densify_noise: bad arguments");
    return launch_densify_noise(c, seed, rows, out);
}

static bool ply_args_ok(int N, int K, const void* a, const void* b, const void* r, const void* o, const void* s,
                        const void* q)
{
    if (N < 0 || K < 1) return false;
    if (N == 0) return true;
    return a && b && o && s && q && (K == 1 || r);
}

int gs_ply_write(gs_ctx* c, const char* path, int N, int K, const float* xyz, const float* features_dc,
                 const float* features_rest, const float* opacity, const float* scales, const float* rotation)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!path || !ply_args_ok(N, K, xyz, features_dc, features_rest, opacity, scales, rotation))
        return fail(c, GS_ERR_INVALID_ARG, "gs_ply_write: bad arguments");
    return ply_write_file(c, path, N, K, xyz, features_dc, features_rest, opacity, scales, rotation);
}

int gs_ply_probe(gs_ctx* c, const char* path, long long* N, int* M, int* D)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!path || !N || !M || !D) return fail(c, GS_ERR_INVALID_ARG, "gs_ply_probe: bad arguments");
    return ply_probe_file(c, path, N, M, D);
}

int gs_ply_load(gs_ctx* c, const char* path, int N, int K, float* xyz, float* features_dc, float* features_rest,
                float* opacity, float* scales, float* rotation)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!path || !ply_args_ok(N, K, xyz, features_dc, features_rest, opacity, scales, rotation))
        return fail(c, GS_ERR_INVALID_ARG, "gs_ply_load: bad arguments");
    return ply_load_file(c, path, N, K, xyz, features_dc, features_rest, opacity, scales, rotation);
}

int gs_ply_pack_rows(gs_ctx* c, int N, int K, const float* xyz, const float* features_dc,
                     const float* features_rest, const float* opacity, const float* scales, const float* rotation,
                     float* rows)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!ply_args_ok(N, K, xyz, features_dc, features_rest, opacity, scales, rotation) || (N > 0 && !rows))
        return fail(c, GS_ERR_INVALID_ARG, "gs_ply_pack_rows: bad arguments");
    return launch_ply_pack(c, N, K, xyz, features_dc, features_rest, opacity, scales, rotation, rows);
}

int gs_dist_topk(gs_ctx* c, int N, int k, int q_begin, int q_count, const float* xyz, float* out)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (N < 0 || k < 1 || k > 8 || q_begin < 0 || q_count < 0 || (long long)q_begin + q_count > N)
        return fail(c, GS_ERR_INVALID_ARG, "gs_dist_topk: bad N / k / query range");
    if (q_count > 0 && (!xyz || !out)) return fail(c, GS_ERR_INVALID_ARG, "gs_dist_topk: null buffer");
    return launch_dist_topk(c, N, k, q_begin, q_count, xyz, out);
}

int gs_profile_enable(gs_ctx* c, unsigned stage_mask)
{
    if (!c) return GS_ERR_INVALID_ARG;
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->profMask = stage_mask;
    if (stage_mask) c->profUsed = 0;
    return GS_OK;
}

int gs_profile_read(gs_ctx* c, float ms[GS_STAGE_COUNT], int calls[GS_STAGE_COUNT])
{
    if (!c || !ms || !calls) return GS_ERR_INVALID_ARG;
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < GS_STAGE_COUNT; i++) { ms[i] = 0.0f; calls[i] = 0; }
    for (size_t i = 0; i < c->profUsed; i++) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, c->profPool[i].a, c->profPool[i].b) == hipSuccess) {
            ms[c->profPool[i].stage] += t;
            if (!c->profPool[i].extra) calls[c->profPool[i].stage] += 1;
        }
    }
    return GS_OK;
}

int gs_last_stats(gs_ctx* c, uint32_t stats[8])
{
    if (!c || !stats) return GS_ERR_INVALID_ARG;
    int rc;
    if (c->binValid && (rc = launch_tile_counts(c))) return rc;
    if ((rc = read_counters(c))) return rc;
    stats[0] = c->countersHost[GS_CNT_NVIS];
    // pairs binned; under depth cuts that is fewer than the pairs required without them (GS_CNT_MREQ, the capacity check)
    stats[1] = c->countersHost[GS_CNT_OVERFLOW] ? c->countersHost[GS_CNT_MREQ] : c->countersHost[GS_CNT_M];
    stats[2] = c->countersHost[GS_CNT_B];
    stats[3] = c->countersHost[GS_CNT_CONTRIB_LO];
    stats[4] = c->countersHost[GS_CNT_CONTRIB_HI];
    stats[5] = c->countersHost[GS_CNT_OVERFLOW];
    stats[6] = (uint32_t)c->capN;
    stats[7] = (uint32_t)(c->capM > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : c->capM);
    return GS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
