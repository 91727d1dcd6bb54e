// blend.hip -- front-to-back alpha blend of the sorted per-tile splat lists, forward and backward.
//
// Replaces gaussian_tile_global_forward / gaussian_tile_global_backward
// (slang/gaussian_tile_global_kernels.slang:437-614, 648-881).  The reference runs the forward with
// one thread per pixel, every pixel re-reading its tile's whole list from device memory; here a
// workgroup owns one 16x16 pixel block, the block's waves stage the sorted list through LDS in
// coalesced index bursts + 48-B record gathers, every lane blends PPL pixels out of registers, and a
// block leaves as soon as all its pixels have saturated (T < 1e-4).
//   PPL = 4 : one wavefront per tile (64 lanes x 4 px)        -- least LDS traffic, longest critical path
//   PPL = 2 : two wavefronts per tile
//   PPL = 1 : four wavefronts per tile
// Backward walks the list in reverse, rebuilds T by division exactly as the reference's
// undoTileGlobalPixelState does, sums each splat's 11 gradients over the lane's pixels in registers, then
// the ten distinct ones over the wave with the transposed reduction of gs_wavesum.h (one total per lane
// quad), over the block's waves through LDS, and adds them per (tile, splat) into a 64-B-aligned
// accumulator row with native f32 atomics.
// VALU/transcendental-bound (about 24 flop per pixel-splat forward, 70 backward, against 48 B per splat).
//
// One kernel template per direction.  CULL = false: tiles of one 16x16 block, whose list is staged as it is.
// CULL = true: larger tiles, where a block stages only the entries of its tile's list that reach it.  The two
// forms share everything but how a round of the list gets into LDS (fwd_sweep_* / bwd_sweep_*).
#include "gs_ctx.h"
#include "gs_blend_geom.h"
#include "gs_cull.h"
#include "gs_wavesum.h"

namespace gs {

// what a blend kernel is launched with: one struct by value, filled once per launcher (op_args)
struct BlendOpArgs {
    BlockGeom geom;
    GsBackground bgc;
    const float4* packed12;       // a: mx my c00 c01 | b: c10 c11 r g | c: b opacity depth pad
    const uint32_t *sortedIdx, *tileRanges;
    // forward: what it writes
    float *outColor, *outDepth, *outAlpha;
    uint32_t* lastContrib;
    // backward: the cotangents, the forward's alpha and nContrib, the accumulator, the heaviest-first block order
    const float *cotColor, *cotDepth, *cotAlpha, *fwdAlpha;
    const uint32_t *fwdLast, *blockOrder;
    float* gradAcc16;
};

// a work item's 16x16 block, its tile's list, and (for the cull forms) the block's pixel rectangle
struct BlockList {
    BlockRect br;
    uint32_t start, count;
    float rx0, rx1, ry0, ry1;
};
__device__ __forceinline__ BlockList block_list(const BlendOpArgs& a, int blk)
{
    BlockList bl;
    bl.br = block_rect(a.geom, blk);
    const uint32_t end = a.tileRanges[2 * bl.br.tile + 1];
    bl.start = a.tileRanges[2 * bl.br.tile];
    bl.count = end > bl.start ? end - bl.start : 0u;
    bl.rx0 = (float)bl.br.x0; bl.rx1 = (float)(min(bl.br.x0 + TILE, bl.br.xEnd) - 1);
    bl.ry0 = (float)bl.br.y0; bl.ry1 = (float)(min(bl.br.y0 + TILE, bl.br.yEnd) - 1);
    return bl;
}

// -----------------------------------------------------------------------------------------------
// tiles LARGER than a 16x16 block (the reference app builds its renderer with TILE_SIZE = (W/4, H/4): 200x200 at 800x800)
//
// A block sweeps its TILE's list -- 30 k to 54 k entries at 200x200 on the bench scene -- of which only the entries near
// the block can move its pixels: the reference's semantics make every pixel blend every Gaussian of its tile, but a
// Gaussian whose weight exp(-q/2) is below 2^-29 on every pixel of the block moves no state by more than ~5e-8 (the
// fused kernels' staging cull, gs_cull.h).  Blending all of them took 4.5 ms forward, 15.8 ms backward; in the cull forms
// every thread tests one entry per round against the block's pixel rectangle -- a cheap sufficient test first: q >=
// lambda_min(conic) x distance^2 to the rectangle, then the exact rectangle minimum of the quadratic form --, the kept
// entries are compacted IN LIST ORDER into LDS with their list positions, and the sweep visits only those.  A block then
// pays for scanning its tile's list, not for blending it.  nContrib keeps its meaning (positions in the tile's list).
// -----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool block_reach(const BlockList& bl, const float4& a, const float4& b)
{
    const float X0 = bl.rx0 - a.x, X1 = bl.rx1 - a.x, Y0 = bl.ry0 - a.y, Y1 = bl.ry1 - a.y;
    // distance^2 from the mean to the rectangle (0 inside), and the smaller eigenvalue of the conic
    const float ddx = fmaxf(fmaxf(X0, -X1), 0.0f), ddy = fmaxf(fmaxf(Y0, -Y1), 0.0f);
    const float d2 = ddx * ddx + ddy * ddy;
    const float bb = 0.5f * (a.w + b.x), mid = 0.5f * (a.z + b.y), dif = 0.5f * (a.z - b.y);
    const float lmin = mid - sqrtf(dif * dif + bb * bb);
    // (1 % of slack covers the rounding of this bound against rect_min_q's own)
    if (lmin > 0.0f && lmin * d2 > CULL_QMIN * 1.01f) return false;
    return !(rect_min_q(a.z, a.w, b.x, b.y, X0, X1, Y0, Y1) > CULL_QMIN);
}

// ordered block-wide compaction: rank of this thread's kept entry among the kept ones with a LOWER thread id, and the
// total.  waveCnt: NT / 64 words of LDS; contains a barrier.
template <int NT>
__device__ __forceinline__ uint32_t kept_rank(bool keep, uint32_t* waveCnt, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) waveCnt[wv] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t off = 0; total = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) { const uint32_t c = waveCnt[i]; off += i < wv ? c : 0u; total += c; }
    return off + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// -----------------------------------------------------------------------------------------------
// forward
// -----------------------------------------------------------------------------------------------
// a lane's PPL pixels: pixel k of thread tid is pixel tid + k NT of the block, row-major
template <int PPL>
struct FwdPixels {
    float px[PPL], py[PPL], T[PPL], cr[PPL], cg[PPL], cb[PPL], dd[PPL];
    uint32_t nc[PPL];
    bool inside[PPL], done[PPL];
};

template <int PPL>
__device__ __forceinline__ void fwd_init(FwdPixels<PPL>& s, const BlockList& bl)
{
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        const int p = threadIdx.x + k * (256 / PPL);
        const int x = bl.br.x0 + (p & 15), y = bl.br.y0 + (p >> 4);
        s.inside[k] = x < bl.br.xEnd && y < bl.br.yEnd;
        s.done[k] = !s.inside[k];
        s.px[k] = (float)x; s.py[k] = (float)y;       // integer pixel coordinates (reference :555-556)
        s.T[k] = 1.0f; s.cr[k] = s.cg[k] = s.cb[k] = s.dd[k] = 0.0f;
        s.nc[k] = bl.count;
    }
}

template <int PPL>
__device__ __forceinline__ bool fwd_done(const FwdPixels<PPL>& s)
{
    bool d = true;
#pragma unroll
    for (int k = 0; k < PPL; k++) d = d && s.done[k];
    return d;
}

// the staged records [0, n) over the lane's pixels; pos1(j, c): list position + 1 of record j, whose third quarter is c
template <int PPL, class Pos>
__device__ __forceinline__ void fwd_blend_staged(FwdPixels<PPL>& s, const float4* sg, uint32_t n, Pos pos1)
{
    for (uint32_t j = 0; j < n; j++) {
        const float4 a = sg[j * 3], b = sg[j * 3 + 1], c = sg[j * 3 + 2];
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            if (!s.done[k]) {
                const float alpha = splat_alpha<true>(s.px[k], s.py[k], a, b, c.y).alpha;
                const float contrib = s.T[k] * alpha;
                s.cr[k] += contrib * b.z; s.cg[k] += contrib * b.w; s.cb[k] += contrib * c.x;
                s.dd[k] += contrib * c.z;
                s.T[k] = s.T[k] * (1.0f - alpha);
                if (s.T[k] < 1e-4f) { s.nc[k] = pos1(j, c); s.done[k] = true; }
            }
        }
        if (PPL > 1 && __all(fwd_done(s))) break;     // this wave has nothing left to do in the round
    }
}

template <int PPL>
__device__ __forceinline__ void fwd_store(const BlendOpArgs& a, const BlockList& bl, const FwdPixels<PPL>& s)
{
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        if (s.inside[k]) {
            const int p = threadIdx.x + k * (256 / PPL);
            const int x = bl.br.x0 + (p & 15), y = bl.br.y0 + (p >> 4);
            const size_t pix = (size_t)y * a.geom.W + x;
            float bg0, bg1, bg2;
            gs_bg_terms(a.bgc, s.T[k], bg0, bg1, bg2);
            a.outColor[3 * pix] = s.cr[k] + bg0; a.outColor[3 * pix + 1] = s.cg[k] + bg1; a.outColor[3 * pix + 2] = s.cb[k] + bg2;
            if (a.outDepth) a.outDepth[pix] = s.dd[k];
            a.outAlpha[pix] = 1.0f - s.T[k];
            a.lastContrib[pix] = s.nc[k];
        }
    }
}

// the whole list, NT entries per chunk: one coalesced index burst and one record gather per thread
template <int PPL>
__device__ __forceinline__ void fwd_sweep_plain(const BlendOpArgs& a, const BlockList& bl, FwdPixels<PPL>& s, float4* sg)
{
    constexpr int NT = 256 / PPL;
    const int tid = threadIdx.x;
    for (uint32_t chunk = 0; chunk < bl.count; chunk += NT) {
        const bool allDone = fwd_done(s);
        if (__syncthreads_and(allDone)) break;    // also fences the previous chunk's LDS reads
        const uint32_t i = chunk + tid;
        if (i < bl.count) {
            const float4* src = a.packed12 + (size_t)a.sortedIdx[bl.start + i] * 3;
            sg[tid * 3 + 0] = src[0];
            sg[tid * 3 + 1] = src[1];
            sg[tid * 3 + 2] = src[2];
        }
        __syncthreads();
        if (!allDone)
            fwd_blend_staged(s, sg, min((uint32_t)NT, bl.count - chunk),
                             [chunk](uint32_t j, const float4&) { return chunk + j + 1; });
    }
}

// NT list positions per round, of which the entries that reach the block are staged, each with its list position + 1
template <int PPL>
__device__ __forceinline__ void fwd_sweep_cull(const BlendOpArgs& a, const BlockList& bl, FwdPixels<PPL>& s, float4* sg,
                                               uint32_t* waveCnt)
{
    constexpr int NT = 256 / PPL;
    const int tid = threadIdx.x;
    const uint32_t count = bl.count;
    const uint32_t* idx = a.sortedIdx + bl.start;
    // records one round ahead, indices two: each is a dependent memory latency
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
    if ((uint32_t)tid < count) {
        const float4* src = a.packed12 + (size_t)idx[tid] * 3;
        ra = src[0]; rb = src[1]; rc = src[2];
    }
    uint32_t gAhead = (uint32_t)(NT + tid) < count ? idx[NT + tid] : 0u;
    for (uint32_t base = 0; base < count; base += NT) {
        const bool allDone = fwd_done(s);
        if (__syncthreads_and(allDone)) break;        // also fences the previous round's LDS reads
        const uint32_t i = base + tid;
        const float4 ea = ra, eb = rb, ec = rc;
        const bool keep = i < count && block_reach(bl, ea, eb);
        if (i + NT < count) {
            const float4* src = a.packed12 + (size_t)gAhead * 3;
            ra = src[0]; rb = src[1]; rc = src[2];
        }
        gAhead = i + 2u * NT < count ? idx[i + 2u * NT] : 0u;
        uint32_t total;
        const uint32_t pos = kept_rank<NT>(keep, waveCnt, total);
        if (keep) {
            sg[pos * 3 + 0] = ea;
            sg[pos * 3 + 1] = eb;
            sg[pos * 3 + 2] = make_float4(ec.x, ec.y, ec.z, __uint_as_float(i + 1u));
        }
        __syncthreads();
        if (!allDone) fwd_blend_staged(s, sg, total, [](uint32_t, const float4& c) { return __float_as_uint(c.w); });
    }
}

template <int PPL, bool CULL>
__global__ __launch_bounds__(256 / PPL) void blend_fwd_kernel(BlendOpArgs a)
{
    constexpr int NT = 256 / PPL;
    __shared__ float4 sg[NT * 3];
    const BlockList bl = block_list(a, (int)blockIdx.x);
    FwdPixels<PPL> s;
    fwd_init(s, bl);
    if constexpr (CULL) {
        __shared__ uint32_t waveCnt[NT / 64];
        fwd_sweep_cull(a, bl, s, sg, waveCnt);
    } else fwd_sweep_plain(a, bl, s, sg);
    fwd_store(a, bl, s);
}

// -----------------------------------------------------------------------------------------------
// backward
// -----------------------------------------------------------------------------------------------
struct PixGrad {
    float v[11];   // mx my c00 c01 c10 c11 r g b opacity depth
};

// one (pixel, splat) step of the reverse sweep; updates T and cotT, accumulates into acc
__device__ __forceinline__ void bwd_step(const float4& a, const float4& b, const float4& c, float px, float py,
                                         float cCx, float cCy, float cCz, float cD, float& T, float& cT,
                                         PixGrad& acc)
{
    const SplatAlpha s = splat_alpha<false>(px, py, a, b, c.y);
    const float dx = s.dx, dy = s.dy, ex = s.ex, alpha = s.alpha;
    // undoTileGlobalPixelState (:501-521)
    float denom = 1.0f - alpha;
    if (denom < 1e-6f) denom = 1e-6f;
    const float Tprev = T * __builtin_amdgcn_rcpf(denom);   // v_rcp_f32 (1 ulp): within the 1e-3 gradient bar
    const float contrib = Tprev * alpha;
    // reverse of updateTileGlobalPixelState
    // (c.z cD + c.x cCz + b.w cCy + b.z cCx, written out: which of the first two products is rounded is otherwise the
    // optimiser's choice, and has differed between instantiations of one source)
    const float S13 = fmaf(b.z, cCx, fmaf(b.w, cCy, fmaf(c.z, cD, c.x * cCz)));
    const float dAlpha = -(Tprev * cT) + Tprev * S13;
    cT = (1.0f - alpha) * cT + alpha * S13;
    T = Tprev;
    // reverse of tileGlobalAlphaFromGaussian: the clamp passes iff raw <= 0.99
    const float S32 = s.raw > 0.99f ? 0.0f : dAlpha;
    const float dE = c.y * S32 * ex;
    const float S36 = -0.5f * dE;
    const float S39 = dy * (b.y * S36);
    const float S41 = dx * (a.z * S36);
    const float S42 = b.x * S36 + a.w * S36;
    acc.v[0] += -(S41 + S41 + dy * S42);
    acc.v[1] += -(S39 + S39 + dx * S42);
    acc.v[2] += dx * dx * S36;
    const float S37 = s.dxdy * S36;
    acc.v[3] += S37;
    acc.v[4] += S37;
    acc.v[5] += dy * dy * S36;
    acc.v[6] += contrib * cCx;
    acc.v[7] += contrib * cCy;
    acc.v[8] += contrib * cCz;
    acc.v[9] += ex * S32;
    acc.v[10] += contrib * cD;
}

constexpr int BWD_BATCH = 64;    // staged entries per reduce-and-flush round

template <int PPL>
struct BwdPixels {
    float px[PPL], py[PPL], T[PPL], cT[PPL], cCx[PPL], cCy[PPL], cCz[PPL], cD[PPL];
    uint32_t nc[PPL];
    uint32_t waveMax, blockMax;   // of nContrib: the sweep starts there, not at the end of the list
};

// smax: NT / 64 words of LDS; contains a barrier where the block has more than one wave
template <int PPL>
__device__ __forceinline__ void bwd_load(BwdPixels<PPL>& s, const BlendOpArgs& a, const BlockList& bl, uint32_t* smax)
{
    constexpr int NT = 256 / PPL, NW = NT / 64;
    uint32_t myMax = 0;
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        const int p = threadIdx.x + k * NT;
        const int x = bl.br.x0 + (p & 15), y = bl.br.y0 + (p >> 4);
        s.px[k] = (float)x; s.py[k] = (float)y;
        s.nc[k] = 0; s.T[k] = 0.f; s.cT[k] = 0.f; s.cCx[k] = s.cCy[k] = s.cCz[k] = s.cD[k] = 0.f;
        if (x < bl.br.xEnd && y < bl.br.yEnd) {
            const size_t pix = (size_t)y * a.geom.W + x;
            s.cCx[k] = a.cotColor[3 * pix]; s.cCy[k] = a.cotColor[3 * pix + 1]; s.cCz[k] = a.cotColor[3 * pix + 2];
            s.cD[k] = a.cotDepth ? a.cotDepth[pix] : 0.0f;
            const float cA = a.cotAlpha ? a.cotAlpha[pix] : 0.0f;
            s.T[k] = 1.0f - a.fwdAlpha[pix];
            s.cT[k] = -cA + gs_bg_cot(a.bgc, s.cCx[k], s.cCy[k], s.cCz[k]);
            s.nc[k] = min(a.fwdLast[pix], bl.count);
        }
        myMax = max(myMax, s.nc[k]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) myMax = max(myMax, (uint32_t)__shfl_xor((int)myMax, d, 64));
    s.waveMax = s.blockMax = myMax;
    if (NW > 1) {
        if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = myMax;
        __syncthreads();
        s.blockMax = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) s.blockMax = max(s.blockMax, smax[i]);
    }
}

// One reduce-and-flush round over the staged entries [0, m), m <= BWD_BATCH, which lie in sweep order: records sg, Gaussian
// indices sidx, list positions pos(e).  Every wave runs its pixels through the entries and leaves its ten sums per entry in
// part[]; then one row per entry, summed over the block's waves, goes to the accumulator with f32 atomics.
// The caller's barrier in front of the next round covers the flush's reads of part[] and sidx[].
template <int PPL, class Pos>
__device__ __forceinline__ void bwd_round(BwdPixels<PPL>& s, const float4* sg, const uint32_t* sidx, uint32_t m, Pos pos,
                                          float (*part)[BWD_BATCH][12], float* gradAcc16)
{
    constexpr int NT = 256 / PPL, NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (uint32_t e = 0; e < m; e++) {
        const uint32_t ii = pos(e);
        float w = 0.0f;
        if (ii < s.waveMax) {            // wave-uniform: some lane of this wave still has this splat
            PixGrad acc;
#pragma unroll
            for (int q = 0; q < 11; q++) acc.v[q] = 0.0f;
            const float4 a = sg[e * 3], b = sg[e * 3 + 1], c = sg[e * 3 + 2];
#pragma unroll
            for (int k = 0; k < PPL; k++)
                if (ii < s.nc[k])
                    bwd_step(a, b, c, s.px[k], s.py[k], s.cCx[k], s.cCy[k], s.cCz[k], s.cD[k], s.T[k], s.cT[k], acc);
            // ten sums (dc10 is dc01 again); the totals come out at lanes 4 s of rows 0..2:
            //   slot s:  0 dmx  1 dc00  2 dmy  3 dc01 | 4 5 dop  6 7 ddepth | 8 dc11  9 dg  10 dr  11 db
            const float u[10] = {acc.v[0], acc.v[1], acc.v[2], acc.v[3], acc.v[5], acc.v[6], acc.v[7], acc.v[8],
                                 acc.v[9], acc.v[10]};
            w = wave_sum10_transposed<false>(u);
        }
        if ((lane & 3) == 0 && lane < 48) part[wv][e][lane >> 2] = w;
    }
    __syncthreads();
    for (uint32_t x = tid; x < m * 11; x += NT) {
        const uint32_t e = x / 11, q = x - e * 11;
        // packed column q (dmx dmy dc00 dc01 dc10 dc11 dr dg db dop ddepth) <- slot
        const uint32_t slot = (0x64b9a833120ull >> (q * 4)) & 15u;       // 0 2 1 3 3 8 10 9 11 4 6
        float v = part[0][e][slot];
#pragma unroll
        for (int w2 = 1; w2 < NW; w2++) v += part[w2][e][slot];
        if (v != 0.0f) atomicAdd(&gradAcc16[(size_t)sidx[e] * 16 + q], v);
    }
}

// the list below blockMax in chunks of BWD_BATCH, last chunk first: one coalesced burst per chunk, thread t taking the
// chunk's t-th position from its end (sweep order)
template <int PPL>
__device__ __forceinline__ void bwd_sweep_plain(const BlendOpArgs& a, const BlockList& bl, BwdPixels<PPL>& s, float4* sg,
                                                uint32_t* sidx, float (*part)[BWD_BATCH][12])
{
    const uint32_t tid = threadIdx.x;
    for (int ch = (int)((s.blockMax + BWD_BATCH - 1) / BWD_BATCH) - 1; ch >= 0; ch--) {
        const uint32_t chunkStart = (uint32_t)ch * BWD_BATCH;
        const uint32_t last = min(chunkStart + BWD_BATCH, s.blockMax) - 1u;
        __syncthreads();     // previous chunk's flush has finished reading part[] / sidx[]
        if (chunkStart + tid <= last) {
            const uint32_t g = a.sortedIdx[bl.start + last - tid];
            sidx[tid] = g;
            const float4* src = a.packed12 + (size_t)g * 3;
            sg[tid * 3 + 0] = src[0];
            sg[tid * 3 + 1] = src[1];
            sg[tid * 3 + 2] = src[2];
        }
        __syncthreads();
        bwd_round(s, sg, sidx, last - chunkStart + 1u, [last](uint32_t e) { return last - e; }, part, a.gradAcc16);
    }
}

// the reverse sweep over a large tile's list: NT list positions per round, highest first, the kept entries compacted in
// sweep order; per batch of BWD_BATCH kept entries one reduce-and-flush round
template <int PPL>
__device__ __forceinline__ void bwd_sweep_cull(const BlendOpArgs& a, const BlockList& bl, BwdPixels<PPL>& s, float4* sg,
                                               uint32_t* sidx, uint32_t* spos, uint32_t* waveCnt,
                                               float (*part)[BWD_BATCH][12])
{
    constexpr int NT = 256 / PPL;
    const int tid = threadIdx.x;
    const uint32_t* idx = a.sortedIdx + bl.start;
    const int rounds = (int)((s.blockMax + NT - 1) / NT);
    // thread t of a round takes position base + NT - 1 - t: ascending thread id = descending list position = sweep order
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
    uint32_t gCur = 0u, gAhead = 0u;
    {
        const uint32_t i0 = (uint32_t)(rounds - 1) * NT + (uint32_t)(NT - 1 - tid);
        if (i0 < s.blockMax) {
            gCur = idx[i0];
            const float4* src = a.packed12 + (size_t)gCur * 3;
            ra = src[0]; rb = src[1]; rc = src[2];
        }
        if (rounds >= 2) gAhead = idx[(uint32_t)(rounds - 2) * NT + (uint32_t)(NT - 1 - tid)];
    }
    for (int r = rounds - 1; r >= 0; r--) {
        const uint32_t i = (uint32_t)r * NT + (uint32_t)(NT - 1 - tid);
        __syncthreads();         // the previous round's flush has finished reading sidx[] / part[]
        const float4 ea = ra, eb = rb, ec = rc;
        const uint32_t g = gCur;
        const bool keep = i < s.blockMax && block_reach(bl, ea, eb);
        if (r >= 1) {            // (every position of the rounds below is inside the sweep)
            gCur = gAhead;
            const float4* src = a.packed12 + (size_t)gCur * 3;
            ra = src[0]; rb = src[1]; rc = src[2];
            gAhead = r >= 2 ? idx[(uint32_t)(r - 2) * NT + (uint32_t)(NT - 1 - tid)] : 0u;
        }
        uint32_t total;
        const uint32_t pos = kept_rank<NT>(keep, waveCnt, total);
        if (keep) {
            sg[pos * 3 + 0] = ea; sg[pos * 3 + 1] = eb; sg[pos * 3 + 2] = ec;
            sidx[pos] = g; spos[pos] = i;
        }
        __syncthreads();
        for (uint32_t batch = 0; batch < total; batch += BWD_BATCH) {
            if (batch) __syncthreads();          // the previous batch's flush has finished reading part[]
            const uint32_t* bpos = spos + batch;
            bwd_round(s, sg + batch * 3, sidx + batch, min((uint32_t)BWD_BATCH, total - batch),
                      [bpos](uint32_t e) { return bpos[e]; }, part, a.gradAcc16);
        }
    }
}

template <int PPL, bool CULL>
__global__ __launch_bounds__(256 / PPL) void blend_bwd_kernel(BlendOpArgs a)
{
    constexpr int NT = 256 / PPL, NW = NT / 64;
    constexpr int SLOTS = CULL ? NT : BWD_BATCH;      // entries staged at a time
    __shared__ float4 sg[SLOTS * 3];
    __shared__ uint32_t sidx[SLOTS];
    __shared__ float part[NW][BWD_BATCH][12];
    __shared__ uint32_t smax[NW];
    const BlockList bl = block_list(a, (int)a.blockOrder[blockIdx.x]);      // heaviest blocks are dispatched first
    if (bl.count == 0) return;
    BwdPixels<PPL> s;
    bwd_load(s, a, bl, smax);
    if (s.blockMax == 0) return;
    if constexpr (CULL) {
        __shared__ uint32_t spos[NT];
        __shared__ uint32_t waveCnt[NW];
        bwd_sweep_cull(a, bl, s, sg, sidx, spos, waveCnt, part);
    } else bwd_sweep_plain(a, bl, s, sg, sidx, part);
}

__global__ void gradacc_to_packed11_kernel(int N, const float* __restrict__ acc16, float* __restrict__ out11)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 11) return;
    const int g = i / 11, q = i - g * 11;
    out11[i] = acc16[(size_t)g * 16 + q];
}

// -----------------------------------------------------------------------------------------------
// heaviest-first block order of the backward.  All ~2500 workgroups of an 800x800 frame are resident at once, so a
// workgroup's CU is fixed at launch and per-CU work is whatever the round-robin deal happens to sum to
// (tile lists run from 0 to thousands of splats).  Dealing the blocks in descending-work order gives every
// CU a stratified sample of the distribution: per-CU sums differ by at most about one heavy tile.
// The forward keeps the natural order: the list length says little about where a saturating tile stops
// (correlation 0.07 with the measured sweep length on the bench scene).
// -----------------------------------------------------------------------------------------------
// exact sweep length = max nContrib over the block's pixels (one wave per block)
__global__ __launch_bounds__(64) void block_work_contrib_kernel(BlockGeom geom,
                                                                const uint32_t* __restrict__ lastContrib,
                                                                uint32_t* __restrict__ work)
{
    const int b = blockIdx.x;
    const BlockRect br = block_rect(geom, b);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = threadIdx.x + k * 64;
        const int x = br.x0 + (p & 15), y = br.y0 + (p >> 4);
        if (x < br.xEnd && y < br.yEnd) m = max(m, lastContrib[(size_t)y * geom.W + x]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if (threadIdx.x == 0) work[b] = m;
}

// single workgroup: approximate heaviest-first order by a 256-bucket counting sort on work / max(work)
// (only the rank strata matter, not the exact order)
__global__ __launch_bounds__(1024) void order_blocks_kernel(int n, const uint32_t* __restrict__ work,
                                                            uint32_t* __restrict__ order)
{
    __shared__ uint32_t bucket[256];
    __shared__ uint32_t wmax;
    if (threadIdx.x < 256) bucket[threadIdx.x] = 0;
    if (threadIdx.x == 0) wmax = 0;
    __syncthreads();
    uint32_t m = 0;
    for (int i = threadIdx.x; i < n; i += 1024) m = max(m, work[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&wmax, m);
    __syncthreads();
    const float scale = 255.0f / (float)(wmax + 1u);
    // bucket 0 = heaviest
    for (int i = threadIdx.x; i < n; i += 1024) atomicAdd(&bucket[255 - (int)((float)work[i] * scale)], 1u);
    __syncthreads();
    if (threadIdx.x < 64) {   // exclusive scan of 256 counts by one wave (4 per lane)
        uint32_t c[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { c[k] = bucket[threadIdx.x * 4 + k]; sum += c[k]; }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if ((int)threadIdx.x >= d) incl += t;
        }
        uint32_t run = incl - sum;
#pragma unroll
        for (int k = 0; k < 4; k++) { bucket[threadIdx.x * 4 + k] = run; run += c[k]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const uint32_t pos = atomicAdd(&bucket[255 - (int)((float)work[i] * scale)], 1u);
        order[pos] = (uint32_t)i;
    }
}

static int launch_block_order(gs_ctx* c, const uint32_t* work)
{
    const int n = c->opBlocks;
    hipLaunchKernelGGL(order_blocks_kernel, dim3(1), dim3(1024), 0, c->stream, n, work, c->blockOrder);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// -----------------------------------------------------------------------------------------------
// launchers
// -----------------------------------------------------------------------------------------------
static BlendOpArgs op_args(const gs_ctx* c, const GsBackground& bg)
{
    BlendOpArgs a = {};
    BlockGeom& g = a.geom;
    g.W = c->W; g.H = c->H; g.tileW = c->tileW; g.tileH = c->tileH; g.gridW = c->gridW; g.blocksX = gs_div_up(c->W, TILE);
    g.bptX = c->fast16 ? 0 : gs_div_up(c->tileW, TILE);
    g.bptY = c->fast16 ? 0 : gs_div_up(c->tileH, TILE);
    a.bgc = bg;
    a.packed12 = reinterpret_cast<const float4*>(c->packed12); a.sortedIdx = c->sortedIdx; a.tileRanges = c->tileRanges;
    a.blockOrder = c->blockOrder; a.gradAcc16 = c->gradAcc16;
    return a;
}

// a tile of more than one block: scan, cull, sweep the rest
static bool op_cull(const gs_ctx* c) { return c->tileW > TILE || c->tileH > TILE; }

template <int PPL, bool CULL>
static void launch_fwd(gs_ctx* c, const BlendOpArgs& a)
{
    hipLaunchKernelGGL((blend_fwd_kernel<PPL, CULL>), dim3(c->opBlocks), dim3(256 / PPL), 0, c->stream, a);
}
template <int PPL, bool CULL>
static void launch_bwd(gs_ctx* c, const BlendOpArgs& a)
{
    hipLaunchKernelGGL((blend_bwd_kernel<PPL, CULL>), dim3(c->opBlocks), dim3(256 / PPL), 0, c->stream, a);
}

int launch_blend_forward(gs_ctx* c, const GsBackground& bg, float* outColor, float* outDepth, float* outAlpha, uint32_t* lastContrib)
{
    BlendOpArgs a = op_args(c, bg);
    a.outColor = outColor; a.outDepth = outDepth; a.outAlpha = outAlpha; a.lastContrib = lastContrib;
    const int ppl = c->opFwdPpl == 4 || c->opFwdPpl == 2 ? c->opFwdPpl : 1;
    switch (ppl + (op_cull(c) ? 8 : 0)) {
    case 1: launch_fwd<1, false>(c, a); break;
    case 2: launch_fwd<2, false>(c, a); break;
    case 4: launch_fwd<4, false>(c, a); break;
    case 9: launch_fwd<1, true>(c, a); break;
    case 10: launch_fwd<2, true>(c, a); break;
    case 12: launch_fwd<4, true>(c, a); break;
    }
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

// accumulates d(packed) into ctx->gradAcc16 (zeroed here)
int launch_blend_backward(gs_ctx* c, const GsBackground& bg, int N, const float* cotColor, const float* cotDepth, const float* cotAlpha,
                          const float* outAlpha, const uint32_t* lastContrib)
{
    GS_HIP_CHECK(c, hipMemsetAsync(c->gradAcc16, 0, sizeof(float) * 16 * (size_t)N, c->stream));
    BlendOpArgs a = op_args(c, bg);
    a.cotColor = cotColor; a.cotDepth = cotDepth; a.cotAlpha = cotAlpha; a.fwdAlpha = outAlpha; a.fwdLast = lastContrib;
    // (the ctx's own scratch: a caller's view-hint buffer holds one word per block of the IMAGE grid, which a tile size
    // that is not a multiple of 16 exceeds)
    uint32_t* work = c->fast16 ? c->blockWork : c->blockWorkOwn;
    hipLaunchKernelGGL(block_work_contrib_kernel, dim3(c->opBlocks), dim3(64), 0, c->stream, a.geom, lastContrib, work);
    const int rc = launch_block_order(c, work);
    if (rc) return rc;
    // (cull: two pixels per lane unless the knob says four: 1.54 -> 1.44 ms at 200x200)
    const bool cull = op_cull(c);
    const int ppl = c->opBwdPpl == 4 ? 4 : (c->opBwdPpl == 2 || cull) ? 2 : 1;
    switch (ppl + (cull ? 8 : 0)) {
    case 1: launch_bwd<1, false>(c, a); break;
    case 2: launch_bwd<2, false>(c, a); break;
    case 4: launch_bwd<4, false>(c, a); break;
    case 10: launch_bwd<2, true>(c, a); break;
    case 12: launch_bwd<4, true>(c, a); break;
    }
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_gradacc_to_packed11(gs_ctx* c, int N, float* gradPacked11)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(gradacc_to_packed11_kernel, dim3(gs_div_up((long long)N * 11, 256)), dim3(256), 0, c->stream,
                       N, c->gradAcc16, gradPacked11);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
