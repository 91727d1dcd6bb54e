// blend_v2.hip -- the fused path's alpha-blend kernels (gs_render_forward / gs_render_backward*).
//
// Same arithmetic as blend.hip (which keeps serving the op-level entry points), different mapping.  What the
// measurements on MI355X said (tools/microbench.hip, tools/fwd_trace.py, tools/pmc_fwd.sh):
//
//  * Issue rates, cycles per wave64 instruction per SIMD: v_mul/add/sub/fmac_f32, v_mov, integer add/and/shift
//    2.6-3.0; v_min/max/med3_f32, v_cmp, v_cndmask, v_bfi 4.2-4.5; v_exp_f32 / v_rcp_f32 8.3; v_pk_*_f32 4.8 (no
//    packed advantage); v_readlane_b32 12; DPP add 4.2; v_permlane{16,32}_swap 13.6.  Both kernels end up bound by
//    f32 instruction issue (SQ counters: forward ~100 %, backward 96 % VALU-busy), so the levers are instruction
//    count and not doing work.  The file is built with -fno-slp-vectorize: the SLP vectoriser's v_pk_* forms buy
//    nothing here and cost ~8 v_mov per splat in operand shuffles.
//  * Every wavefront is autonomous: it gathers 64 list entries at a time, one per lane (a coalesced index burst +
//    three 16-B loads per lane), parks them in a wave-private LDS slot and reads entry j back as three broadcast
//    ds_read_b128.  No workgroup barriers; the next 64 entries are in flight while the current ones are blended.
//    (v_readlane broadcast: 131 cycles per record; scalar loads: two dependent scalar-cache misses per group.)
//  * Staging COMPACTS: lane j evaluates, in closed form, the minimum of entry j's quadratic form over the wave's
//    pixel rectangle (rect_min_q) and drops the entry if exp(-q/2) is below 2^-29 = 2e-9 on every pixel (CULL_QMIN).
//    The reference blends everything in its bounding squares, which are much larger than the ellipses; what is
//    dropped moves no rendered value by more than ~5e-8 per entry, and the image's distance to the oracle does not
//    change in the third digit (measured for thresholds 2^-42 ... 2^-24.5; at 2^-20 it does).  Dropped entries cost
//    no LDS broadcast and no VALU.
//  * Forward (blend_fwd_v2q_kernel; "forward" below): one wavefront per 8x8 quadrant of a 16x16 block, one pixel per lane,
//    four splats per trip (exponents and exps first, the short serial chain through T second), branch-free termination
//    (a finished pixel keeps blending with alpha = 0), wave-uniform exit.  Persistent waves: a static first item each, the
//    rest from eight device queues, deepest blocks first.  Every SEG list positions the running state (T, C, D) is saved
//    per pixel.  blend_fwd_v2p_kernel and blend_fwd_v2w_kernel are the same sweep on other schedules.
//  * Backward (blend_bwd_v2_kernel; "backward" below): the saved states make a tile's list SEGMENT-parallel.  The work items
//    are (pixel block, segment) pairs of at most SEG list positions, handed to persistent single-wave workgroups like the
//    forward's.  Inside an item the sweep runs FORWARD (T by multiplication, as the forward pass), with the cotangent of T
//    in closed form,
//        c_i = (sum_{j>i} T_j a_j S_j + T_n cT_n) / T_{i+1},
//    the sum being (final colour - running colour) . cotColour.  Each lane owns 4 pixels, so the per-splat wave
//    reduction is paid once per 256 pixel-splats; it is a TRANSPOSED reduction (gs_wavesum.h): lane swaps and bank-masked
//    DPP adds halve the live registers level by level, 23 instructions instead of 60.
//  * The reference rebuilds T from the rounded output alpha (T_n' = 1 - outAlpha) and divides its way back;
//    every T of a pixel is therefore off by the factor s = T_n' / T_n.  The same factor is applied here, so
//    the gradients match the reference's arithmetic, not just the exact calculus.
//
// Compiled with -ffp-contract=off and explicit fmaf so that forward and backward evaluate the running sums
// bit-identically (the closed form needs the backward's recomputed colour to meet the forward's).
#include "gs_ctx.h"
#include "gs_bwd_prep.h"
#include "gs_cull.h"
#include "gs_wavesum.h"

namespace gs {

constexpr int BLK = 16;
constexpr uint32_t CKPT_POOL_MAX = 8;   // checkpoint slots a forward wave takes from the arena's shared part per atomic: this many
                                        // when the arena is roomy, fewer when a part of it holds less than that per wave (ckpt_pool)
                                        // -- or the waves' unused remainders use up a tiny reserve (~10 k slots for 4 - 5 k waves) and
                                        // every forward reports an arena overflow until the regrow (tools/dp_overflow_rehearsal.py)
static inline uint32_t ckpt_pool(uint32_t partSlots, uint32_t waves)
{
    const uint32_t perWave = partSlots / (waves / 8u + 1u);
    return perWave >= CKPT_POOL_MAX ? CKPT_POOL_MAX : (perWave < 1u ? 1u : perWave);
}

struct Rec {
    float mx, my, c00, c01, c10, c11, r, g, b, op, depth;
};

#ifndef GS_FWD_PREFETCH
#define GS_FWD_PREFETCH 1      // register sets of the one-wave forward's record pipeline (blend_fwd_v2q_kernel)
#endif

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// one record per lane (lane j of a chunk holds splat chunkStart + j of the list)
struct RecV {
    f4 a, b, c;
};

__device__ __forceinline__ RecV load_chunk(const float4* __restrict__ packed12, const uint32_t* __restrict__ idx,
                                           uint32_t idxMask, uint32_t i0, uint32_t iEnd, int lane)
{
    RecV v;
    v.a = v.b = v.c = (f4){0.f, 0.f, 0.f, 0.f};
    if (i0 + lane < iEnd) {
        const f4* p = reinterpret_cast<const f4*>(packed12) + (size_t)(idx[i0 + lane] & idxMask) * 3;
        v.a = p[0]; v.b = p[1]; v.c = p[2];
    }
    return v;
}

// the same in two steps, so that the list index of chunk c + 2 can be in flight while the records of chunk c + 1 are
// gathered: otherwise the gather waits for its index first, two memory latencies in a row per chunk, which is what a
// deep quadrant that runs alone at the end of the kernel spends its time on
__device__ __forceinline__ uint32_t load_chunk_index(const uint32_t* __restrict__ idx, uint32_t idxMask, uint32_t i0,
                                                     uint32_t iEnd, int lane)
{
    return i0 + lane < iEnd ? idx[i0 + lane] & idxMask : 0xFFFFFFFFu;
}
__device__ __forceinline__ RecV gather_chunk(const float4* __restrict__ packed12, uint32_t g)
{
    RecV v;
    v.a = v.b = v.c = (f4){0.f, 0.f, 0.f, 0.f};
    if (g != 0xFFFFFFFFu) {
        const f4* p = reinterpret_cast<const f4*>(packed12) + (size_t)g * 3;
        v.a = p[0]; v.b = p[1]; v.c = p[2];
    }
    return v;
}

__device__ __forceinline__ Rec unpack(const f4 a, const f4 b, const f4 c)
{
    Rec r;
    r.mx = a.x; r.my = a.y; r.c00 = a.z; r.c01 = a.w;
    r.c10 = b.x; r.c11 = b.y; r.r = b.z; r.g = b.w;
    r.b = c.x; r.op = c.y; r.depth = c.z;
    return r;
}

// exp(-q/2) = 2^(q C), C = -1/(2 ln 2).  In f32 the product q C1 (C1 = fl(C)) is rounded to |q C1| 2^-24: a relative
// error of the result of up to ~1e-6 for the exponents that still matter (|q C| ~ 10-20), which is what separated this
// forward from the oracle's libm exp by 3.4e-4 on the bench scene's colours of magnitude ~27.
// The forward therefore carries the product's rounding error lo = fma(q, C1, -hi) (exact) and C's own tail C2 along:
//   exp(-q/2) = 2^hi (1 + (lo + q C2) ln 2),   four more VALU instructions per pixel-splat
// (measured: L-inf 3.41e-4 -> 4.3e-5 against the float32 oracle, the same as with the device math library's expf at a
// third of its cost; blend forward 0.195 -> 0.207 ms).  -DGS_EXP_PLAIN builds the uncompensated forward.  The backward
// only needs alpha to ~1e-6 (gradients are held to 1e-3): it stays plain, and evaluates the quadratic form with a
// pre-multiplied conic instead of in the reference's order (RecB, pair_exponent_bwd).
constexpr float EXP_C1 = -0.72134751081466675f;      // fl(-1 / (2 ln 2))
constexpr float EXP_C2LN2 = -6.674879e-09f;          // (C - C1) ln 2
constexpr float EXP_LN2 = 0.69314718055994531f;

// opacity * exp(-q/2)
__device__ __forceinline__ float gauss_alpha_raw(float q, float op)
{
    const float hi = q * EXP_C1;
#ifndef GS_EXP_PLAIN
    const float lo = fmaf(q, EXP_C1, -hi);
    const float d = fmaf(q, EXP_C2LN2, lo * EXP_LN2);
    const float g = __builtin_amdgcn_exp2f(hi);
    return op * fmaf(g, d, g);
#else
    return op * __builtin_amdgcn_exp2f(hi);
#endif
}

// (cull bound CULL_QMIN and rect_min_q: gs_cull.h)

// ---------------------------------------------------------------------------------------------
// what the forward and the backward kernels share besides the records
// ---------------------------------------------------------------------------------------------
// A word of a table a kernel only reads (blockOrder, tileRanges, segBase, the depth cuts, the item list, the sweep
// lengths: written by the launches in front of it), through the constant address space: at a wave-uniform index it is a
// scalar load.  Flat __restrict__ kernel arguments say as much; the members of a by-value argument struct carry no such
// promise, and the forward item's dependent chain of three look-ups came out as vector loads + v_readfirstlane (blend forward
// on the 300 k / 800x800 scene: 0.1658 -> 0.1676 ms, one-wave kernel).
__device__ __forceinline__ uint32_t table_word(const uint32_t* table, uint32_t i)
{
    return ((const __attribute__((address_space(4))) uint32_t*)table)[i];
}

// kept entries in the lanes below this one, from the ballot of the keepers (v_mbcnt: written as popc(m & ((1 << lane) - 1)),
// the 64-bit lane mask became a loop invariant of the item loop that the four-wave forward, at its register budget, kept in
// scratch)
__device__ __forceinline__ uint32_t rank_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One pop from the work queues, called by a whole wave: the nq queues are tried from the taker's own XCD's on, the ones
// found empty (`dead`) skipped.  Lane 0 takes a ticket k from queue y and the wave reads it back; take(y, k) maps it to an
// item and says whether there was one -- if not, queue y is empty, and since tickets only grow it stays so.  False: every
// queue is empty.
// (No look before the pop: a load of the line the pops hammer queues behind them -- measured, forward, one queue: 0.19 ->
// 0.49 ms with a relaxed load in front of every atomicAdd.  And popping the next item ahead of time was measured slower in
// the backward: vector-memory results return in order, so the current item's first record load waits behind the atomic.)
template <class Take>
__device__ __forceinline__ bool queue_pop(uint32_t* queues, uint32_t nq, uint32_t xcd, uint32_t& dead, int lane, Take take)
{
    bool got = false;
    for (uint32_t t = 0; t < nq && !got; t++) {
        const uint32_t y = (xcd + t) % nq;
        if ((dead >> y) & 1u) continue;
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(&queues[y * GS_QUEUE_STRIDE], 1u);
        k = __builtin_amdgcn_readfirstlane(k);
        got = take(y, k);
        if (!got) dead |= 1u << y;
    }
    return got;
}

// ---------------------------------------------------------------------------------------------
// segment bookkeeping
// ---------------------------------------------------------------------------------------------
// segBase[b] = index of pixel block b's first saved state (state before splat SEG); exclusive scan of
// max(ceil(count/SEG) - 1, 0).  One workgroup.
template <int SEG>
__global__ __launch_bounds__(1024) void seg_base_kernel(SegBaseArgs a)
{
    __shared__ uint32_t lds[GS_SEGBASE_LDS];
    seg_base_body<SEG>(a, lds);
}

// work items of the backward: (block, segment) for segment < ceil(blockWork/SEG).  One workgroup.
// It also renews the view's depth cuts (binning.hip) when the caller keeps them (cutStore != nullptr; 16x16 tiles, so
// tile = block): the cut of a tile whose sweep stopped `work` entries into a list of `len` is the depth key of entry
// 2 work + 128 if the list goes on beyond that (on the bench scene sweeps grow by up to 1.85x between two visits of a
// view; with work + work/4 + 64 a handful of the 2500 tiles missed in nearly every forward); a cut that was in force
// this forward (cutsInForce) and still leaves 1.5 work + 64 entries is kept; anything else means "bin everything
// next time".
template <int SEG>
__global__ __launch_bounds__(1024) void bwd_items_kernel(BwdPrepArgs prep, int cutBlocks)
{
    __shared__ uint32_t sm[17];
    // blocks 0..GS_ITEM_PARTS-1: the item list; the next cutBlocks: the view's depth cuts, one tile per thread; the blocks
    // behind: the accumulator clear (hidden under the item scan).  The loss kernel carries the same three along when the loss
    // of a fused forward is taken through the library (ssim.hip); this launch is for hosts with their own loss.
    constexpr int IP = GS_ITEM_PARTS;
    if ((int)blockIdx.x >= IP + cutBlocks) {
        bwd_clear_part(prep, blockIdx.x - IP - cutBlocks, gridDim.x - IP - cutBlocks);
        return;
    }
    if ((int)blockIdx.x >= IP) {
        bwd_cut_renew(prep, (int)(blockIdx.x - IP) * 1024 + (int)threadIdx.x);
        return;
    }
    bwd_items_scan<SEG>(prep, sm, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// forward: one wavefront per 8x8 quadrant (h, k) of a 16x16 block, one pixel per lane, scalar f32.
//
// Three kernels serve it (launch_blend_forward_v2 picks one per forward): blend_fwd_v2q_kernel, one wave per quadrant (the
// default); blend_fwd_v2p_kernel, a staging wave beside every sweeping wave (deep lists); blend_fwd_v2w_kernel, four waves
// per quadrant (fewer quadrants than wave slots).  What they share exists once, in front of them: the argument struct, the
// pop of the next item, its decode, the staging (fwd_stage_compact), the per-entry arithmetic (fwd_pre / fwd_post /
// fwd_trips), the checkpoint allocator and store (ckpt_save) and the epilogue (fwd_finish).  The three differ in who does
// what when, not in what is computed: test_staging_wave_forward_leaves_the_same_bits holds the pair kernel to the one-wave
// kernel's bits.
//
// Checkpoints.  Every SEG list entries a quadrant that still has a live pixel saves its running state (T, R, G, B[, D])
// for the segment-parallel backward.  A slot is ALLOCATED when it is written (slots addressed by list position size the
// arena for every list being swept to its end: 1.97 GB at the bench reserve, of which 0.1 GB was ever touched): every
// persistent wave keeps a private pool of a few quadrant slots (one atomicAdd per CKPT_POOL_MAX boundaries, ckpt_pool), the
// slot's id goes to a small table indexed by (block's first segment + segment, quadrant) -- 16 B per 64 list entries --
// and the backward's item kernel puts the table row of every (block, segment) item into the item list.  Stale table
// entries are never read: the backward loads a quadrant's state only for pixels that were live at the boundary, and
// then this forward wrote the entry.  An arena that runs out raises the overflow word like a pair reserve that does
// (the render itself is complete; the step is gated, the host regrows: gs_ctx_reserve).
// ---------------------------------------------------------------------------------------------
// what a forward kernel is launched with: one struct by value, filled once by launch_blend_forward_v2
struct BlendFwdArgs {
    int W, H, tileW, tileH, gridW, blocksX, nItems;
    GsBackground bgc;
    const float4* rec12;
    const uint32_t* sortedIdx;
    uint32_t idxMask;
    const uint32_t *tileRanges, *segBase;
    uint32_t segCap;
    int statePlanes;                // 0: a render-only forward, no checkpoints
    float *outColor, *outDepth, *outAlpha;
    uint32_t* lastContrib;
    float* finalT;
    float* segState;
    uint32_t* segSlot;
    uint32_t qslotCap, qslotOwn, qslotShared0, qslotPart, ckptPool;      // the checkpoint arena (CkptPool, ckpt_save)
    uint32_t *blockWork, *counters, *fwdQueue;
    uint32_t nq;
    const uint32_t *blockOrder, *cutStore;
    uint32_t* hostWords;
    GsVirtGeom vg;
    unsigned long long* trace;      // blend_fwd_v2q_kernel only
    uint32_t slowSlot;              // blend_fwd_v2q_kernel only
    float foldScale;                // blend_fwd_v2w_kernel only
};

// Work distribution (round 4).  An item is one 8x8 quadrant of the pixel block at position p of the launch order
// (blockOrder, deepest first).  The four quadrant waves of a block gather the same records; workgroups go to the eight
// XCDs round-robin, each XCD with an L2 of its own, and rounds 1-3 gave the four items of a block to four consecutive
// waves = four XCDs: every record was fetched from the fabric four times (PMC: 3.9x the algorithmic bytes).  Now block
// position p belongs to XCD p mod 8: the taker (a wave of the one-wave kernel, a workgroup of the other two) with slot
// s on XCD x starts on quadrant s mod 4 of position 8 (s / 4) + x -- its static first item: thousands of simultaneous
// pops on one counter take ~6 ns each to resolve, 15 % of the kernel --, and the positions behind the statically assigned
// ones are handed out by EIGHT queues, one per XCD (four consecutive pops = one block), so the quadrants of a block meet in
// one L2 -- and the pops, which resolve at ~6 ns each on one address, spread over eight.  A taker whose XCD's queue has run
// dry takes from the others'.
// nq = 8 queues (default) / 1 (rounds 1-3's mapping: one queue; GS_TUNE_FWD_QUEUES, A/B)
// (workgroup g sits on XCD g mod nq)
struct FwdQueue {
    uint32_t xcd, slot;       // this taker's XCD and its slot there
    uint32_t nPos;            // positions of the launch order: the pixel blocks, padded to whole rows of nq (gs_bwd_prep.h, seg_base_body)
    uint32_t staticRows;      // rows of nq positions covered by the takers' first items
    uint32_t dead;            // queues found empty
};
__device__ __forceinline__ FwdQueue fwd_queue(const BlendFwdArgs& a, uint32_t slot, uint32_t takers)
{
    FwdQueue q;
    q.xcd = blockIdx.x % a.nq; q.slot = slot;
    q.nPos = a.nq * ((((uint32_t)a.nItems >> 2) + a.nq - 1u) / a.nq);
    q.staticRows = takers / (4u * a.nq);
    q.dead = 0;
    return q;
}
// the taker's next (position, quadrant), called by one whole wave: the static item first, then the queues (mayPop).  pos stays
// >= nPos when there is none: every queue is empty, and they only grow, so every taker gets there
__device__ __forceinline__ void fwd_pop(const BlendFwdArgs& a, FwdQueue& q, bool first, bool mayPop, int lane, uint32_t& pos, uint32_t& quad)
{
    pos = 0xFFFFFFFFu; quad = 0;
    if (first && (q.slot >> 2) < q.staticRows) { pos = a.nq * (q.slot >> 2) + q.xcd; quad = q.slot & 3u; }
    else if (mayPop)
        queue_pop(a.fwdQueue, a.nq, q.xcd, q.dead, lane, [&](uint32_t y, uint32_t k) {
            const uint32_t p = a.nq * (q.staticRows + (k >> 2)) + y;
            if (p < q.nPos) { pos = p; quad = k & 3u; }
            return p < q.nPos;
        });
}

// an item, decoded: the block, its quadrant, its list, this lane's pixel
struct FwdItem {
    int b, h, k, tile;
    uint32_t start, count, sbase;      // the tile's list, the block's first saved state (segBase)
    int X0, Y0, XL, YL;                // the block's pixel origin and limits (block lists: blocks are enumerated per tile)
    int x, y;
    bool in;                           // the lane's pixel lies in the image
    float px, py;
    float qx0, qx1, qy0, qy1;          // the quadrant's pixel-centre rectangle, for the lane-private reach test at staging time
};
// false: a position a short last stripe leaves over (an empty list, no pixel in the image)
__device__ __forceinline__ bool fwd_decode(const BlendFwdArgs& a, uint32_t pos, uint32_t quad, int lane, FwdItem& it)
{
    const uint32_t bRaw = __builtin_amdgcn_readfirstlane(table_word(a.blockOrder, pos));
    const bool valid = bRaw != 0xFFFFFFFFu;
    it.b = (int)bRaw;
    it.h = (int)((quad >> 1) & 1u); it.k = (int)(quad & 1u);
    it.start = 0; it.count = 0; it.sbase = 0;
    it.tile = 0; it.X0 = 0; it.Y0 = 0; it.XL = 0; it.YL = 0;
    if (valid) {
        const int by = it.b / a.blocksX, bx = it.b - by * a.blocksX;
        it.tile = ((by * BLK) / a.tileH) * a.gridW + (bx * BLK) / a.tileW;
        it.start = __builtin_amdgcn_readfirstlane(table_word(a.tileRanges, 2 * it.tile));
        const uint32_t end = __builtin_amdgcn_readfirstlane(table_word(a.tileRanges, 2 * it.tile + 1));
        it.count = end > it.start ? end - it.start : 0u;
        it.sbase = __builtin_amdgcn_readfirstlane(table_word(a.segBase, it.b));
        gs_block_pixels(a.vg, bx, by, a.W, a.H, it.X0, it.Y0, it.XL, it.YL);
    }
    it.x = it.X0 + it.k * 8 + (lane & 7); it.y = it.Y0 + it.h * 8 + (lane >> 3);
    it.in = valid && it.x < it.XL && it.y < it.YL;
    it.px = (float)it.x; it.py = (float)it.y;
    it.qx0 = (float)(it.X0 + it.k * 8); it.qx1 = it.qx0 + 7.0f; it.qy0 = (float)(it.Y0 + it.h * 8); it.qy1 = it.qy0 + 7.0f;
    return valid;
}

// Staging compacts the chunk: lane j holds list entry c0 + j and tests it against the whole quadrant -- the
// minimum of its quadratic form over the pixel rectangle (rect_min_q) -- and only entries that can reach a
// pixel are parked in LDS, each with its list position.  An entry whose weight is below 2^-29 everywhere
// moves no pixel's state by more than ~5e-8 (CULL_QMIN), so skipping it changes nothing but the work: no LDS
// broadcast (the CU's LDS port is what saturates first with one pixel per lane), no exponent, no exp.
// Returns the entries parked, a multiple of four.
__device__ __forceinline__ uint32_t fwd_stage_compact(f4* slot, const RecV& v, uint32_t c0, const FwdItem& it, int lane)
{
    const float qmin = rect_min_q(v.a.z, v.a.w, v.b.x, v.b.y, it.qx0 - v.a.x, it.qx1 - v.a.x, it.qy0 - v.a.y, it.qy1 - v.a.y);
    const bool keep = (c0 + lane < it.count) && !(qmin > CULL_QMIN);
    const unsigned long long m = __ballot(keep);
    const uint32_t pos = rank_below(m);
    if (keep) {
        slot[pos * 3] = v.a; slot[pos * 3 + 1] = v.b;
        slot[pos * 3 + 2] = (f4){v.c.x, v.c.y, v.c.z, __uint_as_float(c0 + (uint32_t)lane + 1u)};
    }
    // pad to a multiple of four with null splats (opacity 0: alpha = 0, state untouched) so that the loop runs
    // whole groups only; a pixel still live at a pad entry is live at the end of the chunk, hence its nContrib
    const uint32_t n = (uint32_t)__popcll(m), n4 = (n + 3u) & ~3u;
    if ((uint32_t)lane < n4 - n) {
        const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
        slot[(n + lane) * 3] = z; slot[(n + lane) * 3 + 1] = z;
        slot[(n + lane) * 3 + 2] = (f4){0.f, 0.f, 0.f, __uint_as_float(min(c0 + 64u, it.count))};
    }
    return n4;
}

// a lane's pixel while its list is swept.  Round 6: the colour (depth) sums are kept as BASE + CHUNK -- the entries of the
// current 64-position chunk accumulate from zero, and the chunk's sum is added to the base at the chunk's end (one rounding
// of the size of the total per chunk instead of one per entry).  The backward takes what the rest of a list still owes from
// the difference between the final image and a checkpoint (a base); deep in a list that difference is small against both,
// and its error was the forward's per-entry roundings at the size of the TOTAL.  Same instruction
// count per entry.  (The four-wave kernel keeps its base in LDS meanwhile, not here: trips_abs.)
struct FwdPixel {
    float T;
    float cr, cg, cb, dd;          // this chunk's sums
    float br, bgr, bb, bd;         // the sums of the chunks in front of it
    uint32_t nc;
};
__device__ __forceinline__ FwdPixel fwd_pixel(bool in)
{
    FwdPixel s;
    s.T = in ? 1.0f : 0.0f;        // pixels outside the image start dead and are never stored
    s.cr = s.cg = s.cb = s.dd = 0.f;
    s.br = s.bgr = s.bb = s.bd = 0.f;
    s.nc = 0;
    return s;
}
// the chunk behind us joins the base
template <bool DEPTH>
__device__ __forceinline__ void fwd_join_chunk(FwdPixel& s)
{
    s.br += s.cr; s.bgr += s.cg; s.bb += s.cb; s.cr = 0.f; s.cg = 0.f; s.cb = 0.f;
    if (DEPTH) { s.bd += s.dd; s.dd = 0.f; }
}

// what of a staged entry does not depend on the running state (the exponents and exps first, the short serial chain
// through T second: fwd_trips)
struct Pre {
    float aclamp, r, g, b, depth;
    uint32_t ncv;              // list position + 1 of the splat: nContrib of a pixel that is live when it arrives
};
__device__ __forceinline__ void fwd_pre(const f4* slot, uint32_t j, float px, float py, Pre& o)
{
    const Rec s = unpack(slot[j * 3], slot[j * 3 + 1], slot[j * 3 + 2]);
    const float dx = px - s.mx, dy = py - s.my;
    const float dxdy = dx * dy, dx2 = dx * dx, dy2 = dy * dy;
    const float q = ((dx2 * s.c00 + dy2 * s.c11) + dxdy * s.c01) + dxdy * s.c10;
#ifdef GS_FWD_LIBM_EXP   // experiment: the oracle's exp(-0.5 q) through the device math library instead of v_exp_f32
    o.aclamp = fminf(s.op * expf(-0.5f * q), 0.99f);
#else
    o.aclamp = fminf(gauss_alpha_raw(q, s.op), 0.99f);
#endif
    o.r = s.r; o.g = s.g; o.b = s.b; o.depth = s.depth;
    o.ncv = __float_as_uint(slot[j * 3 + 2].w);
}
template <bool DEPTH>
__device__ __forceinline__ void fwd_post(FwdPixel& s, const Pre& o)
{
    const bool a = s.T >= 1e-4f;
    s.nc = a ? o.ncv : s.nc;
    const float alpha = a ? o.aclamp : 0.0f;
    const float w = s.T * alpha;
#ifdef GS_FWD_UNFUSED   // experiment ("the 1e-4 bar"): the reference's two-rounding C + w c
    s.cr = s.cr + w * o.r; s.cg = s.cg + w * o.g; s.cb = s.cb + w * o.b; if (DEPTH) s.dd = s.dd + w * o.depth;
#else
    s.cr = fmaf(w, o.r, s.cr); s.cg = fmaf(w, o.g, s.cg); s.cb = fmaf(w, o.b, s.cb); if (DEPTH) s.dd = fmaf(w, o.depth, s.dd);
#endif
    s.T = s.T * (1.0f - alpha);
}
__device__ __forceinline__ bool fwd_any_live(float T) { return __any(T >= 1e-4f); }
// the n staged entries (a multiple of four) against the running state, four per trip, until the quadrant has no live pixel
// left (live = false); returns the entries gone through
template <bool DEPTH>
__device__ __forceinline__ uint32_t fwd_trips(const f4* slot, uint32_t n, float px, float py, FwdPixel& s, bool& live)
{
    live = true;
    uint32_t j = 0;
    for (; j < n; j += 4) {
        Pre p0, p1, p2, p3;
        fwd_pre(slot, j, px, py, p0); fwd_pre(slot, j + 1, px, py, p1); fwd_pre(slot, j + 2, px, py, p2); fwd_pre(slot, j + 3, px, py, p3);
        fwd_post<DEPTH>(s, p0); fwd_post<DEPTH>(s, p1); fwd_post<DEPTH>(s, p2); fwd_post<DEPTH>(s, p3);
        if (!fwd_any_live(s.T)) { live = false; break; }
    }
    return j;
}

// A wave's pool of checkpoint slots (wave-uniform): qslotOwn slots of the arena are its own from the start -- every
// wave reaches its first boundary at about the same time, and that many pops on one counter would take ~6 ns each
// to resolve (measured: blend forward 0.19 -> 0.30 ms with a shared counter only) -- and only a wave that uses them
// up draws ckptPool (up to 8) more at a time from the shared part behind them, which is split in eight with a counter each
// (workgroups go round-robin over the eight XCDs: a wave's counter lives in its own L2).  With ONE counter behind
// a static share of 12 slots the 100 k / 800x800 config, whose waves need ~20, lost 54 us of its 175 (blend forward).
struct CkptPool {
    uint32_t next, end;
    uint32_t part, partsEmpty;      // the wave's own eighth of the shared part; the eighths found empty
};
// wave: the dense id of this wave among those that own a pool.  The host sized the arena for their number (launch_blend_forward_v2:
// every wave of the one-wave kernel, the sweeping wave of a pair, all four waves of a four-wave workgroup): qslotOwn each, the
// shared part from qslotShared0 = their number x qslotOwn on -- one value, the host's, under all three kernels
__device__ __forceinline__ CkptPool ckpt_pool_of(const BlendFwdArgs& a, uint32_t wave)
{
    CkptPool p;
    p.next = wave * a.qslotOwn; p.end = p.next + a.qslotOwn;
    p.part = blockIdx.x & 7u; p.partsEmpty = 0;
    return p;
}
// the checkpoint in front of list entry i of the item: draws a slot and stores the state (sT .. sd: the state before splat i,
// absolute; called only while some pixel of the quadrant is live there)
template <int SEG, bool DEPTH>
__device__ __forceinline__ void ckpt_save(const BlendFwdArgs& a, CkptPool& pl, const FwdItem& it, int lane, uint32_t i,
                                          float sT, float sr, float sg, float sb, float sd)
{
    if (pl.next == pl.end) {
        // the wave's own eighth of the shared part first, then the others': since round 4 an XCD works on one stripe
        // of the image, and a deep stripe needs more slots than its eighth holds while a shallow one leaves its
        // own unused (grown bench scene: the arena "ran out" with most of it free).  A part found empty is not
        // asked again (every failed draw still advances its counter: gs_ctx_reserve sizes a regrow from their sum).
        pl.next = a.qslotCap;      // (all parts used up: positions beyond the arena, which the test below reports)
        for (uint32_t t = 0; t < 8u && pl.next == a.qslotCap; t++) {
            const uint32_t y = (pl.part + t) & 7u;
            if ((pl.partsEmpty >> y) & 1u) continue;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&a.counters[GS_CNT_QSLOTS + y], a.ckptPool);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base + a.ckptPool <= a.qslotPart) pl.next = a.qslotShared0 + y * a.qslotPart + base;
            else {      // (give the failed draw back: the counters' sum stays what was drawn + what was wanted and not had)
                pl.partsEmpty |= 1u << y;
                if (lane == 0) atomicSub(&a.counters[GS_CNT_QSLOTS + y], a.ckptPool);
            }
        }
        // nothing left anywhere: keep counting what would have been drawn (the size of the regrow)
        if (pl.next == a.qslotCap && pl.partsEmpty == 0xFFu && lane == 0) atomicAdd(&a.counters[GS_CNT_QSLOTS + pl.part], a.ckptPool);
        pl.end = pl.next + a.ckptPool;
    }
    const uint32_t phys = pl.next++;
    const uint32_t vslot = it.sbase + i / SEG - 1;
    if (phys < a.qslotCap && vslot < a.segCap) {
        if (lane == 0) a.segSlot[(size_t)vslot * 4 + (it.h * 2 + it.k)] = phys;
        // a pixel that has terminated is never read back (the backward loads state only where nContrib > i0)
        float* st = a.segState + (size_t)phys * (a.statePlanes * 64) + lane;
        if (sT >= 1e-4f) {
            st[0] = sT; st[64] = sr; st[128] = sg; st[192] = sb;
            if (DEPTH && a.statePlanes == 5) st[256] = sd;   // wave-uniform: the depth sum only when a depth cotangent may come
        }
    } else if (lane == 0) {
        // out of checkpoint slots: the image is still complete, but no backward can be taken from this forward
        a.counters[GS_CNT_OVERFLOW] = 1u;
        a.hostWords[4] = 2u;        // 2: "the checkpoint arena", 1: "the pair reserve" (binning.hip)
    }
}

// the end of an item, by the wave that holds its final state: the cut-miss flag, the pixel's five outputs, the block's sweep
// length.  The pixel is rebuilt from the lane here, so that a kernel need not keep it across its sweep (the four-wave kernel
// spilled its item-invariant values to scratch at five workgroups per CU).
template <bool DEPTH>
__device__ __forceinline__ void fwd_finish(const BlendFwdArgs& a, const FwdItem& it, int lane, float T, float r, float g, float b,
                                           float d, uint32_t nc)
{
    // depth cuts: live pixels at the end of a list that was cut short -- this forward has to be repeated without
    // cuts (pixels outside the image carry T = 0).  The flag word lives in host memory.
    if (a.cutStore && fwd_any_live(T) && lane == 0 && table_word(a.cutStore, it.tile) != 0u) a.hostWords[0] = 1u;
    const int x = it.X0 + it.k * 8 + (lane & 7), y = it.Y0 + it.h * 8 + (lane >> 3);
    const bool in = x < it.XL && y < it.YL;
    if (in) {
        const size_t pix = (size_t)y * a.W + x;
        float bg0, bg1, bg2;
        gs_bg_terms(a.bgc, T, bg0, bg1, bg2);
        a.outColor[3 * pix] = r + bg0; a.outColor[3 * pix + 1] = g + bg1; a.outColor[3 * pix + 2] = b + bg2;
        if (DEPTH) a.outDepth[pix] = d;
        a.outAlpha[pix] = 1.0f - T; a.lastContrib[pix] = nc; a.finalT[pix] = T;
    }
    uint32_t m = in ? nc : 0u;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if (lane == 0 && m) atomicMax(&a.blockWork[it.b], m);
}

// ---------------------------------------------------------------------------------------------
// the one-wave kernel (the default)
// ---------------------------------------------------------------------------------------------
// DEPTH = false: the caller takes no depth image (gs_render_forward with out_depth NULL): no depth sum in the sweep (one of
// its ~30 vector instructions per splat), none in the checkpoints, nothing stored.
template <int SEG, bool DEPTH>
__global__ __launch_bounds__(256) void blend_fwd_v2q_kernel(BlendFwdArgs a)
{
    static_assert(SEG % 64 == 0, "segment length must be a multiple of the 64-record chunk");
    // Round 6: the launch is workgroups of FOUR independent waves (no barrier between them, every wave its own LDS slots) instead
    // of one-wave workgroups.  The dispatcher spreads a workgroup's waves over the CU's four SIMDs, so every SIMD holds exactly
    // waves-per-SIMD of them; with 16 single-wave workgroups per CU it put five on some SIMDs and three on others (73 of 1024
    // each, tools/fwd_trace.py), and a fifth wave runs at a quarter of the first one's pace (below).  The four waves of a
    // workgroup take the four quadrants of one block as their first items -- the same records, now through one CU's L1.
    __shared__ f4 sgAll[4][2][192];      // per wave: two 64-record slots
    const int wvg = (int)(threadIdx.x >> 6);          // wave of the workgroup
    f4 (*sg)[192] = sgAll[wvg];
    // Round 6 (tools/fwd_trace.py, cycles per blended entry by HW_ID wave slot on c3: slot 0 282, slot 1 314, slot 2 402,
    // slot 3 582, the fifth wave of a SIMD that got five 994): the SIMD's issue arbiter favours its lower wave slots, a
    // wave's slot is fixed for its life, and the launch's last third was the waves of slot 3 finishing a SECOND item
    // (popped at ~60 % of the span, 130 k cycles at their pace) while the slots 0-2 had run out of work at 270 k of 346 k
    // cycles.  Three waves saturate a SIMD's issue (two do), so a wave in a slow slot takes its static first item and no
    // other: what it leaves in the queues the fast slots take, faster once it has gone.  Which wave blends which item
    // never changed a bit of the result (test_forward_queue_count_leaves_the_same_bits).
    const uint32_t hwSlot = (uint32_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (3 << 11));      // HW_ID[3:0]: wave slot in the SIMD
    const int lane = threadIdx.x & 63;
    const uint32_t nWaves = gridDim.x * 4u;                   // every wave takes items and owns a checkpoint pool
    const uint32_t dw = blockIdx.x * 4u + (uint32_t)wvg;      // dense wave id (checkpoint pools, trace)
    CkptPool pool = ckpt_pool_of(a, dw);
    // (wave w of workgroup g is slot 4 (g / nq) + w of its XCD: first item = quadrant w of position nq (g / nq) + g mod nq)
    FwdQueue qc = fwd_queue(a, (blockIdx.x / a.nq) * 4u + (uint32_t)wvg, nWaves);
    for (bool first = true;; first = false) {
        uint32_t pos, quad;
        fwd_pop(a, qc, first, hwSlot < a.slowSlot, lane, pos, quad);      // (a slow slot: no item beyond the static one)
        if (pos >= qc.nPos) {
            if (first) continue;          // (a wave beyond the static rows, or an image smaller than the grid: try the queues)
            break;
        }
        const uint32_t item = pos * 4u + quad;
        const unsigned long long tStart = a.trace ? clock64() : 0ull;
        uint32_t itersDone = 0, chunksDone = 0;
        FwdItem it;
        if (!fwd_decode(a, pos, quad, lane, it)) continue;
        FwdPixel s = fwd_pixel(it.in);
        const uint32_t* __restrict__ idx = a.sortedIdx + it.start;

        // The list runs through GS_FWD_PREFETCH register sets in turn: the set that holds chunk c's records is refilled, right after
        // they are staged, with the records of chunk c + D from indices loaded D chunks earlier, and then takes the indices of chunk
        // c + 2 D.  D = 1 (shipped): indices two chunks ahead, records one.  D = 2, 3 (round 6, tried because the last 15 % of the
        // launch's span move 1.4 % of its entries -- tools/fwd_trace.py -- as if every chunk waited for its gather): 114 / 128 VGPRs
        // against 105, blend forward on c3 0.179 / 0.181 ms against 0.178, c2 0.162 / 0.221 against 0.162 (EXPERIMENTS.md): the
        // tail is not the gather's latency.
        constexpr int D = GS_FWD_PREFETCH;
        RecV recs[D];
        uint32_t gis[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            recs[d] = load_chunk(a.rec12, idx, a.idxMask, 64u * d, it.count, lane);
            gis[d] = load_chunk_index(idx, a.idxMask, 64u * (D + d), it.count, lane);
        }
        auto chunk = [&](uint32_t c0, RecV& rec, uint32_t& gi) -> bool {      // false: the quadrant has no live pixel left
            f4* slot = sg[(c0 >> 6) & 1];
            const uint32_t n = fwd_stage_compact(slot, rec, c0, it, lane);
            if (c0 + 64u * D < it.count) {
                rec = gather_chunk(a.rec12, gi);
                gi = load_chunk_index(idx, a.idxMask, c0 + 128u * D, it.count, lane);
            }
            fwd_join_chunk<DEPTH>(s);
            if (a.statePlanes != 0 && c0 != 0 && (c0 % SEG) == 0) ckpt_save<SEG, DEPTH>(a, pool, it, lane, c0, s.T, s.br, s.bgr, s.bb, s.bd);
            bool live;
            itersDone += fwd_trips<DEPTH>(slot, n, it.px, it.py, s, live); chunksDone++;
            if (!live) return false;
            if (s.T >= 1e-4f) s.nc = min(c0 + 64u, it.count);      // still live: went through the whole chunk
            return fwd_any_live(s.T);
        };
        for (uint32_t c0 = 0; c0 < it.count; c0 += 64u * D) {
            bool go = true;
#pragma unroll
            for (int d = 0; d < D; d++)
                if (go && c0 + 64u * d < it.count) go = chunk(c0 + 64u * d, recs[d], gis[d]);
            if (!go) break;
        }
        if (a.trace && lane == 0 && item < (uint32_t)a.nItems) {
            a.trace[(size_t)item * 4 + 0] = tStart;
            a.trace[(size_t)item * 4 + 1] = clock64();
            a.trace[(size_t)item * 4 + 2] = (unsigned long long)itersDone | ((unsigned long long)chunksDone << 32);      // blended entries (with pads) | chunks
            // blockIdx.x | XCC_ID (4 bits) << 32 | HW_ID[15:0] (wave, SIMD, pipe, CU, SH, SE) << 36
            a.trace[(size_t)item * 4 + 3] = (unsigned long long)dw |
                                            ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32) |
                                            ((unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (15 << 11)) << 36);
        }
        fwd_finish<DEPTH>(a, it, lane, s.T, s.br + s.cr, s.bgr + s.cg, s.bb + s.cb, s.bd + s.dd, s.nc);
    }
}

// ---------------------------------------------------------------------------------------------
// forward with a STAGING WAVE beside every sweeping wave (round 6; GS_TUNE_FWD_PAIR).
//
// What paces a deep quadrant (EXPERIMENTS.md, "where the forward's 31 % go"): its list keeps one entry in six, so a 64-position
// chunk is ~11 blended entries (~360 vector instructions) behind ~275 instructions that do not depend on the running state at
// all -- the record gather's address arithmetic, the reach test, the ballot / compaction into LDS, the pad.  In the one-wave
// kernel both sit on ONE wave's in-order instruction stream, and the launch ends when the deepest such chain does (c3: one
// quadrant's ~3000 positions; no launch order shortens a single item).  Here a workgroup is two waves: wave 1 stages --
// chunk c + 1 goes through load, cull and compaction into the other LDS slot while wave 0 blends chunk c, exactly the
// one-wave kernel's arithmetic in exactly its order (same image, same nContrib, same checkpoints, bit for bit) --, and the
// two meet at one workgroup barrier per chunk.  The chain per chunk is max(staging, blending) instead of their sum; the
// instruction total is the same, on six waves per SIMD (three pairs) instead of four.
// ---------------------------------------------------------------------------------------------
// a workgroup barrier that makes the LDS writes in front of it visible behind it, usable from wave-uniform branches
#define V2P_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); \
                           __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
#ifndef GS_V2P_WAVES
#define GS_V2P_WAVES 6     // waves per SIMD the kernel is compiled for (the second __launch_bounds__ argument): <= 80 VGPRs
#endif
#define GS_V2P_WGS (2 * GS_V2P_WAVES)      // workgroups (pairs) per CU at that occupancy
template <int SEG, bool DEPTH>
__global__ __launch_bounds__(128, GS_V2P_WAVES) void blend_fwd_v2p_kernel(BlendFwdArgs a)
{
    static_assert(SEG % 64 == 0, "segment length must be a multiple of the 64-record chunk");
    __shared__ f4 sg[2][192];          // two 64-record slots: one being blended, one being staged
    __shared__ uint32_t sN[2];         // entries (padded to four) the staging wave left in each slot
    __shared__ uint32_t sItem[2];      // the workgroup's item: position of the launch order, quadrant
    __shared__ uint32_t sStop;         // set by the sweeping wave when the item is finished
    const int lane = threadIdx.x & 63;
    const bool stager = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;      // wave-uniform by construction
    CkptPool pool = ckpt_pool_of(a, blockIdx.x);                 // (the sweeping wave's: one wave per workgroup saves)
    FwdQueue qc = fwd_queue(a, blockIdx.x / a.nq, gridDim.x);    // (the sweeping wave's: the workgroup is the taker)
    for (bool first = true;; first = false) {
        if (!stager) {      // the item of the workgroup, popped by the sweeping wave
            uint32_t pos, quad;
            fwd_pop(a, qc, first, true, lane, pos, quad);
            if (lane == 0) { sItem[0] = pos; sItem[1] = quad; sStop = 0u; }
        }
        __syncthreads();
        const uint32_t pos = sItem[0], quad = sItem[1];
        if (pos >= qc.nPos) {
            __syncthreads();              // (sItem is written again by the next round's pop)
            if (first) continue;
            break;
        }
        // (a position a short last stripe leaves over goes through the item's barriers with an empty list and stores nothing)
        FwdItem it;
        const bool valid = fwd_decode(a, pos, quad, lane, it);
        const uint32_t* __restrict__ idx = a.sortedIdx + it.start;

        // The two roles run SEPARATE loops with the same number of barriers (a barrier counts arriving waves, not program
        // locations; `stager` is wave-uniform): in one shared loop the staging wave's prefetch registers and the sweeping wave's
        // pixel state were all loop-carried together (100 VGPRs: four waves per SIMD instead of six).
        if (stager) {
            // ---- the staging wave's half: load, reach test, compaction ----
            RecV nxt;
            nxt.a = nxt.b = nxt.c = (f4){0.f, 0.f, 0.f, 0.f};
            uint32_t gNext = 0xFFFFFFFFu;
            if (it.count > 0) {       // chunk 0 into slot 0 before the sweep starts; chunk 1's records and chunk 2's indices in flight
                gNext = load_chunk_index(idx, a.idxMask, 64, it.count, lane);
                nxt = load_chunk(a.rec12, idx, a.idxMask, 0, it.count, lane);
                const uint32_t n = fwd_stage_compact(sg[0], nxt, 0, it, lane);
                if (lane == 0) sN[0] = n;
                if (64 < it.count) {
                    nxt = gather_chunk(a.rec12, gNext);
                    gNext = load_chunk_index(idx, a.idxMask, 128, it.count, lane);
                }
            }
            V2P_BARRIER();                // slot 0 is staged (and sItem has been read by both waves)
            for (uint32_t c0 = 0; c0 < it.count; c0 += 64) {
                const uint32_t cur = (c0 >> 6) & 1u;
                if (c0 + 64 < it.count) { // the next chunk into the other slot while the sweeping wave blends this one
                    const uint32_t n = fwd_stage_compact(sg[cur ^ 1u], nxt, c0 + 64, it, lane);
                    if (lane == 0) sN[cur ^ 1u] = n;
                    if (c0 + 128 < it.count) {
                        nxt = gather_chunk(a.rec12, gNext);
                        gNext = load_chunk_index(idx, a.idxMask, c0 + 192, it.count, lane);
                    }
                }
                V2P_BARRIER();
                if (*(volatile uint32_t*)&sStop) break;          // (both waves read the same word behind the same barrier)
            }
            V2P_BARRIER();                // (sStop / sItem / the slots are written again by the next item)
            continue;
        }
        // ---- the sweeping wave's half: the running state and everything that depends on it ----
        FwdPixel s = fwd_pixel(it.in);
        V2P_BARRIER();                    // slot 0 is staged
        for (uint32_t c0 = 0; c0 < it.count; c0 += 64) {
            const uint32_t cur = (c0 >> 6) & 1u;
            const f4* sl = sg[cur];
            const uint32_t n = __builtin_amdgcn_readfirstlane(*(volatile uint32_t*)&sN[cur]);
            fwd_join_chunk<DEPTH>(s);
            if (a.statePlanes != 0 && c0 != 0 && (c0 % SEG) == 0) ckpt_save<SEG, DEPTH>(a, pool, it, lane, c0, s.T, s.br, s.bgr, s.bb, s.bd);
            bool live;
            fwd_trips<DEPTH>(sl, n, it.px, it.py, s, live);
            if (live) {
                if (s.T >= 1e-4f) s.nc = min(c0 + 64u, it.count);      // still live: went through the whole chunk
                live = fwd_any_live(s.T);
            }
            if (!live && lane == 0) sStop = 1u;
            V2P_BARRIER();
            if (*(volatile uint32_t*)&sStop) break;
        }
        V2P_BARRIER();                    // (sStop / sItem / the slots are written again by the next item)
        if (valid) fwd_finish<DEPTH>(a, it, lane, s.T, s.br + s.cr, s.bgr + s.cg, s.bb + s.cb, s.bd + s.dd, s.nc);
    }
}
#undef V2P_BARRIER

// ---------------------------------------------------------------------------------------------
// forward for launches with FEWER ITEMS THAN WAVE SLOTS (small images): four waves per quadrant, along the list.
//
// What the trace of the 10 k / 400x400 scene says (tools/fwd_trace.py, FWD_TRACE_CONFIG=c1_10k_400): a gfx950 wave issues a
// vector instruction every ~8 - 9 cycles at best -- one entry per ~280 cycles alone on its SIMD, 236 beside one other wave,
// and only from two waves on does the SIMD issue every ~4 cycles --, the 2500 quadrant items are two or three to a SIMD, and
// the kernel's 173 us are its deepest item's 1660 entries x 236 cycles while the chip-wide floor is 114.  More independent
// work INSIDE a wave does not help (two streams per wave: measured slower, EXPERIMENTS.md); more waves do.  Here a workgroup
// of four waves (one per SIMD of its CU) owns the quadrant.  The list goes by rounds of four 64-entry chunks, one per wave
// (which wave takes which turns with the round: a list's first chunk is the one every item has): part 0 from the
// quadrant's running state S (exact, the one-wave kernel's trips), parts 1-3 from T = 1, C = 0.  The end states meet in LDS and every wave folds
// them:  C += T_p C_w,  T *= T_w  for a pixel that is live from the part's first entry to its last (T only falls, so
// T_p T_w >= 1e-4 at the end says so); a pixel that is dead at the part's start keeps its state; a pixel that CROSSES 1e-4
// inside part w has sums that hold entries the reference does not blend -- wave w takes its (still staged) chunk again from
// the folded prefix, exactly as the one-wave kernel would have, and publishes that pixel's state; the fold then goes on
// behind part w from THAT state (round 5: a pixel on the threshold can come back live, the composed and the sequential
// product round differently; it is folded -- and re-swept, if it crosses again -- through the parts behind).  A part's
// checkpoint is its prefix, saved once the fold has settled it for every pixel.  The part boundaries depend on the list position only: hinted / unhinted / cut / uncut forwards of a view stay
// the same bits, and a list of at most 64 entries is swept by one wave with the one-wave kernel's arithmetic.
// ---------------------------------------------------------------------------------------------
// workgroups (= waves per SIMD) a CU holds: 102 VGPRs, 23 KB of LDS each.  10 k / 400x400 scene, blend forward: 0.137 ms with
// four, 0.130 with five (six does not launch); two staging slots per wave and 36 KB: four at most
#define GS_V2W_WGS 5
template <int SEG, bool DEPTH>
__global__ __launch_bounds__(256, GS_V2W_WGS) void blend_fwd_v2w_kernel(BlendFwdArgs a)
{
    static_assert(SEG == 64, "a part is one 64-entry chunk = one segment: its only checkpoint is its prefix");
    __shared__ f4 sgAll[4][192];               // per wave: one 64-record slot (DS operations of a wave complete in order)
    __shared__ float xEnd[4][5][64];           // end state of every part (wave 0: absolute, waves 1-3: relative)
    __shared__ float xDead[4][6][64];          // state (and nContrib) of the pixels that finished inside a part swept again
    __shared__ float xPre[4][4][64];           // per wave: the colour (depth) sums in front of its own part = its checkpoint
    __shared__ uint32_t sPop[2];
    const int lane = threadIdx.x & 63, hw = threadIdx.x >> 6;
    f4* sg = sgAll[hw];
    CkptPool pool = ckpt_pool_of(a, blockIdx.x * 4u + (uint32_t)hw);      // (every wave saves its own part's checkpoint)
    FwdQueue qc = fwd_queue(a, blockIdx.x / a.nq, gridDim.x);                             // (wave 0's: the workgroup is the taker)
    for (bool first = true;; first = false) {
        if (hw == 0) {      // the item of the workgroup, popped by wave 0
            uint32_t pos, quad;
            fwd_pop(a, qc, first, true, lane, pos, quad);
            if (lane == 0) { sPop[0] = pos; sPop[1] = quad; }
        }
        __syncthreads();
        const uint32_t pos = sPop[0], quad = sPop[1];
        __syncthreads();
        if (pos >= qc.nPos) {
            if (first) continue;
            break;
        }
        FwdItem it;
        if (!fwd_decode(a, pos, quad, lane, it)) continue;
        // the quadrant's running state S: the same bits in all four waves (cr .. dd: the whole sums, the base included)
        FwdPixel s = fwd_pixel(it.in);
        const uint32_t* __restrict__ idx = a.sortedIdx + it.start;
        // the staged chunk's entries against the running state, as the one-wave kernel takes them (liveness gate, nContrib)
        // (round 6, as there: the chunk's entries accumulate from zero and join the state the chunk started from at its end --
        // one rounding at the size of the total per chunk, not one per entry)
        // (the state the chunk starts from waits in LDS meanwhile -- `park`, four rows of 64 this wave owns at that moment --, not
        // in four registers across the loop: the kernel sits at its register budget for five workgroups per CU)
        auto trips_abs = [&](const f4* sl, uint32_t n, uint32_t c0, float* park) {
            park[lane] = s.cr; park[64 + lane] = s.cg; park[128 + lane] = s.cb; if (DEPTH) park[192 + lane] = s.dd;
            s.cr = 0.f; s.cg = 0.f; s.cb = 0.f; s.dd = 0.f;
            // (fwd_trips' entries in fwd_trips' order, with the exit folded into the loop's condition: through fwd_trips itself,
            // whose loop leaves by a break, this kernel's blend forward of the 10 k / 400x400 scene took 0.1274 ms against 0.1240,
            // with this form 0.1246 -- the inner loop then is the instructions it was, 101 + 18 + 4 vector and 23 scalar per trip)
            bool live = true;
            for (uint32_t j = 0; j < n && live; j += 4) {
                Pre p0, p1, p2, p3;
                fwd_pre(sl, j, it.px, it.py, p0); fwd_pre(sl, j + 1, it.px, it.py, p1); fwd_pre(sl, j + 2, it.px, it.py, p2); fwd_pre(sl, j + 3, it.px, it.py, p3);
                fwd_post<DEPTH>(s, p0); fwd_post<DEPTH>(s, p1); fwd_post<DEPTH>(s, p2); fwd_post<DEPTH>(s, p3);
                live = fwd_any_live(s.T);
            }
            if (live && s.T >= 1e-4f) s.nc = min(c0 + 64u, it.count);     // still live: went through the whole chunk
            s.cr = park[lane] + s.cr; s.cg = park[64 + lane] + s.cg; s.cb = park[128 + lane] + s.cb; if (DEPTH) s.dd = park[192 + lane] + s.dd;
        };

        // chunk of this wave in round r: c(r) = 256 r + 64 ((hw + r) & 3); records run one round ahead, indices two
        auto chunk_of = [&](uint32_t r) { return 256u * r + 64u * (((uint32_t)hw + r) & 3u); };
        RecV nx = load_chunk(a.rec12, idx, a.idxMask, chunk_of(0), it.count, lane);
        uint32_t gN = load_chunk_index(idx, a.idxMask, chunk_of(1), it.count, lane);
        for (uint32_t r = 0; 256u * r < it.count; r++) {
            if (!fwd_any_live(s.T)) break;                         // (S is the same in every wave: a uniform exit)
            const uint32_t s0 = 256u * r;
            const int w = (int)(((uint32_t)hw + r) & 3u);          // this wave's part of the round
            const uint32_t c0 = s0 + 64u * (uint32_t)w;
            const uint32_t nParts = min(4u, (it.count - s0 + 63u) / 64u);
            const bool mine = (uint32_t)w < nParts;
            f4* sl = sg;
            uint32_t n = 0;
            if (mine) n = fwd_stage_compact(sl, nx, c0, it, lane);
            nx = gather_chunk(a.rec12, gN);                        // (0xFFFFFFFF beyond the list: nothing is loaded)
            gN = load_chunk_index(idx, a.idxMask, chunk_of(r + 2), it.count, lane);
            // (parts 1-3 are swept from T = 1; the running state comes back from the fold, where part 0's end state is absolute)
            if (w == 0) {
                if (a.statePlanes != 0 && c0 != 0) ckpt_save<SEG, DEPTH>(a, pool, it, lane, c0, s.T, s.cr, s.cg, s.cb, s.dd);
                trips_abs(sl, n, c0, &xPre[hw][0][0]);          // (wave 0's xPre rows are written in the fold below, behind this)
            } else if (mine) {
                s.T = it.in ? 1.0f : 0.0f; s.cr = 0.f; s.cg = 0.f; s.cb = 0.f; s.dd = 0.f;
                for (uint32_t j = 0; j < n; j += 4) {              // (no liveness gate: the sums are used only where every entry was live)
                    Pre p0, p1, p2, p3;
                    fwd_pre(sl, j, it.px, it.py, p0); fwd_pre(sl, j + 1, it.px, it.py, p1); fwd_pre(sl, j + 2, it.px, it.py, p2); fwd_pre(sl, j + 3, it.px, it.py, p3);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const Pre& o = u == 0 ? p0 : u == 1 ? p1 : u == 2 ? p2 : p3;
                        const float wgt = s.T * o.aclamp;
                        s.cr = fmaf(wgt, o.r, s.cr); s.cg = fmaf(wgt, o.g, s.cg); s.cb = fmaf(wgt, o.b, s.cb); if (DEPTH) s.dd = fmaf(wgt, o.depth, s.dd);
                        s.T = s.T * (1.0f - o.aclamp);
                    }
                }
            }
            if (mine) { xEnd[w][0][lane] = s.T; xEnd[w][1][lane] = s.cr; xEnd[w][2][lane] = s.cg; xEnd[w][3][lane] = s.cb; xEnd[w][4][lane] = s.dd; }
            if (w == 0) xDead[0][5][lane] = __uint_as_float(s.nc);   // (nContrib after part 0)
            __syncthreads();
            // Fold, for this lane's pixel: P = the absolute state behind the parts [0, qDone) of the round.  A part q the pixel
            // is live through (T only falls: P.T x its end T >= 1e-4 says so) is composed onto P; a pixel dead at the part's
            // start keeps its state; a pixel that CROSSES 1e-4 inside part q (crossedIn = q) stops folding there, wave q takes
            // its chunk again from P with the one-wave kernel's gate and publishes that pixel's state, and the fold goes on
            // behind part q FROM THAT STATE.  The composed product and the sequential one round differently: a pixel within
            // ~1e-6 of the threshold can come back from its second take still live (round 4 read it as finished for the
            // round's later parts while the next round blended on: entries skipped, checkpoint lanes the backward reads
            // never written -- the advisor's finding).  So the fold is a loop: such a pixel (`again`) is folded through the
            // parts behind from its re-swept state, crossing and being re-swept again if need be; every other pixel's fold
            // is done in the first pass, and the loop's last vote is the barrier the round needed anyway.
            float PT = xEnd[0][0][lane], Pr = xEnd[0][1][lane], Pg = xEnd[0][2][lane], Pb = xEnd[0][3][lane], Pd = xEnd[0][4][lane];
            uint32_t Pnc = __float_as_uint(xDead[0][5][lane]);
            // prefix of this wave's own part (its checkpoint): known once the fold has passed the parts in front of it; a
            // pixel that never gets there live is not stored (T = 0)
            // (parked in LDS, not in five registers across the loop: the kernel sits at its register budget for five
            // workgroups per CU, and the loop's live state put 8 - 11 VGPRs into scratch)
            float myPT = 0.0f;
            uint32_t qDone = 1;
            for (;;) {
                int crossedIn = 0;
#pragma unroll
                for (int q = 1; q < 4; q++) {
                    if ((uint32_t)q >= qDone && (uint32_t)q < nParts && !crossedIn) {
                        if (q == w) { myPT = PT; xPre[hw][0][lane] = Pr; xPre[hw][1][lane] = Pg; xPre[hw][2][lane] = Pb; if (DEPTH) xPre[hw][3][lane] = Pd; }
                        if (PT >= 1e-4f) {
                            const float Tend = PT * xEnd[q][0][lane];
                            if (Tend * a.foldScale >= 1e-4f) {     // (foldScale: 1 exactly, but for the tests' forced second takes)
                                Pr = fmaf(PT, xEnd[q][1][lane], Pr); Pg = fmaf(PT, xEnd[q][2][lane], Pg); Pb = fmaf(PT, xEnd[q][3][lane], Pb);
                                if (DEPTH) Pd = fmaf(PT, xEnd[q][4][lane], Pd);
                                PT = Tend;
                                Pnc = min(s0 + 64u * (uint32_t)(q + 1), it.count);
                            } else crossedIn = q;
                        }
                        if (!crossedIn) qDone = (uint32_t)q + 1u;
                    }
                }
                if (!__syncthreads_or(crossedIn != 0)) break;
                if (w != 0 && mine && __any(crossedIn == w)) {
                    // pixels finish inside this part: its entries again, in sequence from the folded prefix (the chunk is
                    // still staged); the other lanes idle with T = 0
                    s.T = crossedIn == w ? PT : 0.0f; s.cr = Pr; s.cg = Pg; s.cb = Pb; s.dd = Pd; s.nc = 0;
                    trips_abs(sl, n, c0, &xDead[w][1][0]);          // (this part's xDead rows are written right below, by this wave)
                    if (crossedIn == w) {
                        xDead[w][0][lane] = s.T; xDead[w][1][lane] = s.cr; xDead[w][2][lane] = s.cg; xDead[w][3][lane] = s.cb; xDead[w][4][lane] = s.dd;
                        xDead[w][5][lane] = __uint_as_float(s.nc);
                    }
                }
                __syncthreads();
                bool again = false;
                if (crossedIn) {
                    PT = xDead[crossedIn][0][lane]; Pr = xDead[crossedIn][1][lane]; Pg = xDead[crossedIn][2][lane];
                    Pb = xDead[crossedIn][3][lane]; Pd = xDead[crossedIn][4][lane]; Pnc = __float_as_uint(xDead[crossedIn][5][lane]);
                    qDone = (uint32_t)crossedIn + 1u;
                    again = PT >= 1e-4f && qDone < nParts;         // came back live with parts still in front of it
                    if (!again) qDone = 4u;                        // finished (or nothing left): later parts leave it alone
                }
                if (!__syncthreads_or(again)) break;               // (also: xDead / xEnd are written again in the next round)
            }
            // the part's checkpoint, now that every pixel's prefix of it is final (the one-wave kernel saves one iff some
            // pixel reaches the chunk live)
            if (a.statePlanes != 0 && w != 0 && mine && __any(myPT >= 1e-4f))
                ckpt_save<SEG, DEPTH>(a, pool, it, lane, c0, myPT, xPre[hw][0][lane], xPre[hw][1][lane], xPre[hw][2][lane], DEPTH ? xPre[hw][3][lane] : 0.0f);
            s.T = PT; s.cr = Pr; s.cg = Pg; s.cb = Pb; s.dd = Pd; s.nc = Pnc;
        }
        if (hw == 0) fwd_finish<DEPTH>(a, it, lane, s.T, s.cr, s.cg, s.cb, s.dd, s.nc);
    }
}

// ---------------------------------------------------------------------------------------------
// backward: persistent single-wave workgroups, one (block, segment) item at a time.  The kernel is a short loop over the
// pieces in front of it, in the order it uses them: the argument struct, the pop of the next item, its decode, the per-pixel
// state load, the staging, the per-entry step (pair_exponent_bwd / pair_bwd / the transposed wave sum of gs_wavesum.h) and
// the flush.
// ---------------------------------------------------------------------------------------------
// what the kernel is launched with: one struct by value, filled once by launch_blend_backward_v2
struct BlendBwdArgs {
    int W, H, tileW, tileH, gridW, blocksX;
    GsBackground bgc;                                       // the background the forward composited over
    const float4* rec12;
    const uint32_t* sortedIdx;
    uint32_t idxMask;
    const uint32_t *tileRanges, *blockWork;                 // per tile: its list; per block: how far the forward swept it
    const uint32_t *itemBlock, *itemRow, *counters;         // the item list and its length (bwd_items_scan, counters[GS_CNT_ITEMS])
    const uint32_t* segSlot;                                // [rows][4]: per item row, the four quadrants' checkpoint slots
    const float* segState;                                  // the checkpoint arena, statePlanes x 64 floats per slot
    uint32_t qslotCap;
    int statePlanes;
    uint32_t *bwdQueue, nq;
    const float *cotColor, *cotDepth, *cotAlpha;            // the cotangents (cotDepth: DEPTH kernels only; cotAlpha may be null)
    const float *outColor, *outDepth, *outAlpha, *finalT;   // the forward's images
    const uint32_t* lastContrib;
    float* gradAcc16;                                       // [N][16], cleared by the item kernel: the one thing written
    GsVirtGeom vg;
};

// Work distribution, as in the forward: nq queues, one per XCD.  The item list is in block order, a block's segments next
// to each other; queue x hands out the x-th nq-th of it (by item count), i.e. a horizontal stripe of the image with about
// the same work as the others.  All the segments of a block -- which re-read the block's per-pixel cotangents and state,
// 9 KB per item -- and the blocks next to it -- which share most of their records -- then run on one XCD and find those
// bytes in its L2.  A wave whose own stripe is done takes from the others'.
struct BwdQueue {
    uint32_t xcd, slot;                   // this wave's XCD and its slot there
    uint32_t nItems, perQ, staticPerQ;    // the list's length, a stripe's, and how much of each stripe the waves' first items cover
    uint32_t dead;                        // queues found empty
};
__device__ __forceinline__ BwdQueue bwd_queue(const BlendBwdArgs& a)
{
    BwdQueue q;
    q.nItems = __builtin_amdgcn_readfirstlane(table_word(a.counters, GS_CNT_ITEMS));
    q.xcd = blockIdx.x % a.nq; q.slot = blockIdx.x / a.nq;
    q.perQ = (q.nItems + a.nq - 1u) / a.nq;
    q.staticPerQ = min(gridDim.x / a.nq, q.perQ);
    q.dead = 0;
    return q;
}
// the wave's next item: its static one first, then the queues.  >= nItems: none -- every queue is empty, and since they only
// grow every wave gets there; for a first item: the wave lies beyond the static share or its stripe is short, and asks again
__device__ __forceinline__ uint32_t bwd_pop(const BlendBwdArgs& a, BwdQueue& q, bool first, int lane)
{
    uint32_t item = 0xFFFFFFFFu;
    if (first && q.slot < q.staticPerQ) item = q.xcd * q.perQ + q.slot;
    else
        queue_pop(a.bwdQueue, a.nq, q.xcd, q.dead, lane, [&](uint32_t y, uint32_t k) {
            const uint32_t idx = q.staticPerQ + k;
            const bool has = idx < q.perQ && y * q.perQ + idx < q.nItems;
            if (has) item = y * q.perQ + idx;
            return has;
        });
    return item;
}

// an item, decoded
struct BwdItem {
    uint32_t seg, start;               // the segment; the first entry of the tile's list
    uint32_t i0, i1;                   // the segment's list positions, cut at the forward's sweep length
    uint32_t qslot[4];                 // the four quadrants' checkpoint slots in front of the segment (unused for segment 0)
    int X0, Y0, XL, YL;                // the block's pixel origin and limits (block lists: blocks are enumerated per tile)
};
template <int SEG>
__device__ __forceinline__ BwdItem bwd_decode(const BlendBwdArgs& a, uint32_t item)
{
    BwdItem it;
    const uint32_t packed = __builtin_amdgcn_readfirstlane(table_word(a.itemBlock, item));
    const uint32_t row = __builtin_amdgcn_readfirstlane(table_word(a.itemRow, item));
    const int b = (int)(packed >> 10);
    it.seg = packed & 1023u;
    const int by = b / a.blocksX, bx = b - by * a.blocksX;
    const int tile = ((by * BLK) / a.tileH) * a.gridW + (bx * BLK) / a.tileW;
    it.start = __builtin_amdgcn_readfirstlane(table_word(a.tileRanges, 2 * tile));
    const uint32_t work = __builtin_amdgcn_readfirstlane(table_word(a.blockWork, b));
    it.i0 = it.seg * SEG; it.i1 = min(it.i0 + SEG, work);
    it.qslot[0] = it.qslot[1] = it.qslot[2] = it.qslot[3] = 0;
    if (it.seg != 0)
#pragma unroll
        for (int k = 0; k < 4; k++) it.qslot[k] = __builtin_amdgcn_readfirstlane(table_word(a.segSlot, 4 * row + k));
    gs_block_pixels(a.vg, bx, by, a.W, a.H, it.X0, it.Y0, it.XL, it.YL);
    return it;
}

// packed-f32 helpers.  The f32 VALU of gfx950 retires one wave64 instruction per 4 cycles per SIMD (measured:
// both blend kernels ran at >90 % of that issue rate while "using" 25 % of the 157 TFLOP/s headline, which
// counts v_pk_fma_f32).  Each lane of the backward therefore owns pixel PAIRS (x, x+8) on one image row and does the pair's
// arithmetic with v_pk_mul/add/fma_f32; the row term dy is shared by the pair and stays scalar per lane.
__device__ __forceinline__ f2 splat2(float v) { return (f2){v, v}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// per-pixel-pair state of the backward sweep.  With T the running transmittance, R_i = sum_{j<=i} T_j a_j S_j
// (S_j = cot . sample_j), K = cot . final (colour, depth) + T_n cT_n and sc the reference's T-anchor scale
// (T' = 1 - outAlpha = sc T_n), the sweep carries the three products it actually uses:
//   Ts = sc T,   Q = sc (K - R)   (what the rest of the list and the background still owe, times sc).
struct PairState {
    f2 px, Ts, Q;
    f2 cCx, cCy, cCz, cD;                // cotangents of colour / depth
    float py;
    uint32_t nc0, nc1;
};
// The lane's two pixel pairs, (x, x + 8) on rows y and y + 8 of the block, at the segment's start, from the image planes and
// the checkpoint in front of the segment.  A pixel outside the image, or one the forward had finished before the segment
// (nContrib <= i0), stays at nContrib 0 and takes no part.  hm: the sweep length of each 16x8 half (max nContrib over its
// pixels): past it the half is dead, like one out of reach.
template <bool DEPTH>
__device__ __forceinline__ void bwd_load_pixels(const BlendBwdArgs& a, const BwdItem& it, int lane, PairState (&ps)[2], uint32_t (&hm)[2])
{
#pragma unroll
    for (int h = 0; h < 2; h++) {
        PairState& p = ps[h];
        const int y = it.Y0 + h * 8 + (lane >> 3);
        p.py = (float)y;
        p.Ts = p.Q = p.cCx = p.cCy = p.cCz = p.cD = splat2(0.f);
        uint32_t ncs[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int x = it.X0 + k * 8 + (lane & 7);
            p.px[k] = (float)x;
            if (x < it.XL && y < it.YL) {
                const size_t pix = (size_t)y * a.W + x;
                const uint32_t n = a.lastContrib[pix];
                if (n > it.i0) {
                    ncs[k] = n;
                    const float gx = a.cotColor[3 * pix], gy = a.cotColor[3 * pix + 1], gz = a.cotColor[3 * pix + 2];
                    const float gd = DEPTH ? a.cotDepth[pix] : 0.0f;
                    p.cCx[k] = gx; p.cCy[k] = gy; p.cCz[k] = gz; p.cD[k] = gd;
                    const float cA = a.cotAlpha ? a.cotAlpha[pix] : 0.0f;
                    const float Tn = a.finalT[pix];
                    float bg0, bg1, bg2;      // T_n b_c: the products the forward added (gs_bg_terms)
                    gs_bg_terms(a.bgc, Tn, bg0, bg1, bg2);
                    const float cTn = -cA + gs_bg_cot(a.bgc, gx, gy, gz);
                    // What the rest of the list still owes: cot . (final sums - the sums in front of the segment).  The
                    // DIFFERENCE per channel first, then the dot product -- deep in a list both are of the size of the total
                    // and their difference small, and cot . final - cot . checkpoint would carry two dot products' roundings at
                    // the size of the total; the forward keeps its sums so that the difference itself is good (FwdPixel)
                    const float sc = (1.0f - a.outAlpha[pix]) / Tn;     // the reference's T = 1 - outAlpha anchor
                    float T0 = 1.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;      // state in front of the segment
                    const uint32_t phys = it.qslot[h * 2 + k];
                    if (it.seg != 0 && phys < a.qslotCap) {
                        const float* st = a.segState + (size_t)phys * (a.statePlanes * 64) + lane;
                        T0 = st[0]; s0 = st[64]; s1 = st[128]; s2 = st[192];
                        if (DEPTH) s3 = st[256];
                    }
                    const float d0 = (a.outColor[3 * pix] - bg0) - s0, d1 = (a.outColor[3 * pix + 1] - bg1) - s1, d2 = (a.outColor[3 * pix + 2] - bg2) - s2;
                    const float owedC = fmaf(gx, d0, fmaf(gy, d1, fmaf(gz, d2, DEPTH ? gd * (a.outDepth[pix] - s3) : 0.0f)));
                    p.Ts[k] = sc * T0;
                    p.Q[k] = sc * (owedC + Tn * cTn);
                }
            }
        }
        p.nc0 = ncs[0]; p.nc1 = ncs[1];
        hm[h] = max(ncs[0], ncs[1]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        hm[0] = max(hm[0], (uint32_t)__shfl_xor((int)hm[0], d, 64));
        hm[1] = max(hm[1], (uint32_t)__shfl_xor((int)hm[1], d, 64));
    }
}

// A list entry as the backward keeps it in LDS: the conic pre-multiplied by C = -1/(2 ln 2), so that the exponent of
// 2^e comes out of two fused multiply-adds, e = dx^2 A + dxdy B + dy^2 Dq (A = c00 C, B = (c01 + c10) C, Dq = c11 C).
// The FORWARD has to evaluate the quadratic form in the reference's operation order to stay within 1e-4 of it
// (fwd_pre, gauss_alpha_raw); the backward only needs alpha to ~1e-6 (gradients are held to 1e-3), and this
// form is four instructions per 16x8 half and splat shorter.
struct RecB {
    float mx, my, A, B, Dq, r, g, b, op, depth;
};
constexpr float EXP_INV_C1 = -1.3862943611198906f;     // 1 / C = -2 ln 2: gives the conic back at the flush
// Staging compacts the 64-entry chunk at c0, as in the forward: lane j tests list entry c0 + j against the two 16x8 halves
// of the block (rect_min_q) and parks it only if it can reach one of them, as a RecB (mx, my, A, B | Dq, -, r, g | b, op,
// depth, tag) tagged with its position in the segment and the halves it does NOT reach (256, 512).  Entries out of reach cost
// nothing afterwards.  Returns the entries parked.
__device__ __forceinline__ uint32_t bwd_stage(const BlendBwdArgs& a, const BwdItem& it, const uint32_t (&hm)[2],
                                              const uint32_t* __restrict__ idx, uint32_t c0, int lane, f4* sg)
{
    const float bx0 = (float)it.X0, bx1 = bx0 + 15.0f, by0 = (float)it.Y0;
    const RecV v = load_chunk(a.rec12, idx, a.idxMask, c0, it.i1, lane);
    const float X0 = bx0 - v.a.x, X1 = bx1 - v.a.x, Yt = by0 - v.a.y;
    const uint32_t li = c0 + (uint32_t)lane;
    const bool far0 = li >= hm[0] || rect_min_q(v.a.z, v.a.w, v.b.x, v.b.y, X0, X1, Yt, Yt + 7.0f) > CULL_QMIN;
    const bool far1 = li >= hm[1] || rect_min_q(v.a.z, v.a.w, v.b.x, v.b.y, X0, X1, Yt + 8.0f, Yt + 15.0f) > CULL_QMIN;
    const bool keep = (c0 + lane < it.i1) && !(far0 && far1);
    const unsigned long long m = __ballot(keep);
    const uint32_t pos = rank_below(m);
    if (keep) {
        const uint32_t tag = (c0 - it.i0 + (uint32_t)lane) | (far0 ? 256u : 0u) | (far1 ? 512u : 0u);
        sg[pos * 3] = (f4){v.a.x, v.a.y, v.a.z * EXP_C1, (v.a.w + v.b.x) * EXP_C1};
        sg[pos * 3 + 1] = (f4){v.b.y * EXP_C1, 0.0f, v.b.z, v.b.w};
        sg[pos * 3 + 2] = (f4){v.c.x, v.c.y, v.c.z, __uint_as_float(tag)};
    }
    return (uint32_t)__popcll(m);
}

struct PairB {
    f2 dx, dxdy, dx2, e2;
    float dy, dy2;
};
__device__ __forceinline__ void pair_exponent_bwd(const RecB& s, f2 px, float py, PairB& o)
{
    o.dx = px - splat2(s.mx);
    o.dy = py - s.my;
    o.dxdy = o.dx * splat2(o.dy);
    o.dx2 = o.dx * o.dx;
    o.dy2 = o.dy * o.dy;
    o.e2 = fma2(o.dxdy, splat2(s.B), fma2(o.dx2, splat2(s.A), splat2(o.dy2 * s.Dq)));
}

// One splat against one pixel pair; adds the pair's contributions to the packed accumulators
//   acc: 0 sum h dx   1 sum h dy   2 sum h dx^2   3 sum h dxdy   4 sum h dy^2   5 dop   6 dr   7 dg   8 db   9 ddepth
// with h = dL/d(alpha) raw gated = -2 x (-1/2 dL/d(exponent)): the factor -1/2, the conic factors of the mean gradient
// (linear in the first two sums) and the sign are applied once per splat at the flush, not once per pixel.
// The cotangent of T_{i+1} is what the rest of the list and the background still owe,
//   c_i = (K - R_i) / T_{i+1},   since  cot . (C_final - C_i) = sum_{j>i} T_j a_j S_j,
// so   dL/d(alpha_i) = sc T_i (S_i - c_i) = Ts_i S_i - Q_i / (1 - alpha_i),   Q_i = Q_{i-1} - sc T_i a_i S_i:
// the sweep needs neither T nor R themselves, and one reciprocal of 1 - alpha (>= 0.01) per pixel.
// ABSGRAD (gs_set_absgrad): two more sums, of the ABSOLUTE per-pixel terms of the mean gradient,
//   10 sum |h u|   11 sum |h v|,   u = A dx + (B/2) dy,  v = Dq dy + (B/2) dx   (the conic as the record holds it, times C;
// 1/|C| at the flush).  |h u| = |h| |u|: both abs are source modifiers of one v_fma_f32 per pixel, which the packed forms
// do not have -- ten scalar VALU per pixel pair and call (two products, four fma for u and v, four for the sums), B/2 once.
template <bool DEPTH, bool ABSGRAD, int NACC>
__device__ __forceinline__ void pair_bwd(const RecB& s, uint32_t i, const PairB& e, PairState& p, f2 (&acc)[NACC])
{
    static_assert(NACC == (ABSGRAD ? 12 : 10), "ten sums, twelve with the absolute ones");
    const f2 G = (f2){__builtin_amdgcn_exp2f(e.e2.x), __builtin_amdgcn_exp2f(e.e2.y)};
    const f2 raw = splat2(s.op) * G;
    const bool a0 = i < p.nc0, a1 = i < p.nc1;
    f2 alpha;
    alpha.x = a0 ? fminf(raw.x, 0.99f) : 0.0f;
    alpha.y = a1 ? fminf(raw.y, 0.99f) : 0.0f;
    const f2 contrib = p.Ts * alpha;
    // without a depth cotangent cD = 0: the product is +-0 and fma(cCz, b, +-0) is the rounded product itself
    const f2 S = fma2(p.cCx, splat2(s.r), fma2(p.cCy, splat2(s.g),
                      DEPTH ? fma2(p.cCz, splat2(s.b), p.cD * splat2(s.depth)) : p.cCz * splat2(s.b)));
    p.Q = fma2(-contrib, S, p.Q);
    const f2 oma = splat2(1.0f) - alpha;
    const f2 owed = p.Q * (f2){__builtin_amdgcn_rcpf(oma.x), __builtin_amdgcn_rcpf(oma.y)};
    const f2 dAlpha = fma2(p.Ts, S, -owed);
    f2 gate;
    gate.x = (a0 && !(raw.x > 0.99f)) ? dAlpha.x : 0.0f;
    gate.y = (a1 && !(raw.y > 0.99f)) ? dAlpha.y : 0.0f;
    const f2 hh = gate * raw;
    acc[0] = fma2(hh, e.dx, acc[0]);
    acc[1] = fma2(hh, splat2(e.dy), acc[1]);
    acc[2] = fma2(e.dx2, hh, acc[2]);
    acc[3] = fma2(e.dxdy, hh, acc[3]);
    acc[4] = fma2(splat2(e.dy2), hh, acc[4]);
    acc[5] = fma2(G, gate, acc[5]);
    acc[6] = fma2(contrib, p.cCx, acc[6]);
    acc[7] = fma2(contrib, p.cCy, acc[7]);
    acc[8] = fma2(contrib, p.cCz, acc[8]);
    if (DEPTH) acc[9] = fma2(contrib, p.cD, acc[9]);
    if constexpr (ABSGRAD) {
        const float hB = 0.5f * s.B;
        const float tx = hB * e.dy, ty = s.Dq * e.dy;
        const float u0 = fmaf(e.dx.x, s.A, tx), u1 = fmaf(e.dx.y, s.A, tx);
        const float v0 = fmaf(e.dx.x, hB, ty), v1 = fmaf(e.dx.y, hB, ty);
        acc[10].x = fmaf(fabsf(hh.x), fabsf(u0), acc[10].x);
        acc[10].y = fmaf(fabsf(hh.y), fabsf(u1), acc[10].y);
        acc[11].x = fmaf(fabsf(hh.x), fabsf(v0), acc[11].x);
        acc[11].y = fmaf(fabsf(hh.y), fabsf(v1), acc[11].y);
    }
    p.Ts = p.Ts * oma;
}

// One parked entry against the block: the two halves it reaches, the transposed wave sum of the 10 (12) per-lane sums, and
// the park of the result in the entry's row of `part` -- a PartRow (gs_wavesum.h): every fourth lane holds one slot, and
// three slots the reduction leaves idle take the conic terms the flush needs for the mean gradient.
template <bool DEPTH, bool ABSGRAD>
__device__ __forceinline__ void bwd_entry(const f4* sg, uint32_t jl, uint32_t i0, PairState (&ps)[2], int lane, float (*part)[16])
{
    const f4 ra = sg[jl * 3], rb = sg[jl * 3 + 1], rc = sg[jl * 3 + 2];
    const uint32_t tag = __builtin_amdgcn_readfirstlane(__float_as_uint(rc.w));
    const uint32_t i = i0 + (tag & 255u);
    const RecB s = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.z, rb.w, rc.x, rc.y, rc.z};
    PairB e0, e1;
    const bool k0 = (tag & 256u) != 0, k1 = (tag & 512u) != 0;     // wave-uniform: half out of reach
    if (!k0) pair_exponent_bwd(s, ps[0].px, ps[0].py, e0);
    if (!k1) pair_exponent_bwd(s, ps[1].px, ps[1].py, e1);
    constexpr int NACC = ABSGRAD ? 12 : 10;
    f2 acc2[NACC];
#pragma unroll
    for (int q = 0; q < NACC; q++) acc2[q] = splat2(0.0f);
    if (!k0) pair_bwd<DEPTH, ABSGRAD, NACC>(s, i, e0, ps[0], acc2);
    if (!k1) pair_bwd<DEPTH, ABSGRAD, NACC>(s, i, e1, ps[1], acc2);
    float acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; q++) acc[q] = acc2[q].x + acc2[q].y;
    float w;
    if constexpr (ABSGRAD) w = wave_sum12_transposed<!DEPTH>(acc);
    else w = wave_sum10_transposed<!DEPTH>(acc);
    if (lane == PartRow::lane(PartRow::c00)) w = s.A * EXP_INV_C1;
    if (lane == PartRow::lane(PartRow::c11)) w = s.Dq * EXP_INV_C1;
    if (lane == PartRow::lane(PartRow::c01c10)) w = s.B * EXP_INV_C1;
    if ((lane & 3) == 0) part[i - i0][lane >> 2] = w;
}

// The segment's n rows of `part` into gradAcc16, in the reference's packed column order (dmx dmy dc00 dc01 dc10 dc11 dr dg
// db dop ddepth; PartRow says which slot a column reads).  The factor -1/2 of the exponent's derivative, the conic factors
// of the mean gradient and the sign are applied here, once per splat.  Without a depth cotangent the depth column is not
// written; ABSGRAD: the two absolute sums, times 1/|C|, go to columns 12 and 13 of the row (Ax, Ay in pixel units; column 11
// is left alone, the item kernel clears whole rows, no kernel of the backward reads the row's fourth quarter).
template <bool DEPTH, bool ABSGRAD>
__device__ __forceinline__ void bwd_flush(const BlendBwdArgs& a, const uint32_t* __restrict__ idx, uint32_t n, int lane,
                                          const float (*part)[16])
{
    constexpr uint32_t NCOL = ABSGRAD ? 13u : 11u;
    constexpr int A1 = PartRow::sumSlot[0], A2 = PartRow::sumSlot[1];
    for (uint32_t e = lane; e < n * NCOL; e += 64) {
        const uint32_t j = e / NCOL, q = e - j * NCOL;
        float v;
        if (ABSGRAD && q >= 11) {
            v = part[j][PartRow::slotOfColumn(q)] * -EXP_INV_C1;
        } else if (q < 2) {
            // d mean = -(2 c00 A1 + (c01 + c10) A2,  2 c11 A2 + (c01 + c10) A1),  A = -1/2 of the stored sums
            const float a1 = -0.5f * part[j][A1], a2 = -0.5f * part[j][A2], cs = part[j][PartRow::c01c10];
            v = q == 0 ? -(2.0f * part[j][PartRow::c00] * a1 + cs * a2) : -(2.0f * part[j][PartRow::c11] * a2 + cs * a1);
        } else {
            v = (DEPTH || q != 10) ? part[j][PartRow::slotOfColumn(q)] : 0.0f;
            if (q < 6) v *= -0.5f;                                            // the four conic columns
        }
        if (v != 0.0f) atomicAdd(&a.gradAcc16[(size_t)(idx[j] & a.idxMask) * 16 + (ABSGRAD && q >= 11 ? q + 1 : q)], v);
    }
}

// SEG list positions per item at most; DEPTH = false: no depth cotangent (the default training case): nine sums per splat;
// ABSGRAD: the two absolute sums of pair_bwd on top.
// Four waves per SIMD, no more: the default grid (16 waves per CU, gs_ctx::bwdWavesPerCu) is one wave per slot of the chip at
// that occupancy, and the instantiations without a depth cotangent need few enough registers for a fifth wave, with which
// the dispatcher is free to fill some CUs with 20 workgroups and leave others 12.
template <int SEG, bool DEPTH, bool ABSGRAD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void blend_bwd_v2_kernel(BlendBwdArgs a)
{
    __shared__ float part[SEG][16];   // per entry of the segment: a PartRow
    __shared__ f4 sg[192];            // the staged chunk: three f4 per parked entry
    const int lane = threadIdx.x;
    BwdQueue q = bwd_queue(a);
    for (bool first = true;; first = false) {
        const uint32_t item = bwd_pop(a, q, first, lane);
        if (item >= q.nItems) {
            if (first) continue;
            break;
        }
        const BwdItem it = bwd_decode<SEG>(a, item);
        PairState ps[2];
        uint32_t hm[2];
        bwd_load_pixels<DEPTH>(a, it, lane, ps, hm);
        const uint32_t* __restrict__ idx = a.sortedIdx + it.start;
        const uint32_t n = it.i1 - it.i0;
        // rows of splats that turn out culled are never written: start from zeros
        for (uint32_t r = lane; r < n * 4; r += 64) reinterpret_cast<f4*>(&part[0][0])[r] = (f4){0.f, 0.f, 0.f, 0.f};
        for (uint32_t c0 = it.i0; c0 < it.i1; c0 += 64) {
            const uint32_t nEff = bwd_stage(a, it, hm, idx, c0, lane, sg);
            for (uint32_t jl = 0; jl < nEff; jl++) bwd_entry<DEPTH, ABSGRAD>(sg, jl, it.i0, ps, lane, part);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the LDS writes have landed (single wave)
        __builtin_amdgcn_wave_barrier();
        bwd_flush<DEPTH, ABSGRAD>(a, idx + it.i0, n, lane, part);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
constexpr int SEGLEN = GS_SEG_LEN;
// four waves per quadrant (blend_fwd_v2w_kernel) where the image has fewer quadrants than the chip has wave slots
// (gs_ctx::fwdWide: 1 / 0 force, -1 by that rule; the trace buffer and GS_TUNE_FWD_QUADRANTS 0 keep the one-wave kernel)
bool blend_forward_v2_wide(const gs_ctx* c)
{
    if (c->fwdTrace || !c->fwdQuadrants) return false;
    return c->fwdWide == 1 || (c->fwdWide < 0 && c->numPixBlocks * 4 <= c->numCUs * 4 * c->fwdWavesPerSimd);
}
// a staging wave beside every sweeping wave (blend_fwd_v2p_kernel; gs_ctx::fwdPair): where the one-wave kernel would run
// fwdPair < 0: by the depth of the lists -- the pair count of the context's PREVIOUS forward (a word the expansion leaves in
// mapped host memory: read without a wait, a forward late) per pixel block.  Measured (MI355X, blend forward, one-wave / pair):
// c3 grown to 1 M Gaussians, 8400 pairs per block: 0.890 -> 0.805 ms; c3 at 200 x 200 tiles, 5070: 0.237 / 0.238; c3, 3160:
// 0.175 / 0.176; c2 0.174 / 0.174; the 2 M garden scene under its depth cuts, 740: 0.311 -> 0.320.  The decision is taken ONCE
// per forward (gs_render_forward, fwdPairNow): the word it reads changes while the forward is being enqueued, and the grid,
// the checkpoint pools sized by it and the kernel launched must follow from one reading.
bool blend_forward_v2_pair_decide(const gs_ctx* c)
{
    if (c->fwdTrace || !c->fwdQuadrants || blend_forward_v2_wide(c)) return false;
    if (c->fwdPair >= 0) return c->fwdPair != 0;
    const unsigned long long lastM = c->missHost ? c->missHost[8] : 0u;
    // (4500: round 6's lists are trimmed rects in row groups -- the grown scene's 8400 pairs per block became 5500, its staging-wave
    // forward still 5 % ahead, 0.868 -> 0.825 ms; 200 x 200 tiles on block lists, 5070: level either way)
    return c->numPixBlocks > 0 && lastM / (unsigned long long)c->numPixBlocks >= 4500ull;
}
// the grid the fused forward is launched with, in takers (waves of the one-wave kernel, workgroups of the other two)
static int blend_forward_v2_grid(const gs_ctx* c)
{
    const int fwdItems = c->numPixBlocks * 4;
    const int fwdGrid = blend_forward_v2_wide(c) ? c->numCUs * GS_V2W_WGS
                        : c->fwdPairNow ? c->numCUs * (c->fwdPair > 1 ? c->fwdPair : GS_V2P_WGS)
                                                   : c->numCUs * 4 * c->fwdWavesPerSimd;
    return fwdGrid > fwdItems ? fwdItems : fwdGrid;
}

void fill_seg_base(gs_ctx* c, SegBaseArgs& a)
{
    a.nBlocks = c->numPixBlocks; a.blocksX = c->blocksX; a.tileW = c->tileW; a.tileH = c->tileH; a.gridW = c->gridW;
    a.tileRanges = c->tileRanges; a.tileTotal = nullptr;
    a.segBase = c->segBase; a.blockWork = c->blockWork; a.counters = c->counters; a.workHint = c->workHint;
    a.blockOrder = c->blockOrder; a.fwdQueue = c->fwdQueue;
}

int launch_blend_forward_v2(gs_ctx* c, float* outColor, float* outDepth, float* outAlpha)
{
    // the backward of THIS forward reads what it wrote; without a depth image there is no depth cotangent to come either
    // (render-only forwards keep no checkpoints at all: the arena's arithmetic below then runs on four planes and is not used)
    const int planes = c->depthGradient && outDepth ? 5 : 4;
    c->fwd.statePlanes = planes;
    const int grid = blend_forward_v2_grid(c);
    if (c->segBaseDone) c->segBaseDone = false;        // the tile sort's launch has done it (binning.hip)
    else {
        SegBaseArgs sa;
        fill_seg_base(c, sa);
        hipLaunchKernelGGL(seg_base_kernel<SEGLEN>, dim3(1), dim3(1024), 0, c->stream, sa);
    }
    const bool wide = blend_forward_v2_wide(c), pair = !wide && c->fwdPairNow;
    // capacity in slots of THIS forward's planes (the arena is sized for five)
    const uint32_t qcap = (uint32_t)(c->qslotCap * 5 / c->fwd.statePlanes);
    c->fwd.qslotCap = qcap;
    // the waves that own a checkpoint pool: every wave of the one-wave kernel (its grid counts waves), the sweeping wave of a
    // pair, all four waves of a four-wave workgroup
    const uint32_t poolWaves = (uint32_t)grid * (wide ? 4u : 1u);
    // three quarters of the arena at most are handed out statically, up to 32 slots (2048 list entries of one quadrant)
    // per wave; the rest is the shared part, in eight
    uint32_t own = (uint32_t)(((unsigned long long)qcap * 3ull / 4ull) / (unsigned long long)poolWaves);
    if (own > 32u) own = 32u;
    c->fwd.qslotStatic = own * poolWaves;
    const uint32_t partSlots = (qcap - c->fwd.qslotStatic) / 8u;
    // test knob (GS_TUNE_POISON_CHECKPOINTS): every checkpoint lane this forward does not write reads back as NaN
    if (c->poisonCheckpoints && c->segState)
        GS_HIP_CHECK(c, hipMemsetAsync(c->segState, 0xFF, (size_t)c->qslotCap * 5 * 64 * sizeof(float), c->stream));
    BlendFwdArgs a;
    a.W = c->W; a.H = c->H; a.tileW = c->tileW; a.tileH = c->tileH; a.gridW = c->gridW; a.blocksX = c->blocksX;
    a.nItems = c->numPixBlocks * 4;
    a.bgc = c->modes.bg;
    a.rec12 = reinterpret_cast<const float4*>(c->packed12); a.sortedIdx = c->sortedRaw; a.idxMask = c->idxMask;
    a.tileRanges = c->tileRanges; a.segBase = c->segBase; a.segCap = (uint32_t)c->segCap;
    a.statePlanes = c->renderOnly ? 0 : c->fwd.statePlanes;
    a.outColor = outColor; a.outDepth = outDepth; a.outAlpha = outAlpha; a.lastContrib = c->lastContrib; a.finalT = c->finalT;
    a.segState = c->segState; a.segSlot = c->segSlot;
    a.qslotCap = qcap; a.qslotOwn = own; a.qslotShared0 = c->fwd.qslotStatic; a.qslotPart = partSlots; a.ckptPool = ckpt_pool(partSlots, poolWaves);
    a.blockWork = c->blockWork; a.counters = c->counters; a.fwdQueue = c->fwdQueue; a.nq = (uint32_t)c->fwdQueues;
    a.blockOrder = c->blockOrder; a.cutStore = c->fwd.cutsActive ? c->fwd.cutStore : nullptr; a.hostWords = c->missDev;
    a.vg = c->virt;
    a.trace = c->fwdTrace; a.slowSlot = (uint32_t)c->fwdSlowSlot; a.foldScale = c->fwdFoldScale;
    auto kw = outDepth ? blend_fwd_v2w_kernel<SEGLEN, true> : blend_fwd_v2w_kernel<SEGLEN, false>;
    auto kp = outDepth ? blend_fwd_v2p_kernel<SEGLEN, true> : blend_fwd_v2p_kernel<SEGLEN, false>;
    auto kq = outDepth ? blend_fwd_v2q_kernel<SEGLEN, true> : blend_fwd_v2q_kernel<SEGLEN, false>;
    if (wide) hipLaunchKernelGGL(kw, dim3(grid), dim3(256), 0, c->stream, a);               // four waves per quadrant: the grid is workgroups
    else if (pair) hipLaunchKernelGGL(kp, dim3(grid), dim3(128), 0, c->stream, a);          // a sweeping and a staging wave: the grid is workgroups
    else hipLaunchKernelGGL(kq, dim3(grid / 4), dim3(256), 0, c->stream, a);                // four independent waves: the grid is waves, a multiple of four
    GS_HIP_CHECK(c, hipGetLastError());
    if (c->renderOnly) c->fwd.statePlanes = 0;          // (backward_preflight refuses such a forward)
    return GS_OK;
}

void fill_bwd_prep(gs_ctx* c, int N, BwdPrepArgs& p)
{
    p.nBlocks = c->numPixBlocks;
    p.blockWork = c->fwd.blockWork;
    p.itemBlock = c->itemBlock;
    p.itemRow = c->itemRow;
    p.segBase = c->segBase;
    p.itemCap = (uint32_t)c->itemCap;
    p.counters = c->counters;
    p.bwdQueue = c->bwdQueue;
    p.clearBuf = reinterpret_cast<float4*>(c->gradAcc16);
    p.clearCount = (size_t)N * 4;
    // the view's cuts are renewed whenever the caller keeps them (gs_set_view_hints), in force this forward or not
    p.cutStore = c->fwd.cutStore;
    p.cutsInForce = c->fwd.cutsActive ? 1 : 0;
    p.tileRanges = c->tileRanges;
    p.sortedIdx = c->sortedRaw;
    p.idxMask = c->idxMask;
    p.rec12 = c->packed12;
}

int launch_blend_backward_v2(gs_ctx* c, int N, const float* cotColor, const float* cotDepth, const float* cotAlpha,
                             const float* outColor, const float* outDepth, const float* outAlpha, bool absgrad)
{
    int grid = c->numCUs * c->bwdWavesPerCu;           // single-wave workgroups
    if ((long long)grid > c->itemCap) grid = (int)c->itemCap;
    if (grid < 1) grid = 1;
    BwdPrepArgs prep;
    fill_bwd_prep(c, N, prep);
    // gs_loss_forward_backward has carried all of this along with its own kernel (ssim.hip) when the loss of this
    // forward went through the library
    const bool prepared = c->fwd.bwdPrepared && c->fwd.preparedN == N;
    c->fwd.bwdPrepared = false;          // consumed: a second backward of the same forward prepares for itself
    if (!prepared) {
        const int cutBlocks = prep.cutStore ? gs_div_up(c->numPixBlocks, 1024) : 0;
        const int clearBlocks = (int)((prep.clearCount + 8191) / 8192 < 1024 ? (prep.clearCount + 8191) / 8192 : 1024);
        hipLaunchKernelGGL(bwd_items_kernel<SEGLEN>, dim3(GS_ITEM_PARTS + cutBlocks + clearBlocks), dim3(1024), 0, c->stream, prep, cutBlocks);
    }
    BlendBwdArgs a;
    a.W = c->W; a.H = c->H; a.tileW = c->tileW; a.tileH = c->tileH; a.gridW = c->gridW; a.blocksX = c->blocksX;
    a.bgc = c->fwd.modes.bg;
    a.rec12 = reinterpret_cast<const float4*>(c->packed12); a.sortedIdx = c->sortedRaw; a.idxMask = c->idxMask;
    a.tileRanges = c->tileRanges; a.blockWork = c->fwd.blockWork;
    a.itemBlock = c->itemBlock; a.itemRow = c->itemRow; a.counters = c->counters;
    a.segSlot = c->segSlot; a.segState = c->segState;
    a.qslotCap = c->fwd.qslotCap; a.statePlanes = c->fwd.statePlanes;
    a.bwdQueue = c->bwdQueue; a.nq = GS_QUEUES;
    a.cotColor = cotColor; a.cotDepth = cotDepth; a.cotAlpha = cotAlpha;
    a.outColor = outColor; a.outDepth = outDepth; a.outAlpha = outAlpha; a.finalT = c->finalT;
    a.lastContrib = c->lastContrib; a.gradAcc16 = c->gradAcc16; a.vg = c->virt;
    auto kern = absgrad ? (cotDepth ? blend_bwd_v2_kernel<SEGLEN, true, true> : blend_bwd_v2_kernel<SEGLEN, false, true>)
                        : (cotDepth ? blend_bwd_v2_kernel<SEGLEN, true, false> : blend_bwd_v2_kernel<SEGLEN, false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, c->stream, a);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace gs
