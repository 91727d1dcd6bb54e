// gs_ctx.h -- context/workspace shared by the translation units of libgsplat_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/gsplat.h"
#include "gs_math.h"
#include "gs_mem.h"

// device counters held in ctx->counters (u32 each)
enum {
    GS_CNT_M = 0,         // pairs actually binned (0 on overflow)
    GS_CNT_OVERFLOW = 1,  // 1 if M exceeded the reserved capacity
    GS_CNT_MREQ = 2,      // M that was required
    GS_CNT_B = 3,         // max tile list length
    GS_CNT_NVIS = 4,      // Gaussians with radius > 0
    GS_CNT_CONTRIB_LO = 5,
    GS_CNT_CONTRIB_HI = 6,
    GS_CNT_ITEMS = 9,     // backward work items (block, segment)
    GS_CNT_CUT_DROPPED = 12,  // statistics: candidate pairs the depth cuts left out (low 32 bits)
    GS_CNT_QSLOTS = 16,   // ... + 8: checkpoint slots (one 8x8 quadrant each) the fused forward's waves have drawn from the
                          // shared part of the arena, one counter per eighth of it (blend_v2.hip)
    GS_CNT_COUNT = 24
};

// work queues of the fused blend kernels (blend_v2.hip): one head per XCD, each on a 128-byte line of its own
constexpr uint32_t GS_QUEUES = 8;
constexpr uint32_t GS_QUEUE_STRIDE = 32;    // words from one queue's head to the next

constexpr int GS_SORT_THREADS = 256;
constexpr int GS_SORT_ITEMS = 16;
constexpr int GS_SORT_TILE = GS_SORT_THREADS * GS_SORT_ITEMS;  // elements per sort block
constexpr int GS_SMALL_SORT_ITEMS = 16;     // elements per thread of the small (depth) sort's tiles (4: 1024-element tiles were
                                            // slower, 11 -> 14 us per scatter: four times the histogram rows to sum per block)
constexpr int GS_SMALL_SORT_BLOCKS = 160;   // depth sorts of up to this many tiles (655 k Gaussians) take the two-launch passes
constexpr int GS_SORT_MAX_GRID = 2048;      // blocks of a radix kernel launched for a device-resident count (they walk the rest)
constexpr uint32_t GS_SORT_NO_KEY = 0xFFFFFFFFu;   // depth key of a Gaussian that touches no tile (never a real key: a NaN)
constexpr int GS_WIDE_BINS = 4096;          // one-pass tile sort: a 12-bit digit covers every tile id when T <= 4096
constexpr int GS_WIDE_CHUNK = 16;           // sort tiles per scan chunk (an exclusive prefix inside a chunk stays < 2^16)
constexpr int GS_SCAN_BLOCK = 256;
constexpr uint32_t GS_SLICE_MIN_PAIRS = 32768;   // ... of the blocks that have at least this many positions
constexpr int GS_EXPAND_SLICES = 8;       // slices of a wave's positions in the expansion of large inputs (binning.hip)
constexpr int GS_FUSED_SCAN_MAX = 2048;   // scan blocks up to which every expansion block sums the block counts itself
constexpr int GS_SEG_LEN = 64;  // splats per saved-state segment of the fused blend (multiple of 4)

// Adam's parameter step lr m / (sqrt(v) + eps) with the hardware's 1-ulp v_sqrt_f32 and v_rcp_f32 instead of the
// correctly rounded sqrtf and division (~22 VALU instructions per element less; the fused projection backward + Adam
// kernel spent 40 % of its instructions there).  The step differs from the IEEE one by at most ~3e-7 relative, the
// moments not at all; MLX's Metal kernels are fast-math themselves and no reference test pins Adam.
#if defined(__HIPCC__)
__device__ __forceinline__ float gs_adam_delta(float lr, float m, float v, float eps)
{
    return (lr * m) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + eps);
}
#endif

// The colour the blend composites over (gs_set_background), a by-value argument of every blend kernel.
// BLACK and WHITE are the creation backgrounds and keep the expressions they always had (0 and T; 0 and gx + gy + gz), so an
// unset context computes bit for bit what it did before the colour existed; COLOUR adds T b_c per channel.
enum { GS_BG_BLACK = 0, GS_BG_WHITE = 1, GS_BG_COLOUR = 2 };
struct GsBackground {
    int mode = GS_BG_BLACK;
    float r = 0.0f, g = 0.0f, b = 0.0f;
};
#if defined(__HIPCC__)
// the three background terms T b_c of a pixel.  Each is ONE rounded product (__fmul_rn: never contracted into the sum it joins,
// whatever -ffp-contract says), so the fused backward takes off the stored image exactly what the forward put on
__device__ __forceinline__ void gs_bg_terms(const GsBackground& bg, float T, float& t0, float& t1, float& t2)
{
    if (bg.mode == GS_BG_COLOUR) { t0 = __fmul_rn(T, bg.r); t1 = __fmul_rn(T, bg.g); t2 = __fmul_rn(T, bg.b); }
    else t0 = t1 = t2 = bg.mode ? T : 0.0f;
}
// d(colour . cot) / dT through the background: g . b
__device__ __forceinline__ float gs_bg_cot(const GsBackground& bg, float gx, float gy, float gz)
{
    if (bg.mode == GS_BG_COLOUR) return fmaf(gx, bg.r, fmaf(gy, bg.g, __fmul_rn(gz, bg.b)));
    return bg.mode ? (gx + gy + gz) : 0.0f;
}
#endif

struct GsDp;      // dp.hip: communicator, side stream and events of the data-parallel step

// the fused forward's SH colours as rider workgroups of the binning kernels (gs_rider.h): what a rider needs, by value
struct GsColourRider {
    const float* xyz;
    const float* fdc;
    const float* frest;
    float* packed12;
    const uint32_t* tilesTouched;
    float cam[3];
    int N, degree;
    int unit0, units;        // this launch's share: the waves [unit0, unit0 + units) of 64 Gaussians each
};
// host kernels of the riders (binning.hip), index into gs_ctx::riderShare
enum { GS_RIDE_SS_HIST = 0, GS_RIDE_SS_SCATTER, GS_RIDE_WIDE_TILE, GS_RIDE_HOSTS };
struct GsRiderState {
    bool on = false;         // a geometry-only projection has run: colour units are outstanding
    GsColourRider args = {};
    int next = 0, total = 0; // units handed out so far / units of the forward
};

// Block geometry of the fused path when the caller's tile size is not a multiple of 16 (the reference app's W/4 x H/4):
// every tile is cut into nbx x nby pixel blocks of 16 x 16 (the last column / row narrower), and the fused path bins, sorts and
// blends per BLOCK -- the context's tileW / tileH / gridW / gridH / T then describe that block grid ("block lists"), while the
// op-level entry points swap the caller's tile grid back in (GsRealGeom, api.hip).  nbx == 0: the regular 16 x 16 grid over the
// image, blocks and tiles related by division as before.
struct GsVirtGeom {
    int nbx = 0, nby = 0;    // blocks per tile
    int tw = 0, th = 0;      // the caller's tile size in pixels
};
// pixel origin and exclusive pixel limits of block (bx, by); all arguments wave-uniform
__device__ __forceinline__ void gs_block_pixels(const GsVirtGeom& g, int bx, int by, int W, int H, int& X0, int& Y0, int& XL, int& YL)
{
    if (g.nbx == 0) { X0 = bx * 16; Y0 = by * 16; XL = W; YL = H; return; }
    const int tx = bx / g.nbx, ix = bx - tx * g.nbx, ty = by / g.nby, iy = by - ty * g.nby;
    X0 = tx * g.tw + ix * 16; Y0 = ty * g.th + iy * 16;
    XL = min(W, min(X0 + 16, (tx + 1) * g.tw)); YL = min(H, min(Y0 + 16, (ty + 1) * g.th));
}
constexpr int GS_F3D_CAM_FLOATS = 16;  // floats per camera of the 3-D filter's table (filter3d.hip)
constexpr int GS_CUT_SUPER = 4;      // tiles per side of a super-tile of the coarse cuts
// coarse depth cuts handed to the fused projection (binning.hip, cut_super_kernel): null superCut = a forward without cuts
struct GsCutCoarse {
    const uint32_t* superCut = nullptr;
    int superW = 0;
    uint32_t* dropPerBlock = nullptr;
};
struct GsRealGeom {          // the caller's tile grid (what the op-level entry points see)
    int tileW = 16, tileH = 16, gridW = 0, gridH = 0, T = 0, tileBits = 1;
    bool fast16 = false;
};

// What a forward runs under, and its backward with it.  gs_ctx holds it twice: `modes`, what the setters write for the next
// forward, and `fwd.modes`, what the last forward ran under -- copied whole by gs_render_forward, so a field added here is
// snapshotted without another line
struct GsRenderModes {
    // pose refinement (gs_set_pose_correction): caller-owned device delta[6] / grad_delta[6] (where the backward writes
    // dL/d delta), nullptr = off
    const float* poseDelta = nullptr;
    float* poseGrad = nullptr;
    bool antialias = false;              // gs_set_antialiasing: the anti-aliased mode
    bool fisheye = false;                // gs_set_camera_model: GS_CAMERA_FISHEYE (also read by the op-level projection)
    int degree = 0;                      // the active SH degree (gs_set_sh_degree), 0 .. gs_ctx::maxDegree
    GsBackground bg;                     // gs_set_background: what the blend composites over (unset: whiteBg's black or white)
    const float* filter3d = nullptr;     // gs_set_filter3d: the caller-owned device widths [>= N], nullptr = off
};

struct gs_ctx {
    int device = 0;
    GsDp* dp = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    int W = 0, H = 0, tileW = 16, tileH = 16, gridW = 0, gridH = 0, T = 0, whiteBg = 0;
    int tileBits = 1;
    GsRenderModes modes;         // the settings of the following forwards (fwd.modes: what the last one ran under)
    bool fast16 = false;
    GsVirtGeom virt;             // block lists (above); virt.nbx != 0 <=> tileW .. T describe the block grid, `real` the caller's
    GsRealGeom real;
    bool binIsBlockLists = false;  // the context's last binning was a fused forward's under block lists
    int blocksX = 0, blocksY = 0;  // pixel blocks per row / column of the fused path (numPixBlocks = blocksX * blocksY)
    std::string err;

    // capacities
    int capN = 0;
    long long capM = 0;
    bool pairsReserved = false;  // caller sized capM itself: no host check of M per call
    bool reserving = false;      // inside gs_ctx_reserve with a pair reserve (pairsReserved is set once it has succeeded)
    GsMem mem;                   // every device and pinned buffer below that the context owns (ctx_alloc .. ctx_grow, below)

    // per-Gaussian workspace
    float* packed12 = nullptr;       // [capN,12] means2d, conic, colour, opacity, depth, pad 
    float* gradAcc16 = nullptr;      // [capN,16] blend-backward accumulator (64-B rows)
    uint32_t* depthKey[2] = {nullptr, nullptr};
    uint32_t* depthVal[2] = {nullptr, nullptr};
    uint32_t* tilesTouched = nullptr;  // [capN] by Gaussian index
    uint4* tilePieces = nullptr;       // [capN] trimmed rects: the four row groups of tileRect (first column | columns << 16), gs_math.h rect_row_groups4
    bool piecesValid = false;          // the projection of the forward in flight wrote them: its expansion enumerates row groups
    ushort4* tileRect = nullptr;       // [capN] x0,y0,x1,y1
    uint32_t* blockSums = nullptr;     // [capN/256+1]
    uint32_t* visPerBlock = nullptr;   // [capN/128+1] visible (radius > 0) Gaussians per projection block; summed on demand
    int visBlocks = 0;
    // per-pair workspace
    uint32_t* pairKey[2] = {nullptr, nullptr};
    uint32_t* pairVal[2] = {nullptr, nullptr};
    // radix scratch
    uint32_t* hist = nullptr;  // [256, nbCap]
    uint32_t* rowTotal = nullptr;  // [256]
    uint16_t* wideCnt = nullptr;     // [nbCap][4096] one-pass tile sort: pairs per (sort tile, tile id), then prefixes inside a chunk
    uint32_t* wideChunk = nullptr;   // [nbCap / 16 + 1][4096] pairs per (chunk, tile id), then prefixes over the chunks
    uint32_t* wideTotal = nullptr;   // [4096] pairs per tile id
    uint2* sortBits = nullptr;     // [GS_SMALL_SORT_BLOCKS] per sort tile: AND / OR of the depth keys that have pairs
    // splitter depth sort (binning.hip): splitters of the previous sort (double-buffered), bucket of every record, bucket starts
    uint32_t* sortSplit[2] = {nullptr, nullptr};   // [256] each
    int splitCur = 0;
    bool haveSplitters = false;
    unsigned char* bucketId = nullptr;             // [capN]
    uint32_t* bucketStart = nullptr;               // [520]: first record of every bucket, [256] = n
    int colourRiders = 1;          // 1: K = 25 forwards compute their SH colours as riders of the binning kernels (GS_TUNE_COLOUR_RIDERS)
    GsRiderState rider;
    int riderShare[GS_RIDE_HOSTS] = {200, 500, 300};   // permille of a forward's colour units per host kernel
    int splitterSort = 1;          // 1: depth sorts of 16385 .. 655 k records take the splitter buckets (three launches); 0: LSD passes
    int nbCap = 0;
    // per-tile
    bool superCutReady = false;      // cut_super_kernel has run for the forward being built (the fused projection uses it first)
    uint32_t* dropPerBlock = nullptr; // [capN / 128 + 1] candidate pairs of the Gaussians each projection block dropped whole under the super-cuts
    int dropBlocks = 0;              // how many of them the current forward wrote (0: none -- no cuts, or an op-level binning)
    uint32_t* superCut = nullptr;    // [ceil(gridW / 4) * ceil(gridH / 4)] the deepest cut of every 4 x 4 tiles (binning.hip, cut_super_kernel)
    uint32_t* tileRanges = nullptr;  // [T,2]
    uint32_t* tileCounts = nullptr;  // [T]
    // per 16x16 pixel block: work estimate and heaviest-first launch order (fast path)
    uint32_t* blockWork = nullptr;   // [numPixBlocks] active buffer: blockWorkOwn, or the caller's (gs_set_block_work_buffer)
    uint32_t* blockWorkOwn = nullptr;
    uint32_t* blockOrder = nullptr;  // [numPixBlocks]
    uint32_t* fwdQueue = nullptr;    // [GS_QUEUES][GS_QUEUE_STRIDE] work-queue heads of the fused blend forward, one per XCD
    uint32_t* bwdQueue = nullptr;    // ... and of the fused blend backward (a stripe of the item list each)
    // depth cuts (binning.hip): per tile, 0xFFFFFFFF - (largest depth key still binned); 0 = no cut.  Lives in the
    // caller's per-view hint buffer behind the block-work words (gs_set_view_hints); written by the backward's item
    // kernel, read by the next forward of that view.
    uint32_t* cutStore = nullptr;
    bool allowCuts = true;
    const uint32_t* opCuts = nullptr;    // gs_tile_bin_cut: the caller's per-tile cuts, for the duration of that call
    unsigned long long* scanTmp = nullptr;      // [.. / 1024 + 4] chunk sums of the large prefix
    unsigned long long* scanPrefix = nullptr;   // [capN/64 + 16] prefix of block / segment counts (large inputs only)
    uint2* waveSeg = nullptr;            // [capN/64 + 8] per expansion wave: start and length of its segment of kept pairs
    uint32_t* missHost = nullptr;        // pinned, mapped: [0] = 1 if a tile with a cut ended with live pixels; [1], [2] cut
                                         // statistics; [4] = 1 once a forward overflowed the reserved pairs, [5] = the M it needed
    uint32_t* missDev = nullptr;         // device address of missHost
    hipEvent_t fwdDone = nullptr;        // recorded after the forward blend when cuts were active
    const uint32_t* workHint = nullptr;  // = the caller's block-work buffer: sweep lengths of an earlier forward of this view
    // pose refinement (modes.poseDelta): the composed camera of the last posed forward (pose_camera_kernel) and the backward's
    // wave partials ([16 x waves], grown on demand)
    gs::CamParams* poseCam = nullptr;
    float* posePartials = nullptr;
    long long posePartialsCap = 0;
    // exposure compensation (gs_set_exposure): caller-owned device M[12] / grad[12], nullptr = off; the corrected image the
    // loss reads ([H, W, 3], shared with the bilateral grid) and the backward's per-workgroup float64 partials, both allocated
    // at the first exposure set
    const float* expoM = nullptr;
    float* expoGrad = nullptr;
    float* correctedImage = nullptr;
    double* expoPartials = nullptr;
    // bilateral grid (gs_set_bilateral_grid): caller-owned device grid / grad of bgW x bgH x bgL nodes, nullptr = off (never
    // together with an exposure: the loss reads the corrected image from correctedImage); the backward's per-(cell, chunk) partials,
    // grown only by gs_set_bilateral_grid, and the chunk count of the grid shape they were sized for
    const float* bgGrid = nullptr;
    float* bgGrad = nullptr;
    int bgW = 0, bgH = 0, bgL = 0;
    float bgTv = 0.0f;
    int bgChunks = 0, bgChunksW = 0, bgChunksH = 0;
    float* bgPartials = nullptr;
    long long bgPartialsCap = 0;
    int maxDegree = 0;                   // gs_ctx_create's sh_degree; modes.degree is the active one (gs_set_sh_degree), 0 .. maxDegree
    int shBandSkip = 1;                  // GS_TUNE_SH_BAND_SKIP: 1 = a lower-degree fused Adam step takes the BANDS form (projection.hip)
    bool absgrad = false;                // gs_set_absgrad: the fused backward also sums |g_x|, |g_y| per Gaussian
    int absgradN = -1;                   // N of the last backward that left (Ax, Ay) in gradAcc16's columns 12, 13; -1: none to read
    // sparse Adam (gs_set_sparse_adam): while on, every fused forward leaves radius > 0 of its N Gaussians
    // as bytes in visMask (vis_mask_kernel behind the projection, from the radii the projection wrote: the caller's buffer, or
    // visRadii where the caller takes none); both [visCap], grown by the first forward that needs more, never by a backward
    bool sparseAdam = false;
    unsigned char* visMask = nullptr;
    float* visRadii = nullptr;
    int visCap = 0;
    int visN = -1;                       // N of the last fused forward made under the setting (its mask is in visMask); -1: none
    // adaptive density control (gs_set_adc_stats): caller-owned [N] accumulators, all set or all nullptr.
    // While set, every fused forward keeps its radii (the caller's buffer, or visRadii as under sparse Adam) and the blend backward
    // of gs_render_backward / gs_render_backward_adam adds the step's statistic (adc.hip adc_accum_kernel)
    float* adcGradSum = nullptr;
    float* adcCount = nullptr;
    float* adcMaxRadius = nullptr;
    // 3-D smoothing filter (modes.filter3d): the training cameras' table for gs_compute_filter3d (GS_F3D_CAM_FLOATS floats per
    // camera) and the max word of its never-seen rule, both allocated or grown by gs_set_filter3d_cameras only
    float* f3dCams = nullptr;
    int f3dCamCount = 0, f3dCamCap = 0;
    uint32_t* f3dMax = nullptr;
    bool mcmcOn = false;                 // gs_set_mcmc: the MCMC strategy's step in gs_render_backward_adam, with these parameters
    gs_mcmc_params mcmc = {};
    char* mcmcWs = nullptr;              // mcmc.hip: the event's scratch (grown on demand) and its pinned read-back words
    size_t mcmcWsBytes = 0;
    long long* mcmcHost = nullptr;
    float* gradNormAccum = nullptr;      // caller-owned [N]: the projection backward adds |grad xyz| (gs_set_grad_norm_accum)
    uint32_t* segBase = nullptr;     // [numPixBlocks] first saved-state slot of each block
    float* segState = nullptr;       // [qslotCap][5][64] running (T, C, D) of an 8x8 quadrant, saved every GS_SEG_LEN splats
    uint32_t* segSlot = nullptr;     // [segCap][4] slot of (block's first segment + segment, quadrant); blend_v2.hip
    long long segCap = 0;            // table rows: every list swept to its end
    long long qslotCap = 0;          // slots the arena holds (allocated as they are written)
    long long qslotWanted = 0;       // ... and what the next (re)allocation must hold at least (after an arena overflow)
    bool arenaRegrowPending = false; // an arena overflow has been reported; gs_ctx_reserve acts on it
    uint32_t* itemBlock = nullptr;   // [itemCap] backward work items
    uint32_t* itemRow = nullptr;     // [itemCap] their rows of the checkpoint-slot table
    long long itemCap = 0;
    float* finalT = nullptr;         // [P] exact final transmittance of the fused forward
    int numCUs = 256;
    int numPixBlocks = 0;
    int opBlocks = 0;                // work items of the op-level blend kernels (blend.hip): numPixBlocks, or -- tile sizes
                                     // that are not multiples of 16 -- the 16x16 blocks enumerated per tile
    // launch tuning (gs_ctx_set_tuning; per context): measured optima of tools/sweep.sh as defaults
    int fwdWavesPerSimd = 4, bwdWavesPerCu = 16;
    int fwdQuadrants = 1;            // GS_TUNE_FWD_QUADRANTS: the forward's items are always 8x8 quadrants (the 16x8 variant it once
                                     // selected is gone); 0 still forces the one-wave kernel over the pair and four-wave kernels
                                     // (blend_forward_v2_wide, blend_forward_v2_pair_decide)
    int fwdWide = -1;                // blend forward with four waves per quadrant: 1 / 0, -1 = where the image has fewer quadrants than wave slots (blend_v2.hip)
    float fwdFoldScale = 1.0f;       // test knob (GS_TUNE_FWD_FOLD_TEST_SCALE): factor on the composed T in the four-wave fold's
                                     // "did the pixel cross 1e-4 inside this part" test; below 1 forces second takes that come back live
    int fwdSlowSlot = 3;             // GS_TUNE_FWD_SLOW_SLOT: waves of the one-wave forward in a hardware wave slot >= this take their
                                     // static first item and nothing from the queues (16 = off; blend_v2.hip)
    int fwdPair = -1;                // GS_TUNE_FWD_PAIR: 0 = the one-wave forward, 1 = a staging wave beside every sweeping wave
                                     // (blend_fwd_v2p_kernel, 12 workgroups per CU), n > 1 = that with n workgroups per CU,
                                     // -1 (default) = where the previous forward's lists were deep (blend_forward_v2_pair_decide)
    bool fwdPairNow = false;         // this forward's decision (taken once, in gs_render_forward)
    bool trimRects = true;           // GS_TUNE_TRIM_RECTS: at 16 x 16 tiles the fused forward bins a Gaussian on its 3-sigma square cut by the
                                     // box of q <= 40.3 (projection.hip; gs_math.h block_rect_of_splat) instead of on the whole square
    bool rowGroups = true;           // GS_TUNE_TRIM_RECTS = 2 (default) / 1: trimmed rects cut further into four row groups, or the box alone
    int renderOnly = 0;              // GS_TUNE_RENDER_ONLY: fused forwards keep no checkpoints (statePlanes 0) and can have no backward
    int poisonCheckpoints = 0;       // test knob (GS_TUNE_POISON_CHECKPOINTS): the checkpoint arena is NaN-filled in front of every fused forward
    int fwdQueues = 8;               // work queues of the fused forward: 8 = one per XCD (blend_v2.hip), 1 = one for the chip (A/B)
    int opFwdPpl = 1, opBwdPpl = 1;  // pixels per lane of the op-level blend kernels (blend.hip)
    bool segBaseWanted = false;      // gs_render_forward (16x16-block path): the binning may do the blend forward's
    bool segBaseDone = false;        //   bookkeeping in its tile-sort launch (gs_bwd_prep.h, seg_base_body) / it has
    int wideTileSort = 1;            // 1: one-pass tile sort when T <= 4096 (binning.hip); 0: the two 8-bit passes (A/B, tests)
    int hostOverflowErrors = 1;      // 0: a reserved-capacity overflow is reported by gs_sync only (GS_TUNE_HOST_OVERFLOW_ERRORS)
    int depthGradient = 1;           // 0: the caller promises cot_depth == NULL in every fused backward (default training,
                                     // SURVEY a11): the forward then checkpoints (T, R, G, B) without the depth sum
    unsigned long long* fwdTrace = nullptr;   // diagnostic: per-item (start, end, iterations, hw id) of the fused forward
    const uint32_t* adamGate = nullptr;       // device word: non-zero = every optimizer kernel leaves the parameters alone
                                              // (default: counters + GS_CNT_OVERFLOW; gs_set_update_gate)
    // data-parallel steps, round 5: the step's gate rides in its first collective instead of in a 4-byte all-reduce of its own
    float* overflowRider = nullptr;           // gs_set_overflow_rider: where the first kernel of a backward stores the forward's overflow
                                              // word as 0.0f / 1.0f (behind the colour cotangents / the gradient arena)
    long long ccBlockFloats = 0;              // gs_set_gathered_gate: floats per rank block of the gathered colour cotangents (0: 3 N, no
    int ccBlockCount = 0;                     //   gathered gate), how many blocks,
    uint32_t* gatheredGateOut = nullptr;      //   and where the SH rebuild stores the OR of their rider words
    uint32_t* gateSeen = nullptr;             // gs_set_gate_seen: set to 1 by an optimizer kernel that finds its gate raised
    // per-pixel (saved forward state for the fused path)
    uint32_t* lastContrib = nullptr;  // [P]
    float* lossPartials = nullptr;    // [lossPartialBlocks*4 + 16]
    float* lossTargetCache = nullptr; // caller-owned [2][3][H][W]: the target's windowed mean and mean of squares (ssim.hip)
    bool lossTargetCacheFilled = false;
    const unsigned char* lossMask = nullptr;   // gs_set_loss_mask: caller-owned [H][W] per-pixel loss weights v / 255, nullptr = off
    int lossPartialBlocks = 0;
    double* depthLossWs = nullptr;    // gs_depth_loss: [depth_loss_ws_doubles()] per-block (sum, count) partials + n, allocated at the first call
    float* normalWs = nullptr;        // gs_normal_loss: [normalWsFloats] the normals and q, 7 floats per pixel, allocated at the first
    long long normalWsFloats = 0;     //   call, regrown only for a larger image; normalPartials: [normal_loss_ws_doubles()]
    double* normalPartials = nullptr;
    double* distortionWs = nullptr;   // gs_distortion_loss: [distortion_loss_ws_doubles()] per-block partial sums, allocated at the first call
    // gs_arm_distortion: the distortion term of the current forward (host state only: an unarmed backward launches nothing more);
    // cot [H, W] and totals [H, W, 3] are the caller's, read by the distortion backward behind the blend backward
    struct {
        bool armed = false;
        gs_distortion_params params = {};
        const float* cot = nullptr;
        const float* totals = nullptr;
    } distortion;
    double* metricsWs = nullptr;      // gs_image_metrics / gs_colour_moments: [metricsWsDoubles] per-block partials, allocated at the
    long long metricsWsDoubles = 0;   //   first call, regrown only for a larger image (metrics.hip metrics_ws_doubles)
    float* windowDev = nullptr;       // [121] default SSIM window
    // densify scan scratch: [densifyInts] 5 ints per scan tile (sum, histogram) + 8 counters, grown on demand
    int* densifyTiles = nullptr;
    long long densifyInts = 0;
    // the planned densify event (densify.hip): its plan words on the device, their copy in pinned host memory, the event behind them
    uint32_t* densifyPlan = nullptr;
    uint32_t* densifyPlanHost = nullptr;
    uint32_t* densifyPlanHostDev = nullptr;
    hipEvent_t densifyDone = nullptr;
    bool densifyPlanned = false;
    float** densifyTable = nullptr;      // device: the six tensor starts of a packed planned gather (dn_packed_table_kernel)
    // the last gs_tsdf_mesh_plan (tsdf.hip): what gs_tsdf_mesh_emit must be called with, and the counts it writes (ws null: none)
    struct {
        const void* ws = nullptr;
        gs_tsdf_grid grid = {};
        float minWeight = 0.0f;
        long long V = 0, F = 0;
    } tsdfPlan;
    // counters
    uint32_t* counters = nullptr;  // device [GS_CNT_COUNT]
    uint32_t* countersHost = nullptr;  // pinned host mirror

    // results of the last binning
    const uint32_t* sortedIdx = nullptr;  // plain Gaussian indices (valid when sortedPlainValid)
    const uint32_t* sortedRaw = nullptr;  // what the sort produced: packed (tile << idxBits | index) or plain
    uint32_t idxMask = 0xFFFFFFFFu;
    int idxBits = 0;
    bool sortedPlainValid = false;
    bool binValid = false;
    int binN = 0;

    // stage profiling (HIP events on the ctx stream)
    struct ProfEvent { hipEvent_t a, b; int stage; bool extra; };
    unsigned profMask = 0;
    std::vector<ProfEvent> profPool;   // created lazily, reused
    size_t profUsed = 0;

    // saved fused-forward state
    struct {
        bool valid = false;
        bool blendBackwardDone = false;   // between gs_render_backward_dp_begin and _finish
        bool consumed = false;            // gs_render_backward_adam has overwritten the parameters: no further backward
        uint32_t* blockWork = nullptr;    // the buffer the forward measured into
        int N = 0, K = 0;
        const float *xyz = nullptr, *fdc = nullptr, *frest = nullptr, *scales = nullptr, *rot = nullptr,
                    *opacity = nullptr;
        const float *outColor = nullptr, *outDepth = nullptr, *outAlpha = nullptr;
        gs::CamParams cam;
        GsRenderModes modes;               // what this forward ran under: its backward's pose correction, anti-aliasing, camera
                                           // model, SH degree, background and 3-D filter
        const float* radii = nullptr;      // where this forward's projection wrote its radii (nullptr: nowhere)
        uint32_t* cutStore = nullptr;  // the view's cut words at the time of this forward (nullptr: none kept)
        bool cutsActive = false;     // this forward binned under depth cuts
        bool missChecked = true;     // ... and gs_forward_missed has been asked since
        bool bwdPrepared = false;    // the loss kernel has built the backward's item list and cleared its accumulator
        int preparedN = 0;
        int statePlanes = 5;         // planes per checkpoint slot this forward wrote (5 with the depth sum, 4 without)
        uint32_t qslotCap = 0;       // ... and how many such slots the arena held for it
        uint32_t qslotStatic = 0;    // ... of which handed to the waves up front (the shared counter starts behind them)
        bool arenaOverflow = false;  // the host has been told that this forward ran out of checkpoint slots: no backward
        bool missed = false;         // ... and the answer was yes: its outputs are not final, no backward from it
    } fwd;
};

#define GS_HIP_CHECK(ctx, expr)                                                              \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                  \
            return GS_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

// ---- the context's memory: every device and pinned buffer of gs_ctx and GsDp goes through these (gs_mem.h keeps the record,
// gs_workspace_bytes reports its device bytes, gs_ctx_destroy frees what is left) ------------------------------------------
const GsMemBackend* gs_hip_mem_backend();      // api.hip: hipMalloc / hipFree / hipHostMalloc / hipHostFree

static inline int ctx_mem_error(gs_ctx* c, const char* expr, int e)
{
    c->err = std::string(expr) + ": " + hipGetErrorString((hipError_t)e);
    return GS_ERR_HIP;
}
// count elements of device memory (a count of 0 allocates 1); GS_ERR_HIP with the failing expression in c->err
template <class T>
int ctx_alloc(gs_ctx* c, T** p, size_t count)
{
    if (count == 0) count = 1;
    const int e = c->mem.alloc((void**)p, count * sizeof(T));
    return e ? ctx_mem_error(c, "hipMalloc((void**)p, count * sizeof(T))", e) : GS_OK;
}
// ... of pinned host memory: recorded and freed with the context, not counted in gs_workspace_bytes
template <class T>
int ctx_alloc_pinned(gs_ctx* c, T** p, size_t count, unsigned flags = hipHostMallocDefault)
{
    const int e = c->mem.alloc((void**)p, count * sizeof(T), true, flags);
    return e ? ctx_mem_error(c, "hipHostMalloc((void**)p, count * sizeof(T), flags)", e) : GS_OK;
}
// forgets, frees and nulls p (device or pinned).  A pointer the context does not own is left alone and reported
template <class T>
void ctx_free(gs_ctx* c, T*& p)
{
    if (!c->mem.free((void*)p)) {
        c->err = "ctx_free: a pointer the context does not own";
        fprintf(stderr, "gsplat: %s (%p)\n", c->err.c_str(), (void*)p);
        return;
    }
    p = nullptr;
}
// grow on demand (GsMem::grow): nothing while want <= *cap; otherwise waits for the context's stream if the buffer exists,
// frees it, and allocates `want` units of `per` elements each.  *cap is 0 while *p is null
template <class T, class Cap>
int ctx_grow(gs_ctx* c, T** p, Cap* cap, long long want, size_t per = 1)
{
    const char* expr = "hipMalloc((void**)p, count * sizeof(T))";
    const int e = c->mem.grow((void**)p, cap, want, per * sizeof(T), [&] {
        const hipError_t w = hipStreamSynchronize(c->stream);
        if (w != hipSuccess) expr = "hipStreamSynchronize(c->stream)";
        return (int)w;
    });
    return e ? ctx_mem_error(c, expr, e) : GS_OK;
}
// two buffers that one capacity describes: both hold `want` afterwards, or neither exists
template <class A, class B, class Cap>
int ctx_grow_pair(gs_ctx* c, A** a, B** b, Cap* cap, long long want)
{
    Cap capB = *cap;
    int rc = ctx_grow(c, a, cap, want);
    if (rc == GS_OK) rc = ctx_grow(c, b, &capB, want);
    if (rc) { ctx_free(c, *a); ctx_free(c, *b); *cap = 0; }
    return rc;
}

static inline int gs_div_up(long long a, long long b) { return (int)((a + b - 1) / b); }
// does the depth sort of n records take the splitter buckets or the two-launch passes (binning.hip, depth_sort)?
static inline bool gs_small_depth_sort(long long n) { return gs_div_up(n, GS_SORT_THREADS * GS_SMALL_SORT_ITEMS) <= GS_SMALL_SORT_BLOCKS; }

// RAII stage timer: records a start/stop event pair around a launch sequence when profiling is on
struct GsStageTimer {
    gs_ctx* c;
    int slot = -1;
    // extra: time that belongs to a stage another timer of the same call already counts (its `calls` stay one per call)
    GsStageTimer(gs_ctx* ctx, int stage, bool extra = false) : c(ctx)
    {
        if (!((c->profMask >> stage) & 1u)) return;
        if (c->profUsed == c->profPool.size()) {
            if (c->profPool.size() >= 16384) return;
            gs_ctx::ProfEvent e;
            if (hipEventCreate(&e.a) != hipSuccess) return;
            if (hipEventCreate(&e.b) != hipSuccess) { (void)hipEventDestroy(e.a); return; }
            c->profPool.push_back(e);
        }
        slot = (int)c->profUsed++;
        c->profPool[slot].stage = stage;
        c->profPool[slot].extra = extra;
        (void)hipEventRecord(c->profPool[slot].a, c->stream);
    }
    ~GsStageTimer()
    {
        if (slot >= 0) (void)hipEventRecord(c->profPool[slot].b, c->stream);
    }
};

// ---- internal launchers (defined in the .hip files) -------------------------
namespace gs {

// api.hip: the refusal that api.hip and dp.hip share (host code).  GS_ERR_INVALID_ARG with the message of the first of `unserved`
// that is in force -- set now or, for pose, filter and fisheye, what the last forward ran with; `who` is the entry point's name, in
// front of the message
enum GsMode { GS_MODE_POSE, GS_MODE_FILTER3D, GS_MODE_FISHEYE, GS_MODE_ABSGRAD, GS_MODE_SPARSE_ADAM, GS_MODE_ADC_STATS,
              GS_MODE_DISTORTION };
int refuse_modes(gs_ctx* c, const char* who, std::initializer_list<GsMode> unserved);
int forward_in_arena(gs_ctx* c, const char* who, const float* params_base, long long n_arena);      // the forward's six tensors

CamParams make_cam(const gs_camera* cam, int W, int H);

// projection.hip
int launch_projection_forward(gs_ctx* c, int N, int K, const float* scales, const float* rot, const float* means3d,
                              const float* shs, const CamParams& cam, float* means2d, float* depths, float* color,
                              float* cov2d, float* conic, float* radii, float* rectMin, float* rectMax);
int launch_projection_backward(gs_ctx* c, int N, int K, const float* scales, const float* rot, const float* means3d,
                               const float* shs, const CamParams& cam, const float* cotDepths,
                               const float* cotMeans2d, const float* cotCov2d, const float* cotColor,
                               const float* cotConic, float* gScales, float* gRot, float* gMeans, float* gShs,
                               float* gCam);
int launch_projection_fused_forward(gs_ctx* c, int N, int K, const float* xyz, const float* fdc, const float* frest,
                                    const float* scales, const float* rot, const float* opacity,
                                    const CamParams& cam, float* radii);
// (the backwards of the context's forward: its tensors, camera and settings are c->fwd's)
int launch_projection_fused_backward(gs_ctx* c, float* gXyz, float* gFdc, float* gFrest, float* gScales, float* gRot, float* gOpacity,
                                     bool emitColorCot = false);
int launch_projection_fused_backward_adam(gs_ctx* c, const float* pBase, float* mBase, float* vBase, const float lr[6], float b1,
                                          float b2, float eps, float gscale);
int launch_vis_mask(gs_ctx* c, int N, const float* radii);      // sparse Adam: radii > 0 -> c->visMask
bool depth_sort_takes_splitters(const gs_ctx* c, int N);      // binning.hip
int launch_pose_camera(gs_ctx* c, const gs::CamParams& host, const float* delta);   // projection.hip, pose refinement
int launch_pose_grad(gs_ctx* c, int N);
long long pose_partials_floats(int N);
int launch_exposure_apply(gs_ctx* c, long long n, const float* M, const float* in, float* out);      // exposure.hip
int launch_exposure_backward(gs_ctx* c, long long n, const float* M, const float* render, float* cot, double* partials,
                             float* grad);
long long exposure_partials_doubles();
bool bilateral_shape_ok(int gw, int gh, int gl);       // bilateral_grid.hip
int bilateral_chunks(int W, int H, int gw, int gh);
long long bilateral_partials_floats(int gw, int gh, int gl, int nch);
int launch_bilateral_apply(gs_ctx* c, int W, int H, const float* G, int gw, int gh, int gl, const float* in, float* out);
int launch_bilateral_backward(gs_ctx* c, int W, int H, const float* G, int gw, int gh, int gl, int nch, float tvWeight,
                              const float* render, float* cot, float* partials, float* grad);
int launch_composite_target(gs_ctx* c, long long n, const float* rgb, const float* alpha, const float bg[3], float* out);   // background.hip
long long depth_loss_ws_doubles();      // depth_loss.hip
int launch_depth_loss(gs_ctx* c, int mode, float lambda, float alphaMin, float scale, float offset, const float* depth,
                      const float* alpha, const float* target, const unsigned char* mask, float* loss, float* cotDepth,
                      float* cotAlpha);
int launch_depth_normalize(gs_ctx* c, long long n, const float* depth, const float* alpha, float alphaMin, float* out);
long long normal_loss_ws_floats(long long np);      // normal_loss.hip
long long normal_loss_ws_doubles();
int launch_depth_normals(gs_ctx* c, const gs_normal_loss_params& s, const float* depth, const float* alpha, float* out);
int launch_normal_loss(gs_ctx* c, const gs_normal_loss_params& s, const float* depth, const float* alpha, const float* target,
                       const unsigned char* mask, const float* edge, float* loss, float* normalOut, float* cotDepth,
                       float* cotAlpha, float* ws, double* partials);
long long metrics_ws_doubles(int H, int W);      // metrics.hip
int launch_image_metrics(gs_ctx* c, int H, int W, const float* render, const float* target, const unsigned char* mask, double* out);
int launch_colour_moments(gs_ctx* c, long long n, const float* render, const float* target, const unsigned char* mask, double* out);
// filter3d.hip: the camera table's row is view[0..3][0], view[0..3][1], view[0..3][2], limX, limY, focalX, 0
int launch_filter3d_width(gs_ctx* c, int N, const float* xyz, float* filter);
int launch_filter3d_bake(gs_ctx* c, int N, const float* scalesRaw, const float* opacityRaw, const float* filter, float* outScales,
                         float* outOpacity);
int launch_undistort(gs_ctx* c, const gs_lens& lens, int srcW, int srcH, int dstW, int dstH, int channels, int mode, const void* src,
                     void* dst, unsigned char* valid);
int launch_undistort_fisheye(gs_ctx* c, const gs_fisheye_lens& lens, int srcW, int srcH, int dstW, int dstH, int channels, int mode, const void* src,
                     void* dst, unsigned char* valid);      // lens.hip
int launch_colour_rest(gs_ctx* c);      // gs_rider.h: the colour units the binning kernels have not taken along
int launch_color_cot(gs_ctx* c, int N, float* out);
int launch_sh_grad_from_views(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll,
                              const float* camCentersHost, float* gFdc, float* gFrest);
int launch_sh_grad_from_views_adam(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll,
                                   const float* camCentersHost, const float* fdcParam, const float* frestParam,
                                   const float* pBase, float* mBase, float* vBase, float lrDc, float lrRest, float b1,
                                   float b2, float eps, float gscale);
int launch_projection_geom_backward(gs_ctx* c, float* gXyz, float* gScales, float* gRot, float* gOpacity, float* xyzOwn,
                                    float* colorCot = nullptr);
int launch_sh_views_dir_adam(gs_ctx* c, int N, int K, int R, const float* xyz, const float* mgAll, const float* camCentersHost,
                             const float* const* ownXyzHost, const float* fdcParam, const float* frestParam, const float* pBase,
                             float* mBase, float* vBase, float lrDc, float lrRest, float b1, float b2, float eps, float gscale,
                             float* xyzAdd);
int launch_pack11_to_12(gs_ctx* c, int N, const float* packed11);
int launch_pack_gaussians(gs_ctx* c, int N, const float* means2d, const float* conic, const float* color,
                          const float* opacity, const float* depths, float* packed11);

// binning.hip
int launch_bin_prep(gs_ctx* c, int N, const float* rectMin, const float* rectMax, const float* radii,
                    const float* depths);
int launch_binning(gs_ctx* c, int N, bool wantPlain);  // depth sort, scan, expand, tile sort, ranges
int ensure_plain_sorted(gs_ctx* c);
int launch_tile_counts(gs_ctx* c);
int launch_cut_super(gs_ctx* c, const uint32_t* cuts);   // the view's cuts reduced to the deepest cut of every 4 x 4 tiles (c->superCut)
int cut_super_width(const gs_ctx* c);
int launch_build_packed_tile_indices(gs_ctx* c, uint32_t B, int32_t* out);

// blend.hip
int launch_blend_forward(gs_ctx* c, const GsBackground& bg, float* outColor, float* outDepth, float* outAlpha, uint32_t* lastContrib);
int launch_blend_backward(gs_ctx* c, const GsBackground& bg, int N, const float* cotColor, const float* cotDepth, const float* cotAlpha,
                          const float* outAlpha, const uint32_t* lastContrib);
int launch_gradacc_to_packed11(gs_ctx* c, int N, float* gradPacked11);

// contrib.hip: per-Gaussian blend weight scores over the lists of the last binning (either output may be null), and the prune
// decision on a score
int launch_blend_contrib(gs_ctx* c, float* maxW, float* sumW);
int launch_contrib_actions(gs_ctx* c, int N, const float* score, float threshold, int* actions, int* outputCounts);

// features.hip: C-channel feature images over the lists of the last binning (out [H, W, C] fully written) and their gradient
// with respect to the features (grad [N, C] accumulates); the channels a sweep of the list carries
int launch_blend_features(gs_ctx* c, int C, const float* features, float* out);
int launch_blend_features_backward(gs_ctx* c, int C, const float* cot, float* grad);
int feature_channel_group();

// distortion.hip: the depth distortion image D [H, W] and the pixels' totals (A, mu, S) [H, W, 3] over the lists of the last
// binning (both fully written), their gradient into rows of 16 floats in gradAcc16's column order (accumulates), and the
// term's loss sum and cotangent image
int launch_blend_distortion(gs_ctx* c, const gs_distortion_params& p, float* outDistort, float* outTotals);
int launch_blend_distortion_backward(gs_ctx* c, const gs_distortion_params& p, const float* cot, const float* totals, float* rows16);
long long distortion_loss_ws_doubles();
int launch_distortion_loss(gs_ctx* c, float weight, long long n, const float* distort, const unsigned char* mask, float* loss,
                           float* cotOut);

// blend_v2.hip (fused fast path)
int launch_blend_forward_v2(gs_ctx* c, float* outColor, float* outDepth, float* outAlpha);
int launch_blend_backward_v2(gs_ctx* c, int N, const float* cotColor, const float* cotDepth, const float* cotAlpha,
                             const float* outColor, const float* outDepth, const float* outAlpha, bool absgrad = false);
bool blend_forward_v2_pair_decide(const gs_ctx* c);

// ssim.hip
int launch_ssim_forward(gs_ctx* c, int H, int W, int C, int K, const float* img1, const float* img2,
                        const float* window, float* ssim, float* mu1, float* mu2, float* s1, float* s2, float* s12);
int launch_ssim_backward(gs_ctx* c, int H, int W, int C, int K, const float* gradOut, float gradOutConst,
                         const float* img1, const float* img2, const float* window, const float* mu1,
                         const float* mu2, const float* s1, const float* s2, const float* s12, float* g1, float* g2,
                         float l1Weight);
int launch_loss(gs_ctx* c, const float* render, const float* target, const float* renderDepth,
                const float* targetDepth, const unsigned char* depthMask, float lambdaDssim, float lambdaDepth,
                float* lossOut, float* cotColor, float* cotDepth);

// optim.hip
// densify.hip
int launch_accum_grad_norm(gs_ctx* c, int N, const float* xyzGrad, const float* accumIn, float* accumOut);
// AbsGS (gs_set_absgrad): accum += hypot(W/2 Ax, H/2 Ay) from the rows the blend backward left (gate: null or the overflow
// word), and (Ax, Ay) copied out
int launch_absgrad_accum(gs_ctx* c, int N, const uint32_t* gate, float* accum);
int launch_absgrad_copy(gs_ctx* c, int N, float* out);
int launch_classify(gs_ctx* c, int N, const float* gradAccum, float denom, const float* scales, int scaleStride,
                    const float* opacity, float gradThreshold, float maxScale, float minOpacity, int allowDensify,
                    int* actions, int* outputCounts);
int launch_densify_offsets(gs_ctx* c, int N, const int* actions, const int* outputCounts, int* offsets,
                           long long stats[5]);
int launch_build_densify_map(gs_ctx* c, int N, const int* actions, const int* offsets, int total, int* gather,
                             int* noiseMode);
int launch_densify_gather(gs_ctx* c, int total, int K, const float* xyz, const float* fdc, const float* frest,
                          const float* scales, const float* rot, const float* opacity, const int* gather,
                          const int* noiseMode, const float* baseNoise, float* oXyz, float* oFdc, float* oFrest,
                          float* oScales, float* oRot, float* oOpacity);
int launch_densify_plan(gs_ctx* c, int N, const int* actions, const int* outputCounts, int* offsets);
int densify_plan_read(gs_ctx* c, int wait, long long stats[8], int* ready);
int launch_build_densify_map_planned(gs_ctx* c, int N, const int* actions, const int* offsets, int cap, int* gather, int* noiseMode);
int launch_densify_gather_planned(gs_ctx* c, int cap, int K, const float* xyz, const float* fdc, const float* frest,
                                  const float* scales, const float* rot, const float* opacity, const int* gather,
                                  const int* noiseMode, unsigned long long noiseSeed, float* oXyz, float* oFdc, float* oFrest,
                                  float* oScales, float* oRot, float* oOpacity);
int launch_densify_gather_planned_packed(gs_ctx* c, int cap, int K, const float* xyz, const float* fdc, const float* frest,
                                         const float* scales, const float* rot, const float* opacity, const int* gather,
                                         const int* noiseMode, unsigned long long noiseSeed, float* outBase, const int order[6]);
int launch_densify_noise(gs_ctx* c, unsigned long long seed, int rows, float* out);
// out[j, :] = in[gather[j], :] for rows of L floats (plan / table: the planned and the packed forms, nullptr without)
void launch_gather_rows(gs_ctx* c, long long rows, int L, const float* in, const int* gather, float* out, const uint32_t* plan,
                        float* const* table = nullptr);
// adc.hip (include/gsplat.h gs_set_adc_stats and the gs_adc_* entry points; arguments checked by api.hip)
int launch_adc_accum(gs_ctx* c, int N, const float* rows16, const float* radii, bool useAbs, const uint32_t* gate, float* gradSum,
                     float* count, float* maxRadius);
int launch_adc_classify(gs_ctx* c, int N, const float* gradSum, const float* count, const float* maxRadius, const float* scales,
                        int scaleStride, const float* opacity, float gradThreshold, float denseMax, float minOpacity,
                        float maxScreenSize, float worldMax, int allowDensify, int sizePrune, int* actions, int* outputCounts);
int launch_adc_gather(gs_ctx* c, int total, int K, const float* xyz, const float* fdc, const float* frest, const float* scales,
                      const float* rot, const float* opacity, const int* gather, const int* noiseMode, const float* noise,
                      int revisedOpacity, float* oXyz, float* oFdc, float* oFrest, float* oScales, float* oRot, float* oOpacity);
int launch_adc_gather_moments(gs_ctx* c, int total, int K, const int* gather, const int* noiseMode, const int* actions,
                              const float* const in[6], float* const out[6]);
int launch_adc_reset_opacity(gs_ctx* c, int N, float* opacity, float* m, float* v, float resetRaw);
// mcmc.hip (include/gsplat.h gs_set_mcmc and the gs_mcmc_* entry points; arguments checked by api.hip)
struct McmcRows {            // the six tensors of rows [0, capacity) and where their moments lie
    float* t[6];             // xyz, f_dc, f_rest, scales, rotation, opacity
    const float* pBase;
    float* mBase;
    float* vBase;
};
int launch_mcmc_regularizer(gs_ctx* c, int N, const float* scales, const float* opacity, float* gScales, float* gOpacity,
                            const gs_mcmc_params& p);
int launch_mcmc_noise(gs_ctx* c, int N, float* xyz, const float* scales, const float* rot, const float* opacity, float lrXyz,
                      const gs_mcmc_params& p);
int launch_mcmc_random(gs_ctx* c, unsigned long long seed, int iteration, int stream, int n, uint32_t* words, float* normals,
                       double* uniforms);
int mcmc_relocate(gs_ctx* c, int N, int K, const McmcRows& rows, const gs_mcmc_params& p, long long stats[4]);
int mcmc_grow(gs_ctx* c, int N, int capacity, int K, const McmcRows& rows, const gs_mcmc_params& p, int* nOut);
// knn.hip
int launch_dist_topk(gs_ctx* c, int N, int k, int qBegin, int qCount, const float* xyz, float* out);
// ply.hip
int launch_ply_pack(gs_ctx* c, int N, int K, const float* xyz, const float* fdc, const float* frest,
                    const float* opacity, const float* scales, const float* rot, float* rows);
int ply_write_file(gs_ctx* c, const char* path, int N, int K, const float* xyz, const float* fdc, const float* frest,
                   const float* opacity, const float* scales, const float* rot);
int ply_probe_file(gs_ctx* c, const char* path, long long* N, int* M, int* D);
int ply_load_file(gs_ctx* c, const char* path, int N, int K, float* xyz, float* fdc, float* frest, float* opacity,
                  float* scales, float* rot);
int launch_adam(gs_ctx* c, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                const long long* segEnd, const float* segLr, float b1, float b2, float eps, float gradScale,
                const float* add = nullptr, long long addN = 0);
// gs_adam_step_visible: the same update on the rows below N whose mask byte is set (segment s holds rows of rowFloats[s] floats)
int launch_adam_visible(gs_ctx* c, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                        const long long* segEnd, const float* segLr, const int* rowFloats, float b1, float b2, float eps,
                        float gradScale, int N, const unsigned char* visible);

}  // namespace gs
