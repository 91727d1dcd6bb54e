/*
 * gsplat.h -- C ABI of the MI355X-native 3D-Gaussian-Splatting render/backward path.
 *
 * Drop-in boundary for the reference's Trainer render/backward path: every entry
 * point replaces one MLX CustomFunction / MLXFastKernel launch site of the
 * reference (file:line cited per function, relative to the reference repo).
 * A Swift (or any FFI) host keeps the GaussianRenderer / GaussianTrainer API and
 * calls these instead of MLXFast.metalKernel; see INTEGRATION.md.
 *
 * Conventions
 *  - All array arguments are DEVICE pointers (hipMalloc'd, or any framework's
 *    device buffer) to dense row-major f32 / u32 / i32 data, unless marked HOST.
 *  - The caller owns every input/output buffer.  The library owns only the
 *    context workspace (sort scratch, tile lists, saved forward state) and never
 *    frees caller memory.
 *  - Every call is asynchronous on the context's HIP stream; only the functions
 *    marked [sync] wait for the device.
 *  - A context is bound to one device + stream, is not thread-safe, and holds
 *    ONE forward in flight (like the reference's saved-state closures,
 *    GaussianRenderer.swift:119-122): a backward follows its forward on the same ctx.
 *  - Return value: 0 = GS_OK, otherwise a gs_status; gs_last_error() gives text.
 *    Nothing aborts, nothing throws across the ABI (the reference fatalError()s,
 *    GaussianRenderer.swift:264, 721-733, 808, 814).
 */
#ifndef GSPLAT_H
#define GSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSPLAT_ABI_VERSION 6

typedef enum gs_status {
    GS_OK = 0,
    GS_ERR_INVALID_ARG = 1,        /* null pointer, negative size, bad degree ... */
    GS_ERR_SIZE_MISMATCH = 2,      /* image size / N / K differs from what the ctx or the saved forward holds */
    GS_ERR_WORKSPACE_OVERFLOW = 3, /* tile-splat pairs exceeded the reserved capacity (see gs_ctx_reserve, "Overflow") */
    GS_ERR_HIP = 4,                /* a HIP runtime call failed */
    GS_ERR_NO_FORWARD = 5,         /* backward / tile query without a matching forward on this ctx */
    GS_ERR_NO_DEVICE = 6,          /* no usable GPU */
    GS_ERR_IO = 7,                 /* snapshot file missing, unwritable, truncated or malformed */
    GS_ERR_COMM = 8,               /* RCCL could not be loaded, or a communicator / collective call failed (gs_dp_*) */
    GS_ERR_REPLICA_MISMATCH = 9    /* gs_dp_check_replicas: the ranks do not hold the same model (every rank gets this code) */
} gs_status;

typedef struct gs_ctx gs_ctx;

/* HOST struct: one view.  Same numbers the reference feeds its projection kernel
 * (Trainer/CameraUtil.swift:5-102; GaussianRenderer.swift:852-857):
 * view = (c2w^-1)^T row-major so that p_view = [p,1].view; proj row-major, p_clip = p_view.proj. */
typedef struct gs_camera {
    float view[16];
    float proj[16];
    float cam_center[3];
    float fov_x, fov_y;     /* radians */
    float focal_x, focal_y; /* pixels */
} gs_camera;

/* ---- context ---------------------------------------------------------------------------------- */

/* Replaces GaussianRenderer.init(active_sh_degree:W:H:TILE_SIZE:whiteBackground:) (GaussianRenderer.swift:703-734).
 * Any tile size is served; what differs is how the FUSED entry points (gs_render_forward / _backward*) work inside:
 *   tile sizes that are multiples of 16 (16x16 is the fastest): tile lists as the reference builds them, swept by 16x16
 *     pixel blocks;
 *   any other tile size (the reference app's TILE_SIZE = (W/4, H/4), ColmapDataLoader.swift:495-498): BLOCK LISTS.  Every
 *     tile is cut into 16x16 pixel blocks (the last column / row of a tile narrower) and the fused path bins, sorts and
 *     blends per block: a block's list holds, in the reference's order, the Gaussians of its tile's list that can reach
 *     the block (weight exp(-q/2) >= 2^-29 somewhere on it -- the bound below which the fused kernels drop an entry anyway).
 *     Outputs are those of the reference's tile lists within the documented bars (image 1e-4, gradients 1e-3).  One
 *     consequence for a TRAINING run: a Gaussian that reaches no block of a tile at 2^-29 gets gradients
 *     below 1e-15 of the tensor's scale from the reference and exactly zero here, and the reference's Adam (eps = 1e-15, no bias
 *     correction) turns any non-zero gradient into a step of about the learning rate -- the reference random-walks such
 *     elements, this library leaves them where they are (measured, ten steps at 50x38 tiles: 0.4 % of the opacity / SH-rest
 *     elements more than 1e-3 apart, every loss within 2e-6).  What changes besides is what the fused path REPORTS about its lists: gs_last_stats' M and max list count (Gaussian, block) pairs,
 *     gs_copy_last_contrib / gs_copy_block_work / gs_block_count / the view-hint words refer to blocks and positions in block
 *     lists, and the tile queries (gs_tile_bin_info / _views / _export, gs_build_packed_tile_indices, gs_blend_forward /
 *     _backward) answer GS_ERR_NO_FORWARD after a fused forward until gs_tile_bin has run (they always describe the
 *     caller's tile grid).  View hints and depth cuts work as with 16x16 tiles.  The op-level entry points are unaffected.
 *     (Environment GSPLAT_BLOCK_LISTS=0 at context creation keeps the older form -- tile lists, every block scanning its
 *     tile's list with the generic kernels, no hints or cuts -- for A/B runs.) [sync] */
int gs_ctx_create(int device, int W, int H, int tile_w, int tile_h, int sh_degree, int white_bg, gs_ctx** out);
int gs_ctx_destroy(gs_ctx* ctx);
/* Bind to a caller stream (hipStream_t passed as void*).  NULL is the HIP default (null) stream, as in any
 * HIP call.  A new ctx starts on a private non-blocking stream of its own. [sync] */
int gs_ctx_set_stream(gs_ctx* ctx, void* hip_stream);
/* Pre-size the workspace so that no call allocates (and so no call synchronises) later.
 * max_pairs = capacity for M (sum of tiles touched).  0 keeps the current value. [sync]
 *
 * Overflow.  Without a reserve every forward checks M on the host and regrows the workspace (one wait per forward, as
 * the reference's .item() reads, GaussianRenderer.swift:399, 462).  With a reserve nothing waits, so a forward whose
 * pairs exceed max_pairs cannot fail at its own call: it renders the background only and raises a flag in host
 * memory.  From then on
 *   - on the device, every optimizer kernel of this ctx (gs_render_backward_adam, gs_adam_step,
 *     gs_sh_grad_from_views_adam) whose step belongs to that forward leaves parameters and moments untouched
 *     (see gs_set_update_gate), so no step is ever taken from a blank render;
 *   - on the host, the next gs_render_forward / gs_render_backward* / gs_loss_forward_backward / gs_adam_step /
 *     gs_forward_missed that sees the flag returns GS_ERR_WORKSPACE_OVERFLOW (gs_last_error names the M needed) and
 *     keeps returning it until gs_sync has reported it once or gs_ctx_reserve has been called again. */
int gs_ctx_reserve(gs_ctx* ctx, int max_gaussians, long long max_pairs);
/* Bytes of device workspace currently held: every device buffer the context owns, including the on-demand ones of the
 * densify, MCMC and data-parallel paths (pinned host memory is not counted). */
size_t gs_workspace_bytes(const gs_ctx* ctx);
/* Wait for the stream and report deferred errors (GS_ERR_WORKSPACE_OVERFLOW of any forward since the last report). [sync] */
int gs_sync(gs_ctx* ctx);
/* The overflow report that is waiting to be delivered, read WITHOUT waiting and WITHOUT clearing it (gs_sync delivers and
 * clears): out[0] = 0 none, 1 a forward needed more pairs than reserved, 2 a fused forward ran out of checkpoint slots;
 * out[1] = the pair count that forward needed (kind 1).  For hosts that must size a regrow from the forward that TRIPPED --
 * which need not be the last one (a data-parallel trainer looks only every 16th step) -- rather than from gs_last_stats.
 * Call it behind a wait for the stream; then gs_sync to take delivery.  (Replaces the reference's per-forward `.item()`
 * check of M, GaussianRenderer.swift:399.) */
int gs_overflow_pending(gs_ctx* ctx, uint32_t out[2] /*HOST*/);
/* Waits for everything queued on the ctx's stream -- the stream captured by gs_ctx_set_stream, which need not be the host
 * framework's current one -- and nothing else: reports nothing, clears nothing (gs_sync does both).  The wait to put in
 * front of gs_overflow_pending. [sync] */
int gs_wait(gs_ctx* ctx);
const char* gs_last_error(const gs_ctx* ctx);
int gs_abi_version(void);

/* ---- a3 / a4: projection ------------------------------------------------------------------------ */

/* gaussian_projection_screen_fused_forward (slang/gaussian_projection_kernels.slang:36-173; launch
 * GaussianRenderer.swift:542-561).  Inputs are ACTIVATED scales/rotations/opacity as in the reference.
 * Outputs: means2d[N,2] depths[N] color[N,3] cov2d[N,2,2] conic[N,2,2] radii[N] rectMin[N,2] rectMax[N,2]. */
int gs_projection_forward(gs_ctx* ctx, int N, int K, const float* scales, const float* rotations,
                          const float* means3d, const float* shs, const gs_camera* cam /*HOST*/,
                          float* means2d, float* depths, float* color, float* cov2d, float* conic,
                          float* radii, float* rect_min, float* rect_max);

/* gaussian_projection_screen_fused_backward (slang/gaussian_projection_kernels.slang:205-398; launch
 * GaussianRenderer.swift:654-675).  grad_shs[N,K,3] is fully written (zeros beyond (deg+1)^2).
 * grad_cam_center_point[N,3] is per point; the reference sums it on the host side (:683-684). */
int gs_projection_backward(gs_ctx* ctx, int N, int K, const float* scales, const float* rotations,
                           const float* means3d, const float* shs, const gs_camera* cam /*HOST*/,
                           const float* cot_depths, const float* cot_means2d, const float* cot_cov2d,
                           const float* cot_color, const float* cot_conic, float* grad_scales,
                           float* grad_rotations, float* grad_means3d, float* grad_shs,
                           float* grad_cam_center_point);

/* ---- a6: tile binning ---------------------------------------------------------------------------- */

/* buildGlobalTileSliceInfo (GaussianRenderer.swift:333-490) = count_tiles_per_gaussian, cumsum,
 * generate_keys, radix_sort_tile_keys_fused_forward, compute_tile_ranges,
 * compute_tile_counts_from_ranges (slang/gaussian_tile_global_kernels.slang:17-367).
 * Result (order: tile, depth bits, Gaussian index) stays in the ctx for gs_blend_*.  No host sync. */
int gs_tile_bin(gs_ctx* ctx, int N, const float* rect_min, const float* rect_max, const float* radii,
                const float* depths);
/* gs_tile_bin under per-tile DEPTH CUTS (the op-level form of what gs_set_view_hints does for the fused path): a pair
 * (Gaussian, tile) is binned only if the Gaussian's depth bits (the u32 pattern of its f32 depth, the reference's low
 * key word, slang/gaussian_tile_global_kernels.slang:73-126) do not exceed 0xFFFFFFFF - tile_cuts[tile];
 * tile_cuts[tile] == 0 means "no cut".  tile_cuts: DEVICE u32 [T], caller-owned, read during the call's kernels.
 * Lists are in key order, so every tile's list is a PREFIX of the list gs_tile_bin builds (ties at the cut are kept);
 * M / B / ranges / counts describe the cut lists.  NULL = gs_tile_bin. */
int gs_tile_bin_cut(gs_ctx* ctx, int N, const float* rect_min, const float* rect_max, const float* radii,
                    const float* depths, const uint32_t* tile_cuts);
/* M = total pairs, B = max pairs in any tile (the reference's two .item() reads, :399, :462). [sync] */
int gs_tile_bin_info(gs_ctx* ctx, uint32_t* M /*HOST*/, uint32_t* B /*HOST*/);
/* Device views owned by the ctx, valid until the next gs_tile_bin / gs_render_forward:
 * sorted_gauss_idx[M], tile_ranges[T,2], tile_counts[T]. */
int gs_tile_bin_views(gs_ctx* ctx, const uint32_t** sorted_gauss_idx, const uint32_t** tile_ranges,
                      const uint32_t** tile_counts);
/* Copies the same three arrays into caller buffers (device; any pointer may be NULL); sorted_gauss_idx
 * must hold M entries (gs_tile_bin_info). */
int gs_tile_bin_export(gs_ctx* ctx, uint32_t* sorted_gauss_idx, uint32_t* tile_ranges, uint32_t* tile_counts);
/* build_packed_tile_indices (slang/gaussian_tile_global_kernels.slang:377-404): the reference's dense
 * zero-padded i32 [T,B] table, for hosts that still want it.  out has T*B entries. */
int gs_build_packed_tile_indices(gs_ctx* ctx, uint32_t B, int32_t* out);

/* ---- a5, a7, a8: packing and alpha blending --------------------------------------------------------- */

/* buildPackedGaussians (GaussianRenderer.swift:85-99): [means2d(2), conic(4), color(3), opacity(1), depth(1)]. */
int gs_pack_gaussians(gs_ctx* ctx, int N, const float* means2d, const float* conic, const float* color,
                      const float* opacity, const float* depths, float* packed /*[N,11]*/);

/* gaussian_tile_global_forward (slang/gaussian_tile_global_kernels.slang:523-614; launch
 * GaussianRenderer.swift:130-141) over the ctx's current tile lists.
 * out_color[P,3] out_depth[P] out_alpha[P] last_contrib[P] (u32). */
int gs_blend_forward(gs_ctx* ctx, int N, const float* packed /*[N,11]*/, float* out_color, float* out_depth,
                     float* out_alpha, uint32_t* last_contrib);

/* gaussian_tile_global_backward (slang/gaussian_tile_global_kernels.slang:648-881; launch
 * GaussianRenderer.swift:208-218).  grad_packed[N,11] is fully written (zero where untouched). */
int gs_blend_backward(gs_ctx* ctx, int N, const float* packed, const float* cot_color, const float* cot_depth,
                      const float* cot_alpha, const float* out_color, const float* out_depth,
                      const float* out_alpha, const uint32_t* last_contrib, float* grad_packed);

/* Per-Gaussian blend weight scores (not in the reference): the quantity contribution-based pruning
 * (RadSplat's maximum, LightGaussian's / Mini-Splatting's sum) scores a Gaussian by.  For a pixel p and the j-th entry g of its
 * tile's depth-ordered list the blend computes, with T = 1 in front of the list (gs_blend_forward's arithmetic),
 *   raw = exp(-1/2 d^T conic d) opacity_g,  alpha = min(raw, 0.99),  w(p, g) = T alpha,  T <- T (1 - alpha),
 * and the pixel stops after the entry that brings T below 1e-4: later entries have w = 0.  Pixels outside the image do not
 * exist.  The scores of a view are
 *   max_w[g] = max over pixels of w(p, g),   sum_w[g] = sum over pixels of w(p, g),
 * 0 for a Gaussian in no list.  One pass over the tile lists of the last gs_tile_bin / gs_tile_bin_cut.  Both outputs
 * ACCUMULATE into caller-owned DEVICE buffers [N]: max_w becomes max(old, this view), sum_w gets this view added -- zero them
 * once, call once per view.  Either may be NULL, not both (GS_ERR_INVALID_ARG).  max_w is exact and the same bits on every
 * run (an integer maximum on the bit patterns of non-negative floats); sum_w is summed with float atomics.  Every tile size
 * gs_ctx_create accepts is supported (tiles larger than 16 x 16 sweep their list once per 16 x 16 block).  No sync, no
 * allocation. */
int gs_blend_contrib(gs_ctx* ctx, int N, const float* packed /*[N,11]*/, float* max_w /*DEVICE [N] or NULL*/,
                     float* sum_w /*DEVICE [N] or NULL*/);

/* N-channel per-Gaussian feature rendering (not in the reference): any per-Gaussian vector f[g, 0..C)
 * -- semantic or language features, identities, normals, albedo -- blended over the same splats with gs_blend_contrib's
 * weights w(p, g) = T alpha (its rule to the bit: clamp at 0.99, a pixel stops after the entry that brings T below 1e-4, no
 * background term, the background setting is not seen):
 *   forward    out[p, c]            = sum over the entries g of p's list of  w(p, g) features[g, c]
 *   backward   grad_features[g, c] += sum over the pixels p of               w(p, g) cot[p, c]
 * The geometry is frozen: there is no gradient into opacity, conic or mean.  One pass over the tile lists of the last
 * gs_tile_bin / gs_tile_bin_cut per group of gs_feature_channel_group() channels.  out DEVICE [H, W, C] is written at every
 * pixel (zeros where nothing blends; the caller does not clear) without atomics: the same bits on every run.  grad_features
 * DEVICE [N, C] ACCUMULATES with float atomics (zero it once, call once per view); rows of Gaussians in no list or behind every
 * pixel's stop are not touched.  cot must be finite.  1 <= C <= GS_MAX_FEATURE_CHANNELS, any C (rows need no alignment), else
 * GS_ERR_INVALID_ARG, as for a NULL buffer.  Preconditions and codes otherwise as gs_blend_contrib; every tile size gs_ctx_create
 * accepts is supported.  No sync, no allocation. */
#define GS_MAX_FEATURE_CHANNELS 256
int gs_blend_features(gs_ctx* ctx, int N, int C, const float* packed /*[N,11]*/, const float* features /*DEVICE [N,C]*/,
                      float* out /*DEVICE [H,W,C]*/);
int gs_blend_features_backward(gs_ctx* ctx, int N, int C, const float* packed /*[N,11]*/, const float* cot /*DEVICE [H,W,C]*/,
                               float* grad_features /*DEVICE [N,C], accumulates*/);
/* The number of channels one sweep of the lists carries (a build constant): C channels cost ceil(C / it) sweeps. */
int gs_feature_channel_group(void);

/* ---- a10: SSIM -------------------------------------------------------------------------------------- */

/* gaussian(windowSize:sigma:) outer product (LossUtil.swift:47-54, GaussianTrainer.swift:308-314);
 * writes K*K floats to HOST memory.  Off-centre on purpose (centre = K/2.0). */
int gs_ssim_window(int K, float sigma, float* window /*HOST [K*K]*/);
/* ssim_forward (slang/ssim_kernels.slang:94-155; launch GaussianTrainer.swift:584-590); images HWC. */
int gs_ssim_forward(gs_ctx* ctx, int H, int W, int C, int K, const float* img1, const float* img2,
                    const float* window /*device [K*K]*/, float* out_ssim, float* out_mu1, float* out_mu2,
                    float* out_sigma1, float* out_sigma2, float* out_sigma12);
/* ssim_backward (slang/ssim_kernels.slang:181-266; launch GaussianTrainer.swift:611-621). */
int gs_ssim_backward(gs_ctx* ctx, int H, int W, int C, int K, const float* grad_out, const float* img1,
                     const float* img2, const float* window, const float* mu1, const float* mu2,
                     const float* sigma1, const float* sigma2, const float* sigma12, float* grad_img1,
                     float* grad_img2);

/* ---- fused convenience path (what the trainer's lossFn does, GaussianTrainer.swift:652-716) ------- */

/* activations (a2, GaussianRenderer.swift:936-963) + projection + packing + binning + blend, from the six
 * RAW parameter tensors.  xyz[N,3] features_dc[N,1,3] features_rest[N,K-1,3] scales[N,3] rotation[N,4]
 * opacity[N].  Outputs render[H,W,3] depth[H,W] alpha[H,W]; radii[N] may be NULL.  out_depth may be NULL
 * too: a training step without a depth term reads no depth image, and the blend then carries no depth sum
 * (its backward accepts no cot_depth: GS_ERR_INVALID_ARG).  Saves the state gs_render_backward needs inside
 * the ctx.  No host sync when capacity was reserved.
 * Two deliberate deviations from the reference's arithmetic, both where the reference's own is 0 x inf: a
 * Gaussian that no pixel blended gets the exact zero gradient from gs_render_backward* (not J^T 0 evaluated term by term), and a
 * Gaussian whose 2-D covariance has no positive determinant in float32 (cancellation on a needle tens of thousands of pixels
 * long: a conic that is not positive definite) is invisible while it is so -- radius 0, no pairs, zero gradient.  The op-level
 * gs_projection_forward / _backward keep the 1:1 arithmetic. */
int gs_render_forward(gs_ctx* ctx, int N, int K, const float* xyz, const float* features_dc,
                      const float* features_rest, const float* scales, const float* rotation,
                      const float* opacity, const gs_camera* cam /*HOST*/, float* out_color, float* out_depth,
                      float* out_alpha, float* radii);

/* VJP of gs_render_forward w.r.t. the six raw tensors (blend backward, a5 split, projection backward,
 * activation VJPs).  cot_depth / cot_alpha may be NULL (= zeros, the default training case, a11).
 * The forward's inputs and outputs must still be alive and unchanged. */
int gs_render_backward(gs_ctx* ctx, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                       float* grad_xyz, float* grad_features_dc, float* grad_features_rest, float* grad_scales,
                       float* grad_rotation, float* grad_opacity);

/* gs_render_backward + gs_adam_step in one: the projection backward applies every element's Adam update in place
 * instead of writing a gradient arena for gs_adam_step to read back (same arithmetic; ~1/3 fewer bytes over the two
 * kernels).  The six tensors handed to the preceding gs_render_forward must lie inside [params_base, params_base +
 * n_arena); m_base / v_base are the moment arenas with the same layout.  lr HOST [6] in the reference's parameter
 * order xyz, f_dc, f_rest, scales, rotation, opacity (GaussianModel.swift:56-65).  Single-device steps only (with
 * several ranks the gradients have to be exchanged first).  Consumes the forward: a second backward needs a new
 * gs_render_forward. */
int gs_render_backward_adam(gs_ctx* ctx, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                            float* params_base, float* m_base, float* v_base, long long n_arena, const float lr[6],
                            float beta1, float beta2, float eps, float grad_scale);

/* gs_blend_contrib's scores of the last gs_render_forward's view, on that forward's own records and lists: the opacity of
 * an anti-aliased forward, of a 3-D filter and the camera of a pose correction are what it was composed with.  (The fused
 * forward bins trimmed rects, and may bin under depth cuts: entries of weight below 2^-29, or behind every pixel's stop, are
 * not in its lists -- a score moves by less than 1e-8.)  Accumulates into max_w / sum_w DEVICE [N of the forward] like
 * gs_blend_contrib.  Refuses what gs_render_backward would refuse, with the same codes: no valid forward (or one a
 * gs_render_backward_adam consumed), a forward reported missed, a forward that overflowed its reserved pairs, checkpoint-arena
 * overflow.  After a forward under depth cuts ask gs_forward_missed first, as for any other use of its outputs.  Consumes
 * nothing: a backward may still follow, the render outputs and gs_last_stats are untouched.  No sync, no allocation. */
int gs_render_contrib(gs_ctx* ctx, float* max_w /*DEVICE [N] or NULL*/, float* sum_w /*DEVICE [N] or NULL*/);

/* gs_blend_features / gs_blend_features_backward for the last gs_render_forward's view, on that forward's own records and
 * lists (its anti-aliased opacity, 3-D filter and pose correction included; trimmed rects and depth cuts as for
 * gs_render_contrib).  features / grad_features are DEVICE [N of the forward, C], out / cot DEVICE [H, W, C].  Refuse what
 * gs_render_contrib refuses, with the same codes; C outside [1, GS_MAX_FEATURE_CHANNELS] or a NULL buffer: GS_ERR_INVALID_ARG.
 * Consume nothing: a backward and further feature calls on the same forward may follow, the render outputs and gs_last_stats
 * are untouched.  No sync, no allocation. */
int gs_render_features(gs_ctx* ctx, int C, const float* features /*DEVICE [N,C]*/, float* out /*DEVICE [H,W,C]*/);
int gs_render_features_backward(gs_ctx* ctx, int C, const float* cot /*DEVICE [H,W,C]*/,
                                float* grad_features /*DEVICE [N,C], accumulates*/);

/* The depth distortion loss (not in the reference): 2DGS's eq. 13, gsplat's `distloss`, which GOF, PGSR
 * and RaDe-GS train with as well.  It pulls the blend weights of a ray together in depth.  Per pixel, over the entries i of its
 * list up to its stop, with gs_blend_contrib's weights w_i = T_i alpha_i (its rule to the bit: clamp at 0.99, the pixel stops
 * after the entry that brings T below 1e-4, no background) and the mapped depth m_i = map(z_i) of the record's depth (column 10):
 *   D = sum_{i<j} w_i w_j (m_i - m_j)^2 = A S,    A = sum w_i,  mu = sum w_i m_i / A,  S = sum w_i (m_i - mu)^2
 * -- 2DGS's convention: every unordered pair once, the weights not normalised.  (A, mu, S) are carried with the weighted Welford
 * update A' = A + w, mu' = mu + (w / A') (m - mu), S' = S + w (m - mu) (m - mu'), which cancels nothing on thin distributions
 * (A M2 - M1^2 and 2DGS's running prefix form both do, in float32); it runs on m - c, c the m of the pixel's first weighted
 * entry, so that the running mean is as small as the deviations (the reported mu is c + mu).  The derivatives by the totals,
 *   dD/dw_i = g_i = A (m_i - mu)^2 + S,   dD/dm_i = 2 w_i A (m_i - mu),   dD/dalpha_i = T_i g_i - R_i / (1 - alpha_i),
 *   R_i = sum_{j>i} g_j w_j = 2 D - sum_{j<=i} g_j w_j,
 * go from alpha_i into mean, conic and opacity with gs_blend_backward's derivatives and clamp rule (the clamp passes the gradient
 * iff raw <= 0.99, the floor of 1 - alpha is 1e-6) and from m_i into the record's depth through map'(z).
 *   GS_DISTORTION_NDC     m = far / (far - near) (1 - near / z)     2DGS's map; its defaults are near 0.2, far 1000
 *   GS_DISTORTION_LINEAR  m = z                                     gsplat's; near and far are not read
 * Forward: out_distort DEVICE [H, W] = D and out_totals DEVICE [H, W, 3] = (A, mu, S), the backward's input; every pixel is
 * written (zeros where nothing blends; the caller does not clear) without atomics: the same bits on every run.
 * Backward: cot DEVICE [H, W] is dL/dD (finite), totals what the forward wrote; rows16 DEVICE [N, 16] ACCUMULATES with float
 * atomics in the column order of the blend backward's accumulator,
 *   dmx dmy dc00 dc01 | dc10 dc11 dr dg | db dop ddepth . | . . . .
 * of which columns 0 .. 5, 9 and 10 are added to (dc10 = dc01); the colour columns and columns 11 .. 15 are not touched, nor
 * are rows of Gaussians in no list or behind every pixel's stop.  One pass over the tile lists of the last gs_tile_bin /
 * gs_tile_bin_cut each.  Preconditions and codes as gs_blend_contrib; GS_ERR_INVALID_ARG also for a NULL params or buffer, a map
 * out of range, or -- GS_DISTORTION_NDC -- near, far not finite or not 0 < near < far.  Every tile size gs_ctx_create accepts is
 * supported.  No sync, no allocation. */
enum { GS_DISTORTION_NDC = 0, GS_DISTORTION_LINEAR = 1 };
typedef struct gs_distortion_params {
    int map;
    float near, far;
} gs_distortion_params;
int gs_blend_distortion(gs_ctx* ctx, int N, const float* packed /*[N,11]*/, const gs_distortion_params* params /*HOST*/,
                        float* out_distort /*DEVICE [H,W]*/, float* out_totals /*DEVICE [H,W,3]*/);
int gs_blend_distortion_backward(gs_ctx* ctx, int N, const float* packed /*[N,11]*/, const gs_distortion_params* params /*HOST*/,
                                 const float* cot /*DEVICE [H,W]*/, const float* totals /*DEVICE [H,W,3]*/,
                                 float* rows16 /*DEVICE [N,16], accumulates*/);
/* gs_blend_distortion / gs_blend_distortion_backward (2DGS eq. 13 / gsplat distloss) for the last gs_render_forward's view, on
 * that forward's own records and lists (its anti-aliased opacity, 3-D filter and pose correction included; trimmed rects and
 * depth cuts as for gs_render_features).  rows16 is DEVICE [N of the forward, 16].  Refuse what gs_render_features refuses, with
 * the same codes.  Consume nothing: a backward and further calls on the same forward may follow, the render outputs and
 * gs_last_stats are untouched.  No sync, no allocation. */
int gs_render_distortion(gs_ctx* ctx, const gs_distortion_params* params /*HOST*/, float* out_distort /*DEVICE [H,W]*/,
                         float* out_totals /*DEVICE [H,W,3]*/);
int gs_render_distortion_backward(gs_ctx* ctx, const gs_distortion_params* params /*HOST*/, const float* cot /*DEVICE [H,W]*/,
                                  const float* totals /*DEVICE [H,W,3]*/, float* rows16 /*DEVICE [N,16], accumulates*/);
/* The distortion term of a step's loss (2DGS eq. 13 as a loss, gsplat's distloss().mean()):
 *   L = weight (1 / n_pixels) sum_p v_p D_p,    cot_out[p] = dL/dD_p = weight v_p / n_pixels,
 * v_p = (float)mask[p] / 255.0f as gs_set_loss_mask's weights (255 is exactly 1, 0 exactly 0; it is this call's own argument),
 * 1 with mask NULL; divided by all n_pixels, as the masked colour loss is.  loss[0] += L (read and written: the call is queued
 * behind the loss that wrote it).  Every element of cot_out is written.  Two launches, the sum in double over per-block
 * partials finished in a fixed order, no float atomics: two calls on the same inputs give the same bits.  The first call
 * allocates 4 KB of workspace, no later one allocates; no wait.  GS_ERR_INVALID_ARG: n_pixels < 0, a weight that is not finite,
 * a NULL distort, loss or cot_out; n_pixels == 0: nothing is launched. */
int gs_distortion_loss(gs_ctx* ctx, float weight, long long n_pixels, const float* distort /*DEVICE [n]*/,
                       const unsigned char* mask /*DEVICE [n] or NULL*/, float* loss /*DEVICE, accumulates into [0]*/,
                       float* cot_out /*DEVICE [n]*/);
/* Arms the distortion term (2DGS eq. 13 / gsplat distloss) for the current forward: the next gs_render_backward or
 * gs_render_backward_adam of it runs gs_render_distortion_backward(params, cot, totals) into the context's own accumulator rows,
 * directly behind the blend backward that fills them and in front of the ADC statistic (gs_set_adc_stats) and the projection
 * backward that read them -- the signed 2-D mean gradient ADC averages then includes the term, as gsplat's means2d.grad does.
 * Columns 12 and 13 of the rows (the AbsGS sums of gs_set_absgrad) stay the colour and depth terms' alone.  The depth column is
 * read by the projection backward of every forward, so the forward need not have rendered a depth image.  cot and totals are
 * DEVICE [H, W] and [H, W, 3], read when the backward runs.  params, cot and totals all NULL: disarms.  A new gs_render_forward
 * disarms too.  The gs_render_backward_dp* family refuses an armed context (GS_ERR_INVALID_ARG): single-device steps only.
 * Refuses what gs_render_features refuses, with the same codes; params as for gs_blend_distortion.  Launches nothing. */
int gs_arm_distortion(gs_ctx* ctx, const gs_distortion_params* params /*HOST*/, const float* cot /*DEVICE [H,W]*/,
                      const float* totals /*DEVICE [H,W,3]*/);

/* Per-view camera pose refinement (not in the reference; DESIGN.md "Pose refinement").  delta DEVICE [6] = (w, tau), float32,
 * a correction of the camera-to-world pose in the camera's own OpenCV frame (x right, y down, z forward):
 *   c2w' = c2w [[R(w), tau], [0, 1]],  R(w) Rodrigues' rotation (its series near w = 0: R(0) = I exactly),
 *   view' = inv(c2w')^T (row-major, as gs_camera.view),  cam_center' = c2w'[:3, 3];
 * proj, the fovs and the focals are unchanged.  While a correction is set, each gs_render_forward composes its camera on the
 * device from the host gs_camera and *delta (six zero words: the host camera bit for bit), and the gs_render_backward /
 * gs_render_backward_adam of that forward OVERWRITE grad_delta DEVICE [6] with dL/d delta: the exact chain rule at the current
 * delta through the means, the 2-D covariance, the depth cotangent and the SH view direction, summed in a fixed order (the same
 * bits on every run).  A Gaussian whose cotangent row is all zero contributes exactly 0.  The backward uses the correction its
 * forward was composed with.  delta and grad_delta are both set or both NULL; NULL (the default) is the behaviour without
 * pose refinement, kernel for kernel.  While a correction is set gs_render_backward_dp* and gs_dp_step return
 * GS_ERR_INVALID_ARG (single-device steps only).  The op-level entry points (gs_projection_*, gs_blend_*) take explicit
 * matrices and are not affected.  Optimise delta with gs_adam_step on its six floats: it is gated with the step's other
 * optimizer kernels. */
int gs_set_pose_correction(gs_ctx* ctx, const float* delta /*DEVICE [6] or NULL*/, float* grad_delta /*DEVICE [6] or NULL*/);

/* Per-view exposure compensation (not in the reference; DESIGN.md "Exposure compensation"): the photometric counterpart of pose
 * refinement, as Inria's 3DGS trains it per training image.  M DEVICE [12] float32 = [A | b], row-major 3 x 4:
 * M[4c + j] = A[c][j] (j < 3), M[4c + 3] = b[c]; the identity is A = I, b = 0.  Inria applies its exposure E as
 * img @ E[:3, :3] + E[:3, 3]: in this convention A = E[:3, :3]^T, b = E[:3, 3].  While an exposure is set, each
 * gs_loss_forward_backward takes the loss of the corrected image c_p = A r_p + b of the render r (no clamp), per channel
 *   c_p[c] = fmaf(A[c][0], r0, fmaf(A[c][1], r1, fmaf(A[c][2], r2, b[c]))),
 * writes dL/dr into cot_color,
 *   dL/dr_p[j] = fmaf(A[0][j], g0, fmaf(A[1][j], g1, A[2][j] * g2)),   g_p = dL/dc_p (the loss's own cotangent),
 * and OVERWRITES grad DEVICE [12] with dL/dM: dL/dA[c][j] = sum_p g_p[c] r_p[j], dL/db[c] = sum_p g_p[c], summed in float64
 * in a fixed order (the same bits on every run) and rounded to float32.  With the identity, the loss and cot_color are the
 * plain ones bit for bit.  The render is not written: the corrected image lives in a ctx-owned [H, W, 3] buffer, allocated at
 * the first non-NULL call (no step allocates), and cot_color must not alias the render.  The depth term, the target cache
 * (gs_set_loss_target_cache) and every render / backward entry point are unchanged; the op-level gs_ssim_* ignore the
 * setting.  A repeated forward is followed by a repeated loss, which writes grad again.  M and grad are both set or both NULL;
 * NULL (the default) issues the loss's launches exactly as without it.  Optimise M with gs_adam_step on its twelve floats: it
 * is gated with the step's other optimizer kernels. */
int gs_set_exposure(gs_ctx* ctx, const float* M /*DEVICE [12] or NULL*/, float* grad /*DEVICE [12] or NULL*/);
/* out[p] = A in[p] + b for n_pixels RGB pixels ([n_pixels, 3] float32, DEVICE), in gs_set_exposure's order of operations; out may
 * be in.  Shows or scores a training view under its learned exposure.  Asynchronous on the ctx stream. */
int gs_apply_exposure(gs_ctx* ctx, long long n_pixels, const float* M /*DEVICE [12]*/, const float* in, float* out);

/* Per-view bilateral grid colour correction (not in the reference; DESIGN.md "Bilateral grid"; Wang et al. 2024, "Bilateral
 * Guided Radiance Field Processing", gsplat's use_bilateral_grid): exposure compensation whose M varies over the image and with
 * the render's luminance.  grid DEVICE float32 of grid_h x grid_w x grid_l nodes, G[y][x][z][k] row-major with the node's
 * 12 coefficients innermost, each an M in gs_set_exposure's convention (m[4c + j] = A[c][j], m[4c + 3] = b[c]); at the
 * default shape (16, 16, 8) 98,304 bytes.  2 <= grid_w, grid_h <= 64, 2 <= grid_l <= 32.  Pixel (x, y) of the W x H render r:
 *   u = (float)((2x + 1)(grid_w - 1)) / (float)(2W),  v likewise with y, grid_h, H  (one correctly rounded division),
 *   gray = fmaf(0.299f, r0, fmaf(0.587f, r1, 0.114f * r2)),  w = min(max(gray, 0), 1) * (grid_l - 1),
 *   x0 = min((int)u, grid_w - 2), fu = u - x0;  y0, fv and z0, fw likewise,
 *   a[k] = lerp over z of (lerp over y of (lerp over x)), lerp(a, b, t) = fmaf(t, b - a, a),
 * and the loss is taken of c[c] = fmaf(a[4c], r0, fmaf(a[4c+1], r1, fmaf(a[4c+2], r2, a[4c+3]))) (no clamp), so a grid whose
 * nodes all hold M gives gs_set_exposure(M)'s loss and cot_color bit for bit.  With g = dL/dc (the loss's own cotangent),
 * P_hi / P_lo the bilinear values at layers z0 + 1 / z0 and da[4c + j] = g[c] r[j], da[4c + 3] = g[c]:
 *   s = sum_k (P_hi[k] - P_lo[k]) da[k],  dgray = s (grid_l - 1) if 0 < gray < 1, else 0,
 *   dL/dr[j] = fmaf(dgray, lum[j], fmaf(a[j], g0, fmaf(a[4 + j], g1, a[8 + j] * g2))),  lum = (0.299f, 0.587f, 0.114f),
 * written into cot_color, and grad (the grid's shape) is OVERWRITTEN with dL/dG[node][k] = sum_p wt(p, node) da_p[k] +
 * tv_weight dTV/dG[node][k], wt the trilinear weight, TV(G) = sum over the axes x, y, z of (1 / n_axis) sum (G_next - G)^2 with
 * n_axis the number of (pair, k) terms on that axis (n_x = 12 grid_l grid_h (grid_w - 1)).  The sums run in a fixed order
 * over a launch grid fixed by the image size and the grid shape (the same bits on every run, no atomics).  The corrected image
 * lives in the ctx's exposure scratch image; the render is not written and cot_color must not alias it.  Everything else is as
 * for gs_set_exposure: the depth term, the target cache and every render / backward entry point are unchanged, a repeated
 * loss writes grad again, and gs_adam_step on the grid's floats is gated with the step's other optimizer kernels.  grid and
 * grad are both set or both NULL; NULL (the default) issues the loss's launches exactly as without it, and ignores the shape
 * and tv_weight.  tv_weight must be finite and >= 0.  A grid and an exposure are exclusive: while one is set, setting the
 * other returns GS_ERR_INVALID_ARG and leaves the state as it was.  The partials buffer is allocated or grown here only. */
int gs_set_bilateral_grid(gs_ctx* ctx, const float* grid /*DEVICE or NULL*/, float* grad /*DEVICE or NULL*/, int grid_w,
                          int grid_h, int grid_l, float tv_weight);
/* out = the W x H image in ([H, W, 3] float32, DEVICE) under the grid, in gs_set_bilateral_grid's order of operations; out may
 * be in.  Shows or scores a training view under its learned grid.  Asynchronous on the ctx stream. */
int gs_apply_bilateral_grid(gs_ctx* ctx, int W, int H, const float* grid /*DEVICE*/, int grid_w, int grid_h, int grid_l,
                            const float* in /*[H,W,3]*/, float* out /*[H,W,3], may be in*/);

/* Anti-aliased mode (not in the reference; DESIGN.md "Anti-aliased mode"): Mip-Splatting's 2-D filter, as Inria's rasterizer
 * (antialiasing) and gsplat (rasterize_mode="antialiased") offer it.  With Sigma a splat's projected 2-D covariance BEFORE the
 * reference's blur (J W Sigma3 W^T J^T) and Sigma_b = Sigma + 0.3 I the blurred one, each following gs_render_forward writes
 *   sigma(o) rho,  rho = sqrt(det Sigma / det Sigma_b)
 * as the packed opacity: the blur stays, and the splat's opacity shrinks by the share its footprint was inflated by.  Conic,
 * means, depth, colour, radius and rect are unchanged; colour, depth and alpha see only the compensated opacity.  det Sigma is
 * formed in float32 from the unblurred entries.  A splat whose det Sigma is not > 0 (or not finite) is invisible while it is so:
 * radius 0, no pairs, an exactly zero gradient (the fused path's GS_DEGENERATE_INVISIBLE convention; Inria's rasterizer
 * clamps the ratio at 2.5e-5 instead, which keeps such a splat faintly visible with the square root's derivative at its
 * singularity).  Backward, with c = dL/d(packed opacity): dL/do_raw = c rho sigma (1 - sigma), and the cotangent of Sigma_b
 * gains c sigma(o) (rho / 2) (Sigma^-T - Sigma_b^-T) in the four-independent-entries convention.  enable: 0 (the default, the
 * reference's semantics, kernel for kernel) or 1; any other value returns GS_ERR_INVALID_ARG and leaves the mode as it was.
 * The mode is the context's; a backward uses the mode its forward ran in.  It composes with every fused entry point:
 * gs_render_backward, gs_render_backward_adam, gs_render_backward_dp*, gs_dp_step, pose refinement, depth cuts and view hints,
 * trimmed rects and block lists (the lists are built from the geometry alone: M does not change).  All ranks of a
 * data-parallel job must agree on it (a rank that does not shows up as a replica mismatch).  The op-level entry points
 * (gs_projection_*, gs_pack_gaussians, gs_blend_*) keep the reference's arithmetic and ignore the mode.  PLY snapshots do not
 * record it: render a model in the mode it was trained in. */
int gs_set_antialiasing(gs_ctx* ctx, int enable);

/* Camera model (not in the reference; gsplat's camera_model="fisheye").  GS_CAMERA_PINHOLE (the default)
 * is the reference's perspective projection, kernel for kernel.  Under GS_CAMERA_FISHEYE every following gs_render_forward and
 * the op-level gs_projection_forward / gs_projection_backward project through the ideal equidistant model: a view-space point
 * (x, y, z) with r = sqrt(x^2 + y^2), theta = atan2(r, z) lands at
 *   means2d = (fx x theta / r + cx - 0.5,  fy y theta / r + cy - 0.5)        (r = 0: the principal point),
 * and the 2-D covariance is (J W) Sigma (J W)^T + 0.3 I with J the full 2 x 3 Jacobian of that map (no frustum clamp).  Depth
 * stays view z and visibility stays z >= 0.2, so the field of view is below 180 degrees.  Colour, radius, rect, conic, the
 * degenerate-determinant rule and the anti-aliased mode are what they are for a pinhole.
 * Read from the gs_camera: focal_x, focal_y (fx, fy), proj[8] and proj[9] (cx = (proj[8] + 1) W / 2, cy = (proj[9] + 1) H / 2,
 * the principal point as DESIGN.md section 23 places it), view, cam_center, and the context's W, H.  Not read: fov_x, fov_y and
 * the rest of proj.  The gs_camera's layout is unchanged.
 * A per-context setting as gs_set_antialiasing is: it allocates nothing and may be changed before every forward, so views of
 * both models can share a context; a fused backward (gs_render_backward, gs_render_backward_adam) uses the model its forward
 * ran in.  Any other value of model returns GS_ERR_INVALID_ARG and leaves the setting as it was.
 * Not served, each GS_ERR_INVALID_ARG with the reason in gs_last_error: a fisheye gs_render_forward while a pose correction
 * (gs_set_pose_correction) or a 3-D filter (gs_set_filter3d) is set; gs_render_backward_dp*, gs_dp_step and
 * gs_set_filter3d_cameras while the model is set or behind a forward made in it. */
#define GS_CAMERA_PINHOLE 0
#define GS_CAMERA_FISHEYE 1
int gs_set_camera_model(gs_ctx* ctx, int model);
int gs_get_camera_model(gs_ctx* ctx, int* model /*HOST*/);

/* Active SH degree (not in the reference, whose degree is fixed; Inria's oneupSHdegree, gsplat's
 * sh_degree_interval).  gs_ctx_create's sh_degree is the context's MAXIMUM and the default; the active degree d, 0 <= d <= maximum,
 * is what the following gs_render_forward calls evaluate: the bands k < (d + 1)^2 of a row of K coefficients, K only the row
 * stride.  A fused backward (gs_render_backward, gs_render_backward_adam, gs_render_backward_dp*) uses the degree its forward ran
 * with; gs_projection_forward / gs_projection_backward and gs_sh_grad_from_views* use the value at the time of the call, and every
 * "K smaller than (degree+1)^2" check is made against the active degree.  The gradient of a coefficient k >= (d + 1)^2 is an
 * exact 0.0.  Any other value returns GS_ERR_INVALID_ARG with the reason in gs_last_error and leaves the setting as it was.
 * A per-context setting as gs_set_antialiasing is: it allocates nothing and may be changed before every forward.  With the
 * setter never called every launch, argument and result is what it was without it.
 * gs_render_backward_adam below the degree K allows -- (d + 2)^2 <= K -- with no pose correction, MCMC step, 3-D filter or
 * sparse Adam set takes a band-limited form: the elements of features_rest in the columns >= 3 ((d + 1)^2 - 1) of a row keep
 * their bits in the parameter and both moment arenas, whatever they hold, and 16-byte words that hold no active column are
 * neither read nor written (at degree 0 no features_rest byte moves).  Every other form runs its full-row update, in which an
 * inactive element meets an exact zero gradient: zero moments stay zero and the parameter stays put (lr 0 / (sqrt(0) + eps) = 0),
 * while moments that are NOT zero decay and keep moving their parameter -- after lowering the degree by hand those forms and the
 * band-limited one differ on the inactive columns, and on nothing else. */
int gs_set_sh_degree(gs_ctx* ctx, int degree);
int gs_get_sh_degree(gs_ctx* ctx, int* degree /*HOST*/);

/* Background colour (not in the reference, which composites over black or white; Inria's
 * --random_background, gsplat's backgrounds=).  With a colour b set, every following blend forward writes, per pixel and channel,
 *   out_c = sums_c + T b_c        (T the final transmittance; alpha, depth and nContrib do not change),
 * and its backward takes cT = -cot_alpha + g . b as the transmittance's cotangent.  T b_c is one rounded float32 product.
 * rgb == NULL (the default) is the creation background (white_bg): images and gradients are then bit for bit what they are on a
 * context that never had a colour.  The three values must be finite and are not confined to [0, 1]; otherwise
 * GS_ERR_INVALID_ARG, and the previous setting stays.  The colour is a by-value kernel argument: the call allocates nothing,
 * waits for nothing and may be made before every step.  A per-context setting as gs_set_antialiasing is: it holds for the
 * forwards that follow, and a fused backward (gs_render_backward, gs_render_backward_adam, gs_render_backward_dp*) uses the
 * background of its gs_render_forward, whatever has been set since.  The op-level gs_blend_forward / gs_blend_backward keep no
 * forward of their own and read the setting in effect at the call.  gs_render_contrib / gs_blend_contrib do not see it: blend
 * weights carry no background.  Honoured on every path a forward can take (one-wave, pair and four-wave forwards, block lists,
 * the generic and cull kernels at every GS_TUNE_OP_*_PPL). */
int gs_set_background(gs_ctx* ctx, const float* rgb /*HOST [3] or NULL*/);
/* The colour in effect: the one set, or (1,1,1) / (0,0,0) for an unset context by its white_bg. */
int gs_get_background(gs_ctx* ctx, float rgb[3] /*HOST*/);
/* The training target of an RGBA view over bg: out_c = fmaf(a, rgb_c, (1 - a) bg_c) for n_pixels pixels, rgb straight
 * (un-premultiplied).  out may be rgb itself.  Asynchronous on the ctx stream, allocates nothing.  n_pixels < 0 or a NULL
 * pointer: GS_ERR_INVALID_ARG; n_pixels == 0: nothing is launched. */
int gs_composite_target(gs_ctx* ctx, long long n_pixels, const float* rgb /*DEVICE [n,3]*/, const float* alpha /*DEVICE [n]*/,
                        const float* bg /*HOST [3]*/, float* out /*DEVICE [n,3]*/);

/* AbsGS densification statistic (not in the reference; Ye et al. 2024, gsplat's absgrad=True).  The
 * gradient of the loss with respect to a splat's 2-D mean is a sum over the pixels it covers; on a large splat over fine detail
 * the pixels pull in opposite directions and the sum cancels ("gradient collision").  With absgrad on, the blend backward of
 * gs_render_backward and gs_render_backward_adam also sums the per-pixel ABSOLUTE values, per Gaussian and in pixel units:
 *   Ax = sum over pixels |g_x|,   g_x = h (c00 dx + 1/2 (c01 + c10) dy),
 *   Ay = sum over pixels |g_y|,   g_y = h (c11 dy + 1/2 (c01 + c10) dx),
 * d = pixel - mean, c the conic, h = dL/d(alpha) raw, 0 for an entry at or past the pixel's stop and for raw > 0.99 (the signed
 * sums of the same terms are the mean's gradient the backward has always produced).  While a grad-norm accumulator is set
 * (gs_set_grad_norm_accum) such a backward adds
 *   accum[p] += hypot(W/2 Ax, H/2 Ay)
 * (gsplat's and Inria's NDC scaling of the screen-space gradient) in place of |grad xyz|; a step whose forward overflowed its
 * reserved pairs adds nothing, as before.  Every gradient, render and parameter update is what it is with absgrad off.
 * enable: 0 (the default: no kernel, buffer or result differs) or 1; any other value returns GS_ERR_INVALID_ARG.  A
 * per-context setting as gs_set_antialiasing is.  GS_ERR_INVALID_ARG with enable = 1 on a context whose tile size is served by
 * the generic blend kernels (not a multiple of 16 and block lists off).  Composes with the anti-aliased mode, the 3-D filter,
 * pose refinement, depth cuts, view hints and block lists.  Single-device steps only: while it is on, gs_render_backward_dp*
 * and gs_dp_step return GS_ERR_INVALID_ARG.  The op-level gs_blend_backward ignores it. */
int gs_set_absgrad(gs_ctx* ctx, int enable);
/* (Ax, Ay) of the last gs_render_backward / gs_render_backward_adam, as defined above, 0 for a Gaussian in no list.  Valid
 * until the next forward or backward on the context.  GS_ERR_NO_FORWARD if no backward has run with absgrad on since it was
 * enabled (or a forward has run since); GS_ERR_SIZE_MISMATCH if N is not that backward's N.  Asynchronous on the context's
 * stream, no allocation. */
int gs_get_absgrad(gs_ctx* ctx, int N, float* out /* DEVICE [N,2] */);

/* Sparse Adam (not in the reference; Taming 3DGS, Mallick et al. 2024: Inria's --optimizer_type sparse_adam,
 * gsplat's visible_adam / SelectiveAdam): the step updates only the Gaussians its view saw.  A Gaussian is VISIBLE in a step iff
 * the step's fused forward gave it a radius > 0 -- the N_visible of gs_last_stats; a Gaussian the forward treats as degenerate has
 * radius 0; under a pose correction or the anti-aliased mode it is whatever that forward computed; depth cuts, view hints, trimmed
 * rects, the tile size and block lists do not enter.  A visible Gaussian no pixel blended (occluded, cut) is still visible: it takes
 * the ordinary update on a zero gradient, so its moments decay.
 * While on, every gs_render_forward keeps the visibility of its N Gaussians in memory of the context's (allocated by the first
 * forward that needs it, regrown only when N outgrows it: no step allocates), and gs_render_backward_adam gives a visible row
 * exactly the update it gets with the setting off, and leaves every element of an invisible row -- parameter, first and second
 * moment, in all six tensors -- bit for bit as it was.  The overflow gate keeps its meaning (raised: no row moves), and the
 * grad-norm accumulator gets what it gets with the setting off (an invisible row adds 0 to it either way).
 * enable: 0 (the default: no kernel, buffer or result differs) or 1; any other value returns GS_ERR_INVALID_ARG.  A per-context
 * setting as gs_set_antialiasing is.  Composes with the anti-aliased mode, pose refinement, the per-view colour corrections,
 * absgrad, depth cuts, view hints and block lists.  Refused with GS_ERR_INVALID_ARG while it is on: gs_render_backward_dp*,
 * gs_dp_step, gs_sh_grad_from_views_adam*, gs_set_mcmc and gs_set_filter3d with a non-NULL argument; turning it on while the MCMC
 * strategy or a 3-D filter is set is refused likewise.  gs_render_backward_adam returns GS_ERR_NO_FORWARD when the setting is on
 * and the forward was made before it was turned on. */
int gs_set_sparse_adam(gs_ctx* ctx, int enable);
/* The visibility mask of the context's last gs_render_forward, which must have been made with sparse Adam on: 1 or 0 per
 * Gaussian.  It stays readable after the setting has been turned off, until the next forward.  GS_ERR_NO_FORWARD if the last
 * forward was not made under the setting (or there is none); GS_ERR_SIZE_MISMATCH if N is not that forward's N.  Asynchronous on
 * the context's stream, no allocation. */
int gs_get_visibility(gs_ctx* ctx, int N, unsigned char* out /* DEVICE [N] */);

/* 3-D smoothing filter (not in the reference; DESIGN.md "3-D smoothing filter"): Mip-Splatting's other filter.  The anti-aliased
 * mode above fixes a model viewed from further away than it was trained; this one fixes the other direction: a Gaussian may
 * not be narrower than the sampling interval of the closest training camera that saw it, or the model shows needle and
 * erosion artefacts when it is viewed closer, or at a higher resolution, than its training views.
 *   Filter width f_i >= 0 per Gaussian, in scene units, a float32 DEVICE array the caller owns.  For each training camera n:
 *     p = [x_i, 1] . view_n (the row-vector convention of gs_camera), z = p.z; the Gaussian is SEEN by n iff z >= 0.2 (the
 *     projection's visibility rule), |p.x / z| <= 1.3 tan(fov_x / 2) and |p.y / z| <= 1.3 tan(fov_y / 2) (Mip-Splatting's
 *     15 % screen margin, 0.65 W / focal, the constant of the EWA clamp); its interval there is T_n = z / focal_x,n.
 *     f_i = sqrt(0.2) min over the seeing cameras of T_n -- the paper's maximal sampling rate max focal / depth, taken per
 *     camera (Mip-Splatting's code takes one global focal).  A Gaussian no camera sees gets the LARGEST f among the seen ones
 *     (Mip-Splatting's convention); if none is seen at all, every f_i is 0.
 *   Activations.  While a filter is set, each gs_render_forward uses, with s_a = exp(scales_raw_a), sigma = sigmoid(opacity_raw):
 *     s_eff_a = sqrt(s_a^2 + f^2) (a = 0, 1, 2),  kappa = prod_a (s_a / s_eff_a) (a product of the three ratios),
 *     opacity = sigma kappa (times rho in the anti-aliased mode, rho from the covariance of s_eff).
 *     Everything downstream is the existing arithmetic on s_eff and that opacity: covariance, conic, radius, rects, trimmed
 *     rects, block lists, depth cuts, the degenerate-invisible rule.  s_eff >= s, so radii and the pair count M can grow.
 *     f = 0 gives s_eff = s and kappa = 1 exactly (sqrtf(s s) = s under correct rounding): the filter-less kernels' results.
 *   Backward, with g_a = dL/ds_eff_a, c = dL/d(packed opacity), rho = 1 outside the anti-aliased mode:
 *     dL/dscales_raw_a = g_a s_a^2 / s_eff_a + c sigma rho kappa f^2 / s_eff_a^2,   dL/dopacity_raw = c kappa rho sigma (1 - sigma),
 *     and the anti-aliased mode's covariance cotangent takes c sigma kappa where it takes c sigma without the filter.
 *     f is not differentiated.  A backward uses the filter pointer its forward ran with; keep the array unchanged between
 *     the two, as the parameter tensors.
 *
 * gs_set_filter3d_cameras: the training cameras gs_compute_filter3d measures against, V >= 0 HOST structs (view, fov_x, fov_y,
 * focal_x and proj[0], proj[5], proj[8], proj[9] are read), copied into a table the context owns.  The table is allocated or
 * grown here only; V = 0 frees it.  A camera with an off-centre principal point (proj[8] or proj[9] non-zero, DESIGN.md
 * section 23) is SEEN-tested against its own frustum with the same margin: |p.x / z + ox| <= 1.3 tan(fov_x / 2) with
 * ox = proj[8] / proj[0], and |p.y / z + oy| likewise with oy = proj[9] / proj[5]; the offset is folded into the table's
 * row (view column 0 gains ox times column 2, column 1 gains oy times column 2), and a zero offset leaves the row's bits.
 * [sync] */
int gs_set_filter3d_cameras(gs_ctx* ctx, int V, const gs_camera* cams /*HOST [V]*/);
/* filter[i] = f_i of xyz[i] against the cameras set above (GS_ERR_INVALID_ARG without any).  Asynchronous on the context's
 * stream, allocates nothing.  The result does not depend on the launch shape: cameras in table order, one fixed float32
 * expression per (Gaussian, camera), a min and a max. */
int gs_compute_filter3d(gs_ctx* ctx, int N, const float* xyz /*DEVICE [N,3]*/, float* filter /*DEVICE [N]*/);
/* The filter of the following forwards: NULL (the default) is the behaviour without the filter, kernel for kernel.  A
 * per-context setting as gs_set_antialiasing is.  It composes with the anti-aliased mode on and off, pose refinement, depth
 * cuts and view hints, trimmed rects and block lists, gs_render_backward and gs_render_backward_adam.  Single-device steps and
 * the reference strategy only: while a filter is set (or the last forward ran with one), gs_render_backward_dp*, gs_dp_step
 * and gs_set_mcmc with non-NULL params return GS_ERR_INVALID_ARG, and so does this call with a non-NULL filter while the
 * MCMC strategy is set.  The op-level entry points (gs_projection_*, gs_pack_gaussians, gs_blend_*) ignore it.  PLY snapshots
 * do not record it: export with gs_filter3d_bake. */
int gs_set_filter3d(gs_ctx* ctx, const float* filter /*DEVICE [>= N] or NULL*/);
/* Mip-Splatting's fused export: out_scales_raw = log(s_eff), out_opacity_raw = logit(sigma kappa).  A model baked this way and
 * rendered with the filter off is the filtered model, for any viewer.  The outputs may alias the inputs they replace (not
 * `filter`).  Asynchronous on the context's stream. */
int gs_filter3d_bake(gs_ctx* ctx, int N, const float* scales_raw /*[N,3]*/, const float* opacity_raw /*[N]*/,
                     const float* filter /*[N]*/, float* out_scales_raw /*[N,3]*/, float* out_opacity_raw /*[N]*/);

/* Lens undistortion (not in the reference; lens.py restates it in float64): resamples a view taken
 * through OpenCV's / COLMAP's radial-tangential lens (fx, fy, cx, cy, k1, k2, p1, p2) into the pinhole camera (dst_fx, dst_fy,
 * dst_cx, dst_cy), once per view when a dataset is loaded.  Pixel i covers [i, i + 1): its centre is at i + 0.5 (COLMAP's and
 * nerfstudio's convention).  For destination pixel (i, j), in float32 and in this order of operations (no contraction):
 *   x = ((i + 0.5) - dst_cx) / dst_fx,  y = ((j + 0.5) - dst_cy) / dst_fy,  r2 = x x + y y,  r4 = r2 r2,
 *   radial = (1 + k1 r2) + k2 r4,
 *   xd = (x radial + (2 p1) (x y)) + p2 (r2 + 2 (x x)),  yd = (y radial + p1 (r2 + 2 (y y))) + (2 p2) (x y),
 *   su = (fx xd + cx) - 0.5,  sv = (fy yd + cy) - 0.5,  x0 = floor(su), y0 = floor(sv), a = su - x0, b = sv - y0.
 * The pixel is VALID iff the four taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) lie inside the source and the
 * radial map has not folded back, (1 + (3 k1) r2) + (5 k2) r4 > 0.  An invalid pixel gets 0 in every channel and valid 0; a
 * valid one gets valid 255 and, from its taps t00, t10 (x0 + 1), t01 (y0 + 1), t11:
 *   mode 0  colour, float32 [src_h, src_w, channels] interleaved, channels in 1 .. 4:
 *           (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b per channel;
 *   mode 1  mask, uint8, channels = 1: the same blend of the levels, then floor(v + 0.5);
 *   mode 2  depth, float32, channels = 1, 0 = hole: sum w_i d_i / sum w_i over the taps with d_i > 0, w00 = (1 - a) (1 - b),
 *           w10 = a (1 - b), w01 = (1 - a) b, w11 = a b, summed in that order; 0 when the weights' sum is 0.
 * Independent of the context's W, H; src and dst do not alias; valid may be NULL.  channels outside 1 .. 4, mask or depth with
 * channels != 1, non-positive or non-finite focal lengths, non-finite coefficients, non-positive sizes or a destination of
 * more than 262140 rows return GS_ERR_INVALID_ARG.  Asynchronous on the context's stream, allocates nothing. */
typedef struct gs_lens { float fx, fy, cx, cy, k1, k2, p1, p2; float dst_fx, dst_fy, dst_cx, dst_cy; } gs_lens;
int gs_undistort(gs_ctx* ctx, const gs_lens* lens /*HOST*/, int src_w, int src_h, int dst_w, int dst_h, int channels,
                 int mode, const void* src /*DEVICE*/, void* dst /*DEVICE*/, unsigned char* valid /*DEVICE [dst_h,dst_w] or NULL*/);

/* The same resampling for OpenCV's / COLMAP's fisheye lens (OPENCV_FISHEYE: fx, fy, cx, cy, k1 .. k4; SIMPLE_RADIAL_FISHEYE and
 * RADIAL_FISHEYE are the family with k3 = k4 = 0) into the IDEAL EQUIDISTANT camera (dst_fx, dst_fy, dst_cx, dst_cy) that
 * GS_CAMERA_FISHEYE renders.  A destination pixel's normalised (x, y) is theta (cos phi, sin phi), and the
 * lens maps theta forward to theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8): no inversion.  In float32
 * and in this order (no contraction), x and y as above:
 *   t2 = x x + y y,  radial = (((k4 t2 + k3) t2 + k2) t2 + k1) t2 + 1,  su = (fx (x radial) + cx) - 0.5,  sv = (fy (y radial) + cy) - 0.5.
 * VALID iff the four taps lie inside the source, d theta_d / d theta = ((((9 k4) t2 + 7 k3) t2 + 5 k2) t2 + 3 k1) t2 + 1 > 0, and t2
 * is below the first root of that derivative inside the destination image (found on the host in float64: a scan of 4096 steps
 * and bisection).  Modes, taps, layouts, the validity output, the argument checks and the asynchrony are gs_undistort's. */
typedef struct gs_fisheye_lens { float fx, fy, cx, cy, k1, k2, k3, k4; float dst_fx, dst_fy, dst_cx, dst_cy; } gs_fisheye_lens;
int gs_undistort_fisheye(gs_ctx* ctx, const gs_fisheye_lens* lens /*HOST*/, int src_w, int src_h, int dst_w, int dst_h, int channels,
                         int mode, const void* src /*DEVICE*/, void* dst /*DEVICE*/, unsigned char* valid /*DEVICE [dst_h,dst_w] or NULL*/);

/* Mesh extraction (not in the reference; tests/tsdf_numpy.py restates both halves): depth images fused
 * into a truncated signed distance volume, then marching tetrahedra.
 *
 * VOLUME.  Lattice point (i, j, k) lies at origin + voxel (i, j, k), in float32 one product and one sum per axis, and has linear
 * index i + nx (j + ny k): x is fastest in memory.  The caller owns the device arrays tsdf [n], weight [n], rgb [n, 3],
 * cweight [n] (float32, n = nx ny nz; zeros = nothing observed); rgb and cweight are both given or both NULL.  Every dimension
 * is 2 .. 1024 and n <= 2^28 (7 n fits 31 bits); voxel and trunc are finite and > 0, the origin finite: otherwise
 * GS_ERR_INVALID_ARG.
 *
 * gs_tsdf_integrate fuses 1 .. GS_TSDF_MAX_VIEWS pinhole views.  A view is the row-major 3 x 4 world-to-view [R | t] (OpenCV
 * axes: x right, y down, z forward), fx, fy, cx, cy (pixel i covers [i, i + 1), camera.py's convention), the image size, a device
 * depth image [height, width] of view-space z (0, negative or non-finite = hole) and an optional device colour image
 * [height, width, 3].  For every lattice point p and every view in order, in float32 and in this order of operations (no
 * contraction):
 *   x = ((R00 px + R01 py) + R02 pz) + t0, y and z likewise from rows 1 and 2; skip unless z > 0 and finite;
 *   u = fx (x / z) + cx, v = fy (y / z) + cy; the pixel is (floor u, floor v); skip unless 0 <= floor u <= width - 1 and
 *     0 <= floor v <= height - 1, compared as floats before any conversion (a NaN fails every test);
 *   d = depth[pixel]; skip unless d > 0 and finite;  s = d - z; skip if s < -trunc;  f = min(1, s / trunc);
 *   tsdf = (tsdf w + f) / (w + 1), w = w + 1 (w the voxel's weight);
 *   where s <= trunc, a colour image is given and rgb is not NULL: rgb_c = (rgb_c cw + colour_c) / (cw + 1) per channel, then
 *     cw = cw + 1 (cw the voxel's cweight).
 * One lane per lattice point, its state in registers across the views of the call: the volume is read once and written once (where
 * a view touched it) per call, and a call of k views computes bit for bit what k one-view calls compute.  A voxel no view
 * reaches keeps every bit.  n_views outside 1 .. GS_TSDF_MAX_VIEWS, a NULL depth image, non-positive sizes, non-finite or
 * non-positive focal lengths or non-finite other numbers return GS_ERR_INVALID_ARG.  Asynchronous on the context's stream (the
 * views are copied into the launch), allocates nothing.
 *
 * EXTRACTION is marching tetrahedra on the Kuhn (Freudenthal) split: every cell (i, j, k) .. (i + 1, j + 1, k + 1) is cut into
 * the 6 tetrahedra that are the paths (0,0,0) -> (1,1,1) adding the axes in one of their 6 permutations, taken in lexicographic
 * order (xyz, xzy, yxz, yzx, zxy, zyx); the split is translation invariant, so neighbouring cells agree on their shared face
 * diagonals.  Inside is tsdf < 0.  A tetrahedron is emitted iff all four corners have weight >= min_weight.  A vertex lies on one
 * lattice edge whose endpoints differ in being inside; every lattice point OWNS the 7 edges towards (1,0,0), (0,1,0), (0,0,1),
 * (1,1,0), (1,0,1), (0,1,1), (1,1,1) (slots 0 .. 6), and with a the owner, b the other end, f the tsdf:
 *   t = f_a / (f_a - f_b),  position_c = p_a_c + t (p_b_c - p_a_c) per axis, p as under VOLUME;
 *   colour_c = rgb_a_c + t (rgb_b_c - rgb_a_c); an endpoint's own colour where the other has cweight 0, 0.5 where both have.
 * A vertex is created once, whoever uses it; only referenced vertices exist.  Vertices ascend in (owner's linear index * 7 +
 * slot), triangles in (cell's linear index, tetrahedron 0 .. 5, triangle 0 / 1).  Triangles are counter-clockwise seen from the
 * tsdf >= 0 side, decided from the tetrahedron's parity (the permutation's sign) and its sign pattern alone, never from
 * positions, so zero-area triangles (a lattice value of exactly 0) are wound like their neighbours.  With the path corners
 * numbered 0 .. 3, for an even tetrahedron (an odd one takes the rule with inside and outside exchanged):
 *   one corner i inside: the vertices on (i, a), (i, b), (i, c), where (i, a, b, c) is an even permutation of (0, 1, 2, 3) and a
 *     the lowest of the three; one corner i outside: those in reverse, (i, c), (i, b), (i, a);
 *   two inside p < q, two outside r < s: the quad pr, ps, qs, qr, walked the other way round from pr (pr, qr, qs, ps) when
 *     (p, r, s, q) is an odd permutation, split along the diagonal from its first vertex: (c0, c1, c2), (c0, c2, c3).
 *
 * gs_tsdf_mesh_plan marks the used edges and counts the triangles per cell, scans both (tile sums, one block over the tiles with
 * 64-bit totals, apply), copies counts = {vertices, triangles} to the HOST and waits [sync].  More than INT32_MAX of either:
 * GS_ERR_INVALID_ARG.  workspace is a device buffer of at least gs_tsdf_mesh_workspace_bytes(grid) bytes (0 for a grid outside
 * the limits), 256-byte aligned.  gs_tsdf_mesh_emit, asynchronous, writes the mesh the context's LAST plan counted into caller
 * buffers of those sizes: vertices [V, 3] float32, colors [V, 3] float32 or NULL (needs rgb and cweight), faces [F, 3] int32.  It
 * takes the plan's workspace, grid and min_weight and the same, unchanged, tsdf and weight (anything else: GS_ERR_INVALID_ARG, or
 * GS_ERR_NO_FORWARD without a plan); a plan of 0 vertices and 0 triangles launches nothing and reads no buffer.  Neither call
 * allocates.  No kernel of the three uses a float atomic or orders workgroups: the output is bit-reproducible. */
#define GS_TSDF_MAX_VIEWS 8
typedef struct gs_tsdf_grid { float origin[3]; float voxel; int nx, ny, nz; float trunc; } gs_tsdf_grid;
typedef struct gs_tsdf_view {
    float Rt[12];
    float fx, fy, cx, cy;
    int width, height;
    const float* depth;   /* DEVICE [height, width] */
    const float* color;   /* DEVICE [height, width, 3] or NULL */
} gs_tsdf_view;
int gs_tsdf_integrate(gs_ctx* ctx, const gs_tsdf_grid* grid /*HOST*/, int n_views, const gs_tsdf_view* views /*HOST [n_views]*/,
                      float* tsdf /*[n]*/, float* weight /*[n]*/, float* rgb /*[n,3] or NULL*/, float* cweight /*[n] or NULL*/);
size_t gs_tsdf_mesh_workspace_bytes(const gs_tsdf_grid* grid /*HOST*/);
int gs_tsdf_mesh_plan(gs_ctx* ctx, const gs_tsdf_grid* grid /*HOST*/, const float* tsdf, const float* weight, float min_weight,
                      void* workspace, size_t workspace_bytes, long long* counts /*HOST [2]*/);
int gs_tsdf_mesh_emit(gs_ctx* ctx, const gs_tsdf_grid* grid /*HOST*/, const float* tsdf, const float* weight, const float* rgb,
                      const float* cweight, float min_weight, void* workspace, float* vertices /*[V,3]*/, float* colors /*[V,3] or NULL*/,
                      int32_t* faces /*[F,3]*/);

/* MCMC densification strategy (not in the reference; DESIGN.md "MCMC strategy"): "3D Gaussian Splatting as Markov Chain Monte
 * Carlo" (Kheradmand et al. 2024), gsplat's MCMCStrategy, with its defaults in brackets.  Notation: o = sigmoid(opacity_raw),
 * s = exp(scales_raw), R the rotation of q / (|q| + 1e-8), Sigma = R diag(s^2) R^T, N the Gaussian count.
 *   Every step (a step the overflow gate skips changes nothing, noise included):
 *     regularisers: the gradient gains opacity_reg o (1 - o) / N on every opacity_raw and scale_reg s_j / (3 N) on every
 *       scales_raw element, visible or not (the gradients of opacity_reg mean(o) + scale_reg mean(s));
 *     Adam, unchanged (the project's, no bias correction);
 *     noise, from the parameters AFTER the update: xyz += Sigma eps noise_lr lr_xyz / (1 + exp(-100 ((1 - o) - 0.995))),
 *       eps ~ N(0, I3) from Philox4x32-10 with counter (row, iteration, "mcmc", "nois") and key seed (gs_mcmc_random stream 0),
 *       lr_xyz the xyz learning rate of the step's Adam.
 *   Every event (the host's cadence), after that step's Adam and noise: gs_mcmc_relocate, then gs_mcmc_grow.
 * The four float64 scalars are rounded to float32 where a kernel uses them; opacity_reg / N, scale_reg / (3 N) and
 * noise_lr lr_xyz are formed in float64 first. */
typedef struct gs_mcmc_params {
    double noise_lr;          /* 5e5 */
    double opacity_reg;       /* 0.01 */
    double scale_reg;         /* 0.01 */
    double min_opacity;       /* 0.005: a row with o <= min_opacity, or o not finite, is dead */
    double grow_rate;         /* 0.05: growth to min(cap_max, floor((1 + grow_rate) N)) */
    long long cap_max;        /* 1000000: the budget; N never exceeds it */
    int n_max;                /* 51: the relocation formula's largest n, 1 .. 51 */
    int iteration;            /* t: keys the step's noise and the event's draws */
    unsigned long long seed;  /* key of every stream of the strategy */
} gs_mcmc_params;

/* The strategy's per-step part for gs_render_backward_adam (NULL = off, the default): while set, that call adds the
 * regularisers' gradients in front of its Adam update and the noise behind it, in the same kernel (plain, posed, either
 * anti-aliasing mode).  The struct is copied; set it again when `iteration` changes.  A per-context setting as
 * gs_set_antialiasing is; gs_render_backward, the data-parallel entry points and the op-level ones ignore it. */
int gs_set_mcmc(gs_ctx* ctx, const gs_mcmc_params* params /*HOST or NULL*/);
/* The regularisers alone (the unfused step: gs_render_backward, this, gs_adam_step, gs_mcmc_inject_noise):
 * grad_opacity[i] += opacity_reg o (1 - o) / N, grad_scales[i, j] += scale_reg s_j / (3 N), over all N rows. */
int gs_mcmc_regularizer_grad(gs_ctx* ctx, int N, const float* scales, const float* opacity, float* grad_scales,
                             float* grad_opacity, const gs_mcmc_params* params /*HOST*/);
/* The noise alone: xyz += the step's noise of the parameters as they are now (call it behind the step's gs_adam_step).
 * lr_xyz: that step's xyz learning rate.  Gated like the optimizer kernels (gs_set_update_gate). */
int gs_mcmc_inject_noise(gs_ctx* ctx, int N, float* xyz, const float* scales, const float* rotation, const float* opacity,
                         float lr_xyz, const gs_mcmc_params* params /*HOST*/);
/* The generator, raw: for i in [0, n), Philox4x32-10 with counter (i, iteration, 0x6d636d63, tag) and key seed, tag by
 * stream: 0 noise 0x6e6f6973, 1 relocation draws 0x72656c6f, 2 growth draws 0x67726f77.  words[n,4] the four output words;
 * normals[n,3] = (r_a cos 2 pi u1, r_a sin 2 pi u1, r_b cos 2 pi u3), r_a = sqrt(-2 ln u0), r_b = sqrt(-2 ln u2),
 * u_k = ((w_k >> 8) + 1/2) 2^-24, in float32; uniforms[n] = ((w0 >> 5) 2^26 + (w1 >> 6) + 1/2) 2^-53 in float64.  Any
 * output may be NULL. */
int gs_mcmc_random(gs_ctx* ctx, unsigned long long seed, int iteration, int stream, int n, uint32_t* words,
                   float* normals, double* uniforms);
/* Relocation.  Rows [0, N) of the six tensors (raw; features_rest [N, K-1, 3]), whose Adam moments lie at the same offsets
 * from exp_avg / exp_avg_sq as the tensors from param_base (gs_render_backward_adam's arenas).  If there is at least one
 * dead and one live row: n_dead sources are drawn from the live rows with replacement, probability proportional to o (the
 * inverse CDF over a float64 prefix sum of the live rows in index order, uniforms from stream 1 keyed by `iteration`); a
 * source drawn c times gets n = min(c + 1, n_max),
 *   o' = clamp(1 - (1 - o)^(1/n), min_opacity, 1 - 2^-23),
 *   s' = s o / sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)       (float64),
 * opacity_raw = logit(o'), scales_raw = log(s'); the k-th dead row (index order) receives the k-th draw's modified source
 * row, all six tensors.  The moments of sources and destinations are zeroed; every other row and moment is left alone.
 * Deterministic (no float atomics).  stats HOST [4] = dead, relocated, live, N.  [sync: one read of the counts] */
int gs_mcmc_relocate(gs_ctx* ctx, int N, int K, float* xyz, float* features_dc, float* features_rest, float* scales,
                     float* rotation, float* opacity, const float* param_base, float* exp_avg, float* exp_avg_sq,
                     const gs_mcmc_params* params /*HOST*/, long long stats[4] /*HOST*/);
/* Growth.  n_add = min(cap_max, floor((1 + grow_rate) N)) - N if positive; n_add sources are drawn from all N rows with
 * probability proportional to o (rows whose opacity_raw is not finite weigh 0; stream 2), modified as gs_mcmc_relocate's sources are,
 * and their modified rows appended at [N, N + n_add) with zero moments.  The tensors must have room for `capacity` rows
 * (GS_ERR_SIZE_MISMATCH if N + n_add would exceed it).  No row weighs anything: nothing is added.  *N_out = the new count.
 * [sync: one read of the counts] */
int gs_mcmc_grow(gs_ctx* ctx, int N, int capacity, int K, float* xyz, float* features_dc, float* features_rest,
                 float* scales, float* rotation, float* opacity, const float* param_base, float* exp_avg, float* exp_avg_sq,
                 const gs_mcmc_params* params /*HOST*/, int* N_out /*HOST*/);

/* Data-parallel form of gs_render_backward (not in the reference, which is single-device): identical, except that
 * instead of the two SH gradient tensors it returns color_cot[N,3] = the cotangent of the SH colour after the
 * max(., 0) gate.  One view's SH gradient is basis_k(xyz - cam_center) x color_cot, so ranks exchange 12 B per
 * Gaussian (all-gather) instead of 12 K B (all-reduce) and rebuild the sum with gs_sh_grad_from_views. */
int gs_render_backward_dp(gs_ctx* ctx, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                          float* grad_xyz, float* grad_scales, float* grad_rotation, float* grad_opacity,
                          float* color_cot /*[N,3]*/);
/* The same in two halves, so that the exchange of color_cot can overlap with the projection backward: _begin runs
 * the blend backward and produces color_cot (from the blend's accumulator and the gate bits the forward kept);
 * _finish runs the projection backward for the four geometry gradients.  _finish must follow _begin on the ctx. */
int gs_render_backward_dp_begin(gs_ctx* ctx, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                                float* color_cot /*[N,3]*/);
int gs_render_backward_dp_finish(gs_ctx* ctx, float* grad_xyz, float* grad_scales, float* grad_rotation,
                                 float* grad_opacity);
/* grad_features_dc[N,1,3] / grad_features_rest[N,K-1,3] = sum over the R views (R <= 16) of
 * basis_k(xyz - cam_centers[r]) * color_cot_all[r][N][3].
 * Alignment, here and in the two _adam forms below: when a row of the rest tensor, 3 (K - 1) floats, is a multiple of four floats
 * (K = 9, 25) the kernels move it as 16-byte words and the tensor (grad_features_rest / features_rest) must be 16-byte aligned;
 * the _adam forms also need params_base, m_base and v_base 16-byte aligned.  GS_ERR_INVALID_ARG otherwise.  Other K may place the
 * tensor on any float. */
int gs_sh_grad_from_views(gs_ctx* ctx, int N, int K, int R, const float* xyz, const float* color_cot_all,
                          const float* cam_centers /*HOST [R,3]*/, float* grad_features_dc, float* grad_features_rest);

/* gs_sh_grad_from_views with the Adam step of the two SH tensors fused in (features_dc / features_rest are the
 * PARAMETER tensors inside [params_base, params_base + n_arena), updated in place; no SH gradient is written).  xyz
 * must still hold the positions the gradients were taken at: call it before the geometry slice's gs_adam_step. */
int gs_sh_grad_from_views_adam(gs_ctx* ctx, int N, int K, int R, const float* xyz, const float* color_cot_all,
                               const float* cam_centers /*HOST [R,3]*/, float* features_dc, float* features_rest,
                               float* params_base, float* m_base, float* v_base, long long n_arena, float lr_dc,
                               float lr_rest, float beta1, float beta2, float eps, float grad_scale);

/* ABI 6 -- the data-parallel step with the SH rows read ONCE.  A view's xyz gradient has a part that comes through the colour:
 * d_r = sum_k grad basis_k(xyz - cam_r) (SH_k . color_cot_r), for which gs_render_backward_dp_finish stages all SH rows a
 * second time.  Like the SH gradient it is a function of replicated values and of the view's gathered colour cotangent,
 * so the kernel that holds the SH rows for their Adam step rebuilds sum_r d_r for all views:
 *   gs_render_backward_dp_finish_geom   = _finish without the SH rows: grad_xyz LACKS d_r (the all-reduce sums the rest),
 *                                         xyz_own[N,3] receives a copy of it (this view's, for the densify statistic);
 *   gs_sh_grad_from_views_adam_dir      = gs_sh_grad_from_views_adam + xyz_add[N,3] = sum_r d_r (16-byte aligned, readable
 *                                         up to 3 N rounded up to four floats, the pad zero) + the densify statistic:
 *                                         own_xyz[r] (HOST array of R DEVICE pointers, NULL for the views of other ranks) is
 *                                         the xyz_own of view r, and |own_xyz[r] + d_r| is added to the accumulator set by
 *                                         gs_set_grad_norm_accum (per view, GaussianTrainer.swift:724-742) -- _finish_geom
 *                                         adds nothing there;
 *   gs_adam_step_add                    = gs_adam_step with gradient g[i] + add[i] on the leading add_n elements (the xyz
 *                                         segment leads the arena): the geometry slice after the all-reduce.
 * sum_r (geometry_r + d_r) becomes (sum_r geometry_r) + (sum_r d_r): the same value up to float association; every rank
 * forms both sums in the same order, so replicas stay bit-identical.  gs_dp_step does this itself. */
int gs_render_backward_dp_finish_geom(gs_ctx* ctx, float* grad_xyz, float* grad_scales, float* grad_rotation,
                                      float* grad_opacity, float* xyz_own /*[N,3]*/);
/* gs_render_backward_dp_begin + _finish_geom with ONE kernel behind the blend backward (the colour cotangents and the rank's
 * gate word ride in the geometry kernel, which is ~10 us without the SH rows -- too short for an all-gather to hide under,
 * so the separate launch and the fork in front of it bought nothing): what gs_dp_step runs. */
int gs_render_backward_dp_geom(gs_ctx* ctx, const float* cot_color, const float* cot_depth, const float* cot_alpha,
                               float* color_cot /*[N,3]*/, float* grad_xyz, float* grad_scales, float* grad_rotation,
                               float* grad_opacity, float* xyz_own /*[N,3]*/);
int gs_sh_grad_from_views_adam_dir(gs_ctx* ctx, int N, int K, int R, const float* xyz, const float* color_cot_all,
                                   const float* cam_centers /*HOST [R,3]*/, const float* const* own_xyz /*HOST [R] or NULL*/,
                                   float* features_dc, float* features_rest, float* params_base, float* m_base, float* v_base,
                                   long long n_arena, float lr_dc, float lr_rest, float beta1, float beta2, float eps,
                                   float grad_scale, float* xyz_add /*[N,3]*/);
int gs_adam_step_add(gs_ctx* ctx, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                     const long long* seg_end /*HOST*/, const float* seg_lr /*HOST*/, float beta1, float beta2, float eps,
                     float grad_scale, const float* add, long long add_n);

/* ---- row e: the data-parallel step (views shard one per rank; RCCL collectives over xGMI issued by the library) ----
 * The reference trains batch-1 on one device (GaussianTrainer.swift:486-498, 958-1086): there is no call site to
 * replace, the contract is BASELINE.json's north-star.  One process per GPU, one ctx per process.  Every rank runs
 * gs_render_forward (+ gs_loss_forward_backward) on its own view -- no data-path collective -- and then gs_dp_step,
 * which runs the backward, exchanges the gradients on a side stream of the library's own and applies Adam with
 * grad_scale = 1 / world: the same update on every rank, so replicas stay identical without a broadcast.  RCCL is
 * dlopen'ed at the first gs_dp_* call (a process that already holds a copy -- PyTorch's -- shares it); a host needs no
 * RCCL binding of its own. */
#define GS_DP_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank by any means (file, socket, launcher). */
int gs_dp_unique_id(void* id /*HOST [GS_DP_UNIQUE_ID_BYTES]*/);
/* ncclCommInitRank on the ctx's device: collective over the `world` ranks (<= 16) that share the id. [sync] */
int gs_dp_init(gs_ctx* ctx, const void* id /*HOST*/, int rank, int world);
/* ... or borrow the host's communicator (an ncclComm_t created on the ctx's device); it is never destroyed here. */
int gs_dp_attach(gs_ctx* ctx, void* nccl_comm, int rank, int world);
/* Drops the communicator (destroys it if gs_dp_init made it); gs_ctx_destroy does the same. [sync] */
int gs_dp_shutdown(gs_ctx* ctx);
int gs_dp_info(gs_ctx* ctx, int* rank /*HOST*/, int* world /*HOST; 0 = no communicator*/);

typedef enum gs_dp_mode {
    GS_DP_ALLREDUCE = 0,     /* one all-reduce (sum) of the whole gradient arena: N (11 + 3K) floats */
    GS_DP_SH_COMPRESSED = 1  /* a view's SH gradient is rank-1 per Gaussian (basis_k(xyz - cam) x colour cotangent): ranks
                              * all-gather the colour cotangents (12 B per Gaussian and rank) under the projection
                              * backward, all-reduce only the geometry slice (44 B per Gaussian) under the SH rebuild, and
                              * every rank rebuilds the summed SH gradient itself, fused with its Adam step */
} gs_dp_mode;
/* HOST struct.  The four arenas (parameters, gradients, Adam moments) share ONE layout of n_arena floats; the six
 * tensors handed to the preceding gs_render_forward must lie inside params_base (their gradients are written at the
 * same offsets of grads_base).  seg_end / seg_lr: the arena's Adam segments as for gs_adam_step (nseg <= 8).
 * GS_DP_SH_COMPRESSED only: geom_numel = length of the LEADING slice of the arena that holds xyz, scales, rotation and
 * opacity (it must end a segment; the SH tensors lie behind it); cam_centers = the camera centres of ALL ranks' views
 * of this step in rank order; color_cot_local [gs_dp_cc_floats(N)] / color_cot_all [world][gs_dp_cc_floats(N)] are
 * caller-owned scratch (a rank's block = its [N,3] cotangents, then its word of the step's gate, padded to four floats).
 * GS_DP_ALLREDUCE: grads_base must have room for n_arena + 1 floats (the gate word rides behind the gradients). */
typedef struct gs_dp_step_args {
    const float *cot_color, *cot_depth, *cot_alpha;   /* DEVICE; depth / alpha may be NULL */
    float *params_base, *grads_base, *m_base, *v_base; /* DEVICE, 16-byte aligned */
    long long n_arena, geom_numel;
    int nseg;
    long long seg_end[8];
    float seg_lr[8];
    float beta1, beta2, eps;
    const float* cam_centers;                          /* HOST [world,3] */
    float *color_cot_local, *color_cot_all;            /* DEVICE */
} gs_dp_step_args;
/* Backward + gradient exchange + Adam of one data-parallel step, after gs_render_forward (and the loss) on this ctx.
 * Collective: every rank of the communicator calls it once per step with the same mode.  Every optimizer kernel of the
 * step is gated on the OR over the ranks of the forwards' overflow words, so a rank whose forward did not fit its pair
 * reserve is never the only one to skip the update.  ABI 5: the word rides in the step's FIRST payload -- behind the
 * colour cotangents of the all-gather (GS_DP_SH_COMPRESSED: the SH rebuild ORs the gathered words) or behind the
 * gradient arena of the all-reduce (GS_DP_ALLREDUCE: summed; any value > 0 gates) -- instead of in a 4-byte all-reduce
 * of its own: two collectives per step (one) instead of three (two).  The deferred host-side overflow error ("Overflow"
 * above) is suppressed inside the call -- no rank leaves a step half-way -- and surfaces through gs_dp_check_overflow.
 * Asynchronous. */
int gs_dp_step(gs_ctx* ctx, int mode, const gs_dp_step_args* args /*HOST*/);
/* Floats of one rank's block of the colour-cotangent all-gather: 3 N cotangents + 1 gate word, padded to a multiple of 4. */
long long gs_dp_cc_floats(int N);
/* In-place all-reduce (sum) of a caller buffer, ordered behind the ctx stream's work and joined back into it (e.g.
 * the densification statistic before gs_classify_gaussians, one per event).  Collective. */
int gs_dp_allreduce_sum(gs_ctx* ctx, float* buf /*DEVICE*/, long long n);
/* Has any step since the last call been gated?  If so the ranks agree on the largest pair count any of them needed
 * (a max all-reduce) and each regrows its reserve to 1.5x that.  Every rank calls it at the same steps (e.g. every
 * 16th, and after a densify event); the decision is built from reduced words, so all ranks take the same branch.
 * *regrown = 1 if the reserve changed, *pairs_needed = the agreed count (0: nothing was gated). [sync] */
int gs_dp_check_overflow(gs_ctx* ctx, int* regrown /*HOST*/, long long* pairs_needed /*HOST*/);

/* "verify with an all-reduce'd checksum every densify step".  After a densify / prune event every rank must
 * hold the same model (same classify inputs, same noise seed: GaussianTrainer.swift:766-908 replicated without
 * communication); a rank that diverged would hang the job in the next size-dependent collective.  Collective, fixed
 * size: (N, sum of the arena in f64, sum of |arena| in f64) of every rank are min- and max-reduced; GS_OK if all three
 * agree, else GS_ERR_REPLICA_MISMATCH on EVERY rank (gs_last_error names what differs and this rank's values).
 * arena: DEVICE, n_arena floats (the parameter arena).  The sums are taken in a fixed order: identical replicas give
 * identical bits. [sync] */
int gs_dp_check_replicas(gs_ctx* ctx, int N, const float* arena, long long n_arena);
/* ABI 6: the same check in two halves, for a host that must not drain its queue at a densify event (the planned event in a
 * data-parallel step).  _begin queues the checksum on the ctx stream and the collective behind it on the side stream
 * (asynchronous; a verdict still outstanding from an earlier _begin is taken first); _end waits for the reduced words
 * alone and returns the verdict (GS_OK when none is outstanding).  Call _end where the host waits for the device anyway
 * (next to gs_dp_check_overflow, at the next event, before shutdown): a parted model is then reported at most that much
 * later -- the hang this check exists to prevent, a diverged N, is caught at once by gs_dp_check_plan. */
int gs_dp_check_replicas_begin(gs_ctx* ctx, int N, const float* arena, long long n_arena);
int gs_dp_check_replicas_end(gs_ctx* ctx);                                             /* [sync on the check's words] */
/* ABI 6: the ranks' densify plans compared.  words: n <= 8 HOST values (gs_densify_plan_read's: new N, applies, total,
 * keep, split, clone, prune, N); one fixed-size max all-reduce of (w, -w) on the side stream, which does not wait for the
 * ctx stream's queue (the event's gather keeps running).  GS_ERR_REPLICA_MISMATCH on EVERY rank unless all agree.
 * Collective: every rank calls it after the same gs_densify_plan_read. [sync on the side stream] */
int gs_dp_check_plan(gs_ctx* ctx, const long long* words /*HOST*/, int n);

/* Exchange timing (measurement only; bench.py's `exchange` block): while enabled, every gs_dp_step records HIP events
 * around its collectives on the library's side stream and around the ctx stream's waits for them (up to 512 steps).
 * gs_dp_exchange_read waits for both streams and returns the SUMS in milliseconds over the `steps` steps timed since the
 * enable: ms[GS_DP_XT_GATE / _GATHER / _REDUCE] = duration of the 4-byte gate all-reduce, the colour-cotangent all-gather
 * and the gradient all-reduce on the side stream (they include the wait for the slowest peer; ABI 5: there is no gate
 * collective any more, ms[GS_DP_XT_GATE] stays 0);
 * ms[GS_DP_XT_EXPOSED_GATHER / _EXPOSED_REDUCE] = time the ctx stream stood in its wait for them, i.e. wire time NOT hidden
 * under compute.  rccl_version: ncclGetVersion's code (0 if the loaded library has none).  No reference call site (the
 * reference has no multi-device step; GaussianTrainer.swift:486-498).  [sync] */
enum { GS_DP_XT_GATE = 0, GS_DP_XT_GATHER = 1, GS_DP_XT_REDUCE = 2, GS_DP_XT_EXPOSED_GATHER = 3, GS_DP_XT_EXPOSED_REDUCE = 4,
       GS_DP_XT_COUNT = 8 };
int gs_dp_exchange_timing(gs_ctx* ctx, int enable);
int gs_dp_exchange_read(gs_ctx* ctx, float ms[GS_DP_XT_COUNT] /*HOST*/, int* steps /*HOST*/, int* rccl_version /*HOST*/);

/* buildLossAndGrad's loss (GaussianTrainer.swift:689-714): L = (1-l)*mean|R-G| + l*(1-mean ssim)
 * + ld*sum(|D-Dgt|*mask)/max(sum mask,1e-6), with its cotangents w.r.t. render colour and depth.
 * loss_out: device float[4] = {total, l1, mean ssim, depth loss}.  target_depth/depth_mask (u8)/
 * render_depth/cot_depth may be NULL when lambda_depth == 0. */
int gs_loss_forward_backward(gs_ctx* ctx, const float* render, const float* target, const float* render_depth,
                             const float* target_depth, const unsigned char* depth_mask, float lambda_dssim,
                             float lambda_depth, float* loss_out, float* cot_color, float* cot_depth);

/* The TARGET's windowed statistics (mean and mean of squares under the 11x11 window, two of SSIM's five) are the same at
 * every visit of a training view; computing them is 40 % of the loss kernel's forward passes.  cache: DEVICE f32
 * [gs_loss_target_cache_floats] (= 2 x 3 x H x W), caller-owned, one per training view (like the view hint buffer).
 * filled = 0: the following gs_loss_forward_backward computes them as always and fills the cache (and then counts it as
 * filled); filled = 1: it reads them -- the target passed must be the image the cache was filled from.  NULL (default):
 * no cache.  The loss and its cotangent are bit-identical in all three cases (the cache holds the very floats the kernel
 * computes). */
int gs_loss_target_cache_floats(gs_ctx* ctx, long long* n /*HOST*/);
int gs_set_loss_target_cache(gs_ctx* ctx, float* cache /*DEVICE or NULL*/, int filled);

/* Per-pixel loss mask (not in the reference; DESIGN.md "Loss masks"): regions of a training view to ignore, as gsplat's
 * masks= and Inria's alpha_mask take them -- both multiply the render and the ground truth by the mask before the loss.
 * mask DEVICE uint8 [H, W] (the ctx's image size), caller-owned and kept alive while set; pixel weight w = (float)v / 255.0f,
 * one correctly rounded division: 255 is exactly 1.0f (keep), 0 exactly 0.0f (ignore), the values between are soft weights
 * (an anti-aliased matte edge).  While a mask is set, the colour loss of each gs_loss_forward_backward is the loss above of
 * the weighted images w R' and w G, with R' the render after a set exposure or bilateral grid (the render itself without):
 *   L = (1-l) sum|w R' - w G| / (3P) + l (1 - sum ssim(w R', w G) / (3P)),   P = H W.
 * Both sums and the divisor run over ALL pixels, as in gsplat and Inria; there is no re-normalisation by sum w.  A fully
 * masked neighbourhood has ssim exactly 1 and L1 exactly 0 (it costs nothing and pushes nothing), and a kept pixel's gradient
 * has the scale it has without a mask, so no learning rate changes.  cot_color = w * dL/d(w R'), the multiply by w being the
 * last operation: exactly 0.0f wherever v = 0, and bit for bit w times the cotangent of the unmasked loss of images weighted
 * beforehand; loss_out likewise equals that loss's.  A mask of all 255 gives the unmasked loss and cotangent bit for bit.
 * With an exposure or a bilateral grid set the order is correction -> masked loss -> the correction's backward, fed the
 * already weighted cotangent: the correction learns from kept pixels only.  The target cache (gs_set_loss_target_cache) then
 * holds the statistics of the MASKED target -- refill it (filled = 0) when the mask changes -- and the three cache modes
 * stay bit-identical.  The depth term (with its own depth_mask), the render, alpha, depth and every forward / backward entry
 * point are unchanged: the blend backward, the densification statistics, sparse Adam and MCMC see the mask through cot_color
 * alone.  Sticky like gs_set_exposure: read by gs_loss_forward_backward only, from this call until a NULL call.  NULL (the
 * default) issues the loss's launches exactly as without it, kernel for kernel.  The op-level gs_ssim_* ignore the setting.
 * No reference call site (GaussianTrainer.swift:689-714 takes the loss of every pixel). */
int gs_set_loss_mask(gs_ctx* ctx, const unsigned char* mask /*DEVICE [H,W] or NULL*/);

/* Depth supervision on the render's depth and alpha images (tests/depth_loss_numpy.py restates it).  The depth term
 * of gs_loss_forward_backward above is the reference's (GaussianTrainer.swift:689-714, :949): it compares the ACCUMULATED depth
 * D = sum T alpha z with a metric depth map, which is right only where the render is opaque.  This entry point has that form and
 * the two that need the render's alpha a inside the loss and a cotangent into it: gsplat's depth_loss (L1 in disparity on the
 * normalised, "expected", depth) and Inria's depth regularisation (inverse depth against a prior with a per-image scale and
 * offset, depth_params.json).  With t = scale * target + offset (two float32 roundings, never contracted), per pixel of the
 * ctx's H x W image:
 *   GS_DEPTH_ACCUMULATED  x = D      valid iff mask                                 cot_depth = g          cot_alpha = 0
 *   GS_DEPTH_EXPECTED     x = D / a  valid iff mask, a >= alpha_min and a > 0       cot_depth = g / a      cot_alpha = -g D / a^2
 *   GS_DEPTH_DISPARITY    x = a / D  valid iff mask, a >= alpha_min, a > 0, D > 0   cot_depth = -g a / D^2 cot_alpha = g / D
 *   n = max(number of valid pixels, 1e-6),  Ld = sum_valid |x - t| / n,  g = lambda sign(x - t) / n (sign 0 on a tie).
 * (a > 0 matters with alpha_min = 0 only: a pixel nothing was blended into has no expected depth.)  In the disparity mode the
 * target is an inverse depth.  mask: uint8, non-zero = the pixel takes part, NULL = all; it is the depth term's OWN mask (sensor
 * holes), not the colour loss's gs_set_loss_mask, which this call does not read.  loss: the float[4] a
 * gs_loss_forward_backward on this ctx's stream has written: loss[3] = Ld, loss[0] += lambda Ld (read and written; the call is
 * queued behind that loss).  cot_depth and cot_alpha are what the fused backwards take as theirs; EVERY element of both is
 * written -- exactly 0.0f on an invalid pixel, nothing stale --, and nothing is NaN or Inf for a = 0, D = 0 or an image
 * without a valid pixel (Ld = 0, cotangents 0), nor for any finite input whose quotients fit float32: a valid pixel's D / a,
 * a / D and the cotangents above are formed as written, so a positive a or D below about 1e-19 beside an ordinary partner
 * (possible only with alpha_min = 0, or a near-zero D in the disparity mode) overflows like any float32 division.  cot_alpha may be NULL in GS_DEPTH_ACCUMULATED, where
 * render_alpha is not read and may be NULL too.  With scale = 1, offset = 0 that mode is gs_loss_forward_backward's depth term:
 * cot_depth agrees with its cot_depth bit for bit.  Three launches (partial sums, one workgroup that finishes them, cotangents),
 * every one a grid-stride loop, no float atomics -- two calls on the same inputs give the same bits --, no wait; the first
 * call allocates 8 KB of workspace, no later one allocates.  GS_ERR_INVALID_ARG: mode out of range, alpha_min < 0 or not finite,
 * a non-finite lambda / scale / offset, cot_alpha or render_alpha NULL in the expected and disparity modes, a NULL params,
 * render_depth, target, loss or cot_depth. */
enum { GS_DEPTH_ACCUMULATED = 0, GS_DEPTH_EXPECTED = 1, GS_DEPTH_DISPARITY = 2 };
typedef struct gs_depth_loss_params {
    int mode;
    float lambda;
    float alpha_min;
    float scale, offset;
} gs_depth_loss_params;
int gs_depth_loss(gs_ctx* ctx, const gs_depth_loss_params* p /*HOST*/, const float* render_depth /*DEVICE [H,W]*/,
                  const float* render_alpha /*DEVICE [H,W]*/, const float* target /*DEVICE [H,W]*/,
                  const unsigned char* mask /*DEVICE [H,W] or NULL = all*/, float* loss /*DEVICE [4], read and written*/,
                  float* cot_depth /*DEVICE [H,W]*/, float* cot_alpha /*DEVICE [H,W]; may be NULL in mode 0*/);
/* The expected depth of a render, for a viewer or an evaluation: out = D / a where a >= alpha_min and a > 0, 0 elsewhere, for
 * n_pixels pixels.  out may be depth itself.  Asynchronous on the ctx stream, allocates nothing.  n_pixels < 0, alpha_min < 0
 * or not finite, or a NULL pointer: GS_ERR_INVALID_ARG; n_pixels == 0: nothing is launched. */
int gs_depth_normalize(gs_ctx* ctx, long long n_pixels, const float* depth /*DEVICE [n]*/, const float* alpha /*DEVICE [n]*/,
                       float alpha_min, float* out /*DEVICE [n]*/);

/* Normal regularisation from the render's depth and alpha images (tests/normal_loss_numpy.py restates it):
 * the normals of the expected depth image z = D / a, supervised by a normal prior (DN-Splatter's and MonoSDF's L1 and cosine
 * terms) and smoothed (a cosine term between neighbours, weighted by the edges of an image), as the methods that extract meshes
 * from splats train.  The call hands the fused backwards the cotangents of D and a, as gs_depth_loss does.
 *
 * Rays and depth.  A pinhole camera with OpenCV axes (x right, y down, z forward) and camera.py's pixel convention: pixel (i, j),
 * column i and row j, has rx = ((i + 0.5) - cx) / fx and ry = ((j + 0.5) - cy) / fy.  A pixel is DEPTH-VALID iff a >= alpha_min,
 * a > 0 and D > 0; its expected depth is z = D / a.
 *
 * The normal.  A pixel has a normal iff it is interior (1 <= i <= W - 2, 1 <= j <= H - 2), it and its four neighbours are
 * depth-valid and, with max_jump > 0, max(|z+ - z-|, |zd - zu|) <= max_jump z (depth edges are left out).  With the right / left
 * neighbours' z+, z- and the lower / upper neighbours' zd, zu:
 *   A = z+ - z-,  S = (z+ + z-) / fx,  B = zd - zu,  T = (zd + zu) / fy
 *   m = (A T, B S, -(A T rx + B S ry + S T)),  n = m / |m|   (no normal if |m| = 0)
 * which is (P_down - P_up) x (P_right - P_left) of the back-projected points, written so that only A and B cancel.  It faces the
 * camera: n . (rx, ry, 1) < 0.
 *
 * The terms.  Nt is the target normal in camera space, OpenCV axes, facing the camera; it is normalised here, and a target of
 * squared norm < 0.25 is a hole.  mask: uint8, non-zero = the pixel takes part in the prior terms, NULL = all; the term's own
 * mask, not gs_set_loss_mask's.  Vp = the pixels with a normal, a target that is no hole and the mask set; the pairs are the
 * horizontally or vertically adjacent pixels that both have a normal (neither mask nor target enters).
 *   L_l1  = sum_Vp |n - Nt|_1 / max(#Vp, 1e-6)                 (its gradient: sign 0 on a tie)
 *   L_cos = sum_Vp (1 - n . Nt) / max(#Vp, 1e-6)
 *   L_s   = sum_pairs w_pq (1 - n_p . n_q) / max(#pairs, 1e-6),  w_pq = exp(-edge_gamma mean_c |I_p - I_q|)
 * I is edge_image (the trainer passes the step's target colour); w_pq is exactly 1 with edge_image NULL or edge_gamma = 0.  The
 * smoothness term is the cosine form on purpose: an L1 total variation has its kink exactly where the term drives the scene
 * (n_p = n_q).  normal_out[3] = (L_l1, L_cos, L_s); loss[0] += lambda_l1 L_l1 + lambda_cos L_cos + lambda_smooth L_s (read and
 * written: the call is queued behind the loss that wrote it; loss[1..3] are left alone).  target_normals NULL: the prior terms
 * are skipped, L_l1 = L_cos = 0, whatever their weights.
 *
 * Cotangents.  g_n of a pixel is the derivative by its normal of the weighted sum: from its own prior terms and its four pairs.
 *   g_m = (g_n - n (n . g_n)) / |m|
 *   g_A = g_m . (T, 0, -T rx),  g_T = g_m . (A, 0, -(A rx + S)),  g_B = g_m . (0, S, -S ry),  g_S = g_m . (0, B, -(B ry + T))
 *   q+ = g_A + g_S / fx,  q- = -g_A + g_S / fx,  qd = g_B + g_T / fy,  qu = -g_B + g_T / fy
 * and a pixel GATHERS what it is to its neighbours: g_z(i, j) = q+(i-1, j) + q-(i+1, j) + qd(i, j-1) + qu(i, j+1),
 * cot_depth = g_z / a, cot_alpha = -g_z D / a^2, both exactly 0 where the pixel is not depth-valid.  Border pixels have no normal
 * but do receive cotangents.  accumulate = 0: EVERY element of both images is written, zeros included.  accumulate = 1: the values
 * are added to what the images hold (a gs_depth_loss queued before this call wrote them).
 *
 * Five launches (normals; per-block partial sums, in double, the counts exact; one workgroup that finishes them; q; the gather),
 * every one a grid-stride loop, no float atomics -- two calls on the same inputs give the same bits --, no wait.  The first call
 * allocates the workspace in the ctx (7 floats per pixel and 20 KB of partials); a later one only when a larger image needs more
 * (it then waits for the stream).  H and W are the params' own.  GS_ERR_INVALID_ARG with the reason in gs_last_error: a NULL
 * params, render_depth, render_alpha, loss, normal_out, cot_depth or cot_alpha; fx or fy not positive and finite, cx or cy not
 * finite, H or W <= 0; a weight, alpha_min, max_jump or edge_gamma negative or not finite; accumulate other than 0 or 1.
 * No reference call site (the reference app has no normal term). */
typedef struct gs_normal_loss_params {
    float fx, fy, cx, cy;
    int H, W;
    float lambda_l1, lambda_cos, lambda_smooth;
    float alpha_min;
    float max_jump;
    float edge_gamma;
    int accumulate;
} gs_normal_loss_params;
int gs_normal_loss(gs_ctx* ctx, const gs_normal_loss_params* p /*HOST*/, const float* render_depth /*DEVICE [H,W]*/,
                   const float* render_alpha /*DEVICE [H,W]*/, const float* target_normals /*DEVICE [H,W,3] or NULL*/,
                   const unsigned char* mask /*DEVICE [H,W] or NULL = all*/, const float* edge_image /*DEVICE [H,W,3] or NULL*/,
                   float* loss /*DEVICE [4], read and written*/, float* normal_out /*DEVICE [3]*/,
                   float* cot_depth /*DEVICE [H,W]*/, float* cot_alpha /*DEVICE [H,W]*/);
/* The forward alone, for a viewer: out = the normal above, the zero vector where a pixel has none.  intrinsics = (fx, fy, cx, cy).
 * One launch on the ctx stream, allocates nothing.  GS_ERR_INVALID_ARG: a NULL pointer, and what gs_normal_loss refuses of the
 * camera, the size, alpha_min and max_jump. */
int gs_depth_normals(gs_ctx* ctx, const float* intrinsics /*HOST [4]*/, int H, int W, const float* depth /*DEVICE [H,W]*/,
                     const float* alpha /*DEVICE [H,W]*/, float alpha_min, float max_jump, float* out /*DEVICE [H,W,3]*/);

/* Held-out evaluation (tests/metrics_numpy.py restates both calls): the sums behind the PSNR and the SSIM
 * that 3DGS papers report, of a render against its target, in one pass and without a statistic map in device memory.  Both images
 * are clamped to [0, 1] first, as Inria's render.py / metrics.py do; r and g below are the clamped render and target.  mask:
 * uint8, pixel weight w = (float)v / 255.0f as gs_set_loss_mask's (255 is exactly 1, 0 exactly 0), NULL = every w is 1; it is
 * this call's own argument, the ctx's loss mask is not read.
 *   out[0] sse      = sum_pixels w sum_c (r_c - g_c)^2
 *   out[1] ssim_sum = sum_{pixels, c} w ssim_map(w r, w g)
 *   out[2] wsum     = sum_pixels w  (once per pixel)          out[3] = 3 wsum
 *   psnr = -10 log10(out[0] / out[3])  (inf for identical images, nan where wsum = 0),  ssim = out[1] / out[3]
 * ssim_map is Inria's loss_utils.ssim: an 11 x 11 Gaussian window of sigma 1.5 that is CENTRED (exp(-(i - 5)^2 / 2 sigma^2),
 * normalised, outer product) -- not gs_ssim_window's, which is off-centre as the reference app's is --, taps outside the image
 * count as zero, C1 = 1e-4, C2 = 9e-4; evaluated separably (rows, then columns, taps ascending) in float32.  With a mask the
 * statistics are those of the weighted images, as in the masked training loss; without one ssim is Inria's plain mean.
 * H, W are the call's own (any ctx measures any image size).  Asynchronous on the ctx stream; out is written by the device.
 * The sums are double, reduced in a fixed order without float atomics: two calls on the same inputs give the same bits, and a
 * mask of all 255 gives the bits of no mask.  The first call allocates the per-block partials (88 KB), a later one only when a
 * larger image needs more (it then waits for the stream).  H or W == 0: no kernel, out = zeros.  GS_ERR_INVALID_ARG: a NULL
 * render, target or out, H or W < 0.  No reference call site (the reference app has no evaluation). */
int gs_image_metrics(gs_ctx* ctx, int H, int W, const float* render /*DEVICE [H,W,3]*/, const float* target /*DEVICE [H,W,3]*/,
                     const unsigned char* mask /*DEVICE [H,W] or NULL*/, double* out /*DEVICE [4]*/);
/* The moments of the best affine colour transform of a render onto its target -- the colour-corrected metrics gsplat reports when a
 * per-view appearance is trained, a held-out view having none.  p = (r, g, b, 1) the clamped render, t the clamped target, w as
 * above:
 *   out[0..9]   S[i][j] = sum w p_i p_j, the upper triangle by rows: 00 01 02 03 11 12 13 22 23 33  (S[3][3] = sum w)
 *   out[10..21] T[i][c] = sum w p_i t_c, out[10 + 3 i + c]
 * The host solves S M^T = T (least squares, minimum norm where S is singular) for M = [A | b], 3 x 4 as gs_apply_exposure takes it;
 * the corrected metrics are gs_image_metrics of gs_apply_exposure(M, render).  Products and sums in double, a grid-stride loop of at
 * most 512 blocks, the same fixed-order reduction and workspace as above.  n_pixels == 0: no kernel, out = zeros.
 * GS_ERR_INVALID_ARG: a NULL render, target or out, n_pixels < 0.  No reference call site. */
int gs_colour_moments(gs_ctx* ctx, long long n_pixels, const float* render /*DEVICE [n,3]*/, const float* target /*DEVICE [n,3]*/,
                      const unsigned char* mask /*DEVICE [n] or NULL*/, double* out /*DEVICE [22]*/);

/* ---- next row: optimizer step ---------------------------------------------------------------- */

/* Adam over one flat parameter arena, as the trainer applies it per tensor (GaussianTrainer.swift:941-948,
 * 1060-1086; learning rates GaussianModel.swift:56-65): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr * m / (sqrt(v) + eps), no bias correction (mlx-swift 0.30.6 Adam default; parity unpinned).
 * The arena is split into nseg contiguous segments ending at seg_end[i] (element index, exclusive), each with
 * its own learning rate.  grad_scale multiplies the gradient first (1/world_size after an all-reduce sum). */
int gs_adam_step(gs_ctx* ctx, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                 const long long* seg_end /*HOST*/, const float* seg_lr /*HOST*/, float beta1, float beta2,
                 float eps, float grad_scale);
/* gs_adam_step on the visible rows only (sparse Adam, above; what the unfused single-device step ends with).  Segment s holds
 * rows of seg_row_floats[s] >= 1 floats: element e of segment s belongs to row (e - start_s) / seg_row_floats[s].  Rows >= N -- the
 * tail of a capacity-strided segment and the pads that align the segments to 16 bytes -- are left alone, and so are the rows whose
 * mask byte is 0: every element of theirs in params, m and v keeps its bits.  Every other element gets gs_adam_step's update.
 * visible == NULL: the mask gs_get_visibility would return (GS_ERR_NO_FORWARD without one,
 * GS_ERR_SIZE_MISMATCH if N is not that forward's N).  Arguments are checked as gs_adam_step checks its own; gated like it. */
int gs_adam_step_visible(gs_ctx* ctx, long long n, float* params, const float* grads, float* m, float* v, int nseg,
                         const long long* seg_end /*HOST*/, const float* seg_lr /*HOST*/, const int* seg_row_floats /*HOST [nseg]*/,
                         float beta1, float beta2, float eps, float grad_scale, int N,
                         const unsigned char* visible /*DEVICE [N] or NULL*/);

/* ---- next row: densify / prune -------------------------------------------------------------
 * The three kernels of GaussianTrainer.swift:317-427 one to one, the scan between them, and the gather + per-slot
 * modification that the reference writes as MLX array ops (:858-893).  The host sequence (when to run, the
 * early-outs, committing the new tensors, resetting the accumulators and the Adam state) is the trainer's:
 * gaussiansplattingmlx_amd/trainer.py mirrors split_and_prune (:766-907).  Parity unpinned (no reference test;
 * MLXRandom noise is an input here). */

/* accum_grad_norm (:320-338): accum_out[i] = accum_in[i] + |xyz_grad[i,:]|.  accum_in NULL = zeros; in place ok. */
int gs_accum_grad_norm(gs_ctx* ctx, int N, const float* xyz_grad, const float* accum_in, float* accum_out);
/* classify_gaussians (:343-393).  denom is the scalar the reference broadcasts to [N] (:796).  scales[N,scale_stride]
 * raw (log) scales, opacity[N] raw.  actions 0 keep / 1 split / 2 clone / 3 prune; output_counts 1 / 2 / 2 / 0. */
int gs_classify_gaussians(gs_ctx* ctx, int N, const float* grad_accum, float denom, const float* scales,
                          int scale_stride, const float* opacity, float grad_threshold, float max_scale_thresh,
                          float min_opacity_thresh, int allow_densify, int* actions, int* output_counts);
/* The prune decision on a contribution score (gs_blend_contrib / gs_render_contrib), in gs_classify_gaussians' words:
 * actions[i] = 3 (prune), output_counts[i] = 0 where score[i] < threshold, else 0 (keep) and 1 -- the scan, the output map and
 * the gather below then perform the prune unchanged. */
int gs_contrib_actions(gs_ctx* ctx, int N, const float* score /*DEVICE [N]*/, float threshold, int* actions,
                       int* output_counts);
/* offsets = cumsum(output_counts) - output_counts (:813-815) plus the action counts (:838-841).  Synchronises (the
 * reference's .item(), :816): stats HOST [5] = total outputs, keep, split, clone, prune. */
int gs_densify_offsets(gs_ctx* ctx, int N, const int* actions, const int* output_counts, int* offsets,
                       long long stats[5]);
/* build_densify_output_map (:398-427): gather_indices[total], noise_mode[total] (0 none, 1 split +, 2 split -,
 * 3 clone copy), zero-initialised first (:852). */
int gs_build_densify_output_map(gs_ctx* ctx, int N, const int* actions, const int* offsets, int total,
                                int* gather_indices, int* noise_mode);
/* Phases 4-5 (:858-893): out_X = X[gather_indices]; split children: scales + Float(-log 1.6), xyz +/- mean(exp(source
 * scales)) * 0.1 * noise; clone copies: xyz + 0.01 * noise.  base_noise[total,3] standard normal, or NULL for the
 * no-split-no-clone branch (:864) that gathers only.  Outputs must not alias inputs. */
int gs_densify_gather(gs_ctx* ctx, int total, int K, const float* xyz, const float* features_dc,
                      const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                      const int* gather_indices, const int* noise_mode, const float* base_noise, float* out_xyz,
                      float* out_features_dc, float* out_features_rest, float* out_scales, float* out_rotation,
                      float* out_opacity);

/* The event WITHOUT a drain of the queue (ABI 5).  gs_densify_offsets hands the count to the host, which then sizes and
 * queues everything behind it on a device that has run dry (the reference's `.item()`, GaussianTrainer.swift:813-817).
 * Planned: the count stays on the device for the kernels that need it, and the host waits for the PLAN alone, with the
 * event's remaining work already queued behind it.
 *   gs_densify_plan            = the scan of gs_densify_offsets, no wait.  Leaves the plan in the ctx: new count (= total
 *                                outputs when the event applies, else N), whether it applies -- the reference's early-outs
 *                                (all pruned :828-832; nothing to split, clone or prune :819-826, :843-847) as a predicate
 *                                --, total, keep, split, clone, prune, N.
 *   ..._output_map_planned     = gs_build_densify_output_map for `capacity` output slots (zero-filled); the identity map
 *                                when the event does not apply.
 *   gs_densify_gather_planned  = gs_densify_gather over a capacity-sized grid: rows [0, new count) are written (the outputs
 *                                must hold `capacity` rows, or at least the new count), the rest is left alone; a row that
 *                                does not apply is a plain copy.  The noise of row j is gs_densify_noise's row j for
 *                                noise_seed: no tensor of `total` rows to size.
 *   gs_densify_plan_read       = plan[8] HOST = new count, applies, total, keep, split, clone, prune, N once the plan
 *                                kernel has run (*ready = 1); wait = 0: asks without waiting.  Waits for the PLAN, not for
 *                                what was queued behind it. [sync on the plan when wait != 0]
 *   gs_densify_noise           = out[rows,3] standard normal, row j a function of (seed, j) alone (Philox4x32-10 +
 *                                Box-Muller): the tensor form of the planned gather's noise, for gs_densify_gather.
 * The host sequence -- laying the new model out at capacity strides so that its pointers do not depend on the count,
 * flipping, resetting the optimizer state, repeating the gather should the new count exceed the capacity -- is the
 * trainer's (gaussiansplattingmlx_amd/trainer.py, split_and_prune). */
int gs_densify_plan(gs_ctx* ctx, int N, const int* actions, const int* output_counts, int* offsets);
int gs_densify_plan_read(gs_ctx* ctx, int wait, long long plan[8] /*HOST*/, int* ready /*HOST*/);
int gs_build_densify_output_map_planned(gs_ctx* ctx, int N, const int* actions, const int* offsets, int capacity,
                                        int* gather_indices, int* noise_mode);
int gs_densify_gather_planned(gs_ctx* ctx, int capacity, int K, const float* xyz, const float* features_dc,
                              const float* features_rest, const float* scales, const float* rotation, const float* opacity,
                              const int* gather_indices, const int* noise_mode, unsigned long long noise_seed, float* out_xyz,
                              float* out_features_dc, float* out_features_rest, float* out_scales, float* out_rotation,
                              float* out_opacity);
/* ABI 6: gs_densify_gather_planned into a PACKED arena -- every tensor's segment sized by the NEW count (padded to four
 * floats), which is what a data-parallel step wants (it all-reduces the arena's leading geometry slice: at capacity strides
 * that slice would carry capacity / N times the bytes).  The tensor starts depend on a count the host does not have yet, so
 * they are computed on the device behind the plan: out_base (16-byte aligned, room for the capacity) + the padded segments
 * of the tensors in front, in arena_order -- tensor ids in the order they lie in the arena (0 xyz, 1 features_dc,
 * 2 features_rest, 3 scales, 4 rotation, 5 opacity; the trainer's arena is 0 3 4 5 1 2: geometry first).  The host lays
 * the same layout out once gs_densify_plan_read has given it the count.  Pads are not written. */
int gs_densify_gather_planned_packed(gs_ctx* ctx, int capacity, int K, const float* xyz, const float* features_dc,
                                     const float* features_rest, const float* scales, const float* rotation,
                                     const float* opacity, const int* gather_indices, const int* noise_mode,
                                     unsigned long long noise_seed, float* out_base, const int arena_order[6] /*HOST*/);
int gs_densify_noise(gs_ctx* ctx, unsigned long long seed, int rows, float* out /*[rows,3]*/);

/* ---- adaptive density control (not in the reference) ---------------------------------
 * The densification of the original 3DGS (Kerbl et al. 2023: Inria's densify_and_prune / reset_opacity; gsplat's
 * DefaultStrategy), beside the reference's rule above, which it replaces under the trainer's strategy="adc":
 * classify_gaussians (GaussianTrainer.swift:343-393) divides one sum by one global step count and has no size test, and the
 * gather (:858-893) moves a split child by +/- 0.1 mean scale noise along no axis of the Gaussian.  Here the statistic is
 * averaged over the steps that SAW the Gaussian, a split samples its children from the Gaussian itself, the Adam moments
 * of what survives an event survive it, and the opacities are reset periodically.  The scan, the plan and the output map
 * between classify and gather are gs_densify_offsets / gs_build_densify_output_map, unchanged.  All of it is asynchronous
 * on the context's stream and allocates nothing, except where noted.  None of these entry points returns
 * GS_ERR_SIZE_MISMATCH: every buffer is the caller's and carries no size the library could compare N with (the accumulators
 * of gs_set_adc_stats must hold the N of the forwards made while they are set). */

/* The step's statistic.  grad_sum, count, max_radius: caller-owned DEVICE [N] float accumulators (N of the forwards that
 * follow; the caller zeroes them), all three set, or all three NULL to turn it off (the default: no kernel, buffer or result
 * differs).  While set, every gs_render_forward keeps the radii it computed -- in the caller's radii buffer, which must then
 * stay alive until the backward, or in memory of the context's (the buffer sparse Adam uses; allocated by the first forward
 * that needs it, regrown only when N outgrows it) --, and the blend backward of gs_render_backward and
 * gs_render_backward_adam adds, for every Gaussian p that forward gave a radius > 0,
 *   grad_sum[p] += hypot(W/2 gx, H/2 gy),   count[p] += 1,   max_radius[p] = max(max_radius[p], radius[p]),
 * (gx, gy) the gradient of the loss with respect to the Gaussian's 2-D mean in pixel units (gsplat's and Inria's NDC scaling;
 * with absgrad on -- gs_set_absgrad -- the absolute sums (Ax, Ay) in their place: gsplat's DefaultStrategy(absgrad=True)).  A
 * Gaussian of radius 0 keeps the bits of its three words; count, a float, is exact up to 2^24 visits.  A step whose forward
 * overflowed its reserved pairs adds nothing (the gate of the fused Adam).  Every render, gradient and parameter update is what
 * it is with the statistic off; a grad-norm accumulator (gs_set_grad_norm_accum) is independent of it.
 * GS_ERR_INVALID_ARG: one or two of the three NULL; a context whose tile size is served by the generic blend kernels.  A
 * backward whose forward was made before the statistic was set (and kept no radii) returns GS_ERR_NO_FORWARD.  Single-device
 * steps only: while it is set, gs_render_backward_dp* and gs_dp_step return GS_ERR_INVALID_ARG. */
int gs_set_adc_stats(gs_ctx* ctx, float* grad_sum, float* count, float* max_radius);
/* The same kernel on the caller's rows: rows16 DEVICE [N,16] (8-byte aligned; a blend backward's accumulator rows: columns
 * 0, 1 are read, columns 12, 13 with use_abs = 1), radii DEVICE [N], W and H the context's.  No gate. */
int gs_adc_accumulate(gs_ctx* ctx, int N, const float* rows16, const float* radii, int use_abs, float* grad_sum, float* count,
                      float* max_radius);

typedef struct gs_adc_params {
    float grad_threshold;   /* densify where grad_sum / count >= this (Inria's densify_grad_threshold, 0.0002) */
    float percent_dense;    /* clone up to, split above, max exp(scale) = percent_dense * scene_extent (0.01) */
    float min_opacity;      /* prune below this sigmoid(opacity) (0.005) */
    float max_screen_size;  /* size pruning: prune above this max_radius in pixels (20); <= 0: no screen test */
    float prune_world;      /* size pruning: prune above max exp(scale) = prune_world * scene_extent (0.1) */
    float scene_extent;     /* Inria's cameras_extent: 1.1 x the largest distance of a camera from the cameras' mean */
} gs_adc_params;

/* The decision per Gaussian, in gs_classify_gaussians' words (actions 0 keep / 1 split / 2 clone / 3 prune; output_counts
 * 1 / 2 / 2 / 0), which it replaces (GaussianTrainer.swift:343-393).  avg = count > 0 ? grad_sum / count : 0,
 * smax = max exp(scales[i,0..2]), op = sigmoid(opacity); the first that holds:
 *   1. op < min_opacity                                                                        prune
 *   2. allow_densify and avg >= grad_threshold          clone if smax <= percent_dense scene_extent, else split
 *   3. size_prune and (max_radius > max_screen_size or smax > prune_world scene_extent)         prune
 *   4.                                                                                         keep
 * (max_screen_size <= 0: no screen test.)  Inria grows first and then prunes the grown set; this one pass differs in two
 * corners: a Gaussian over the gradient threshold AND over a size bound is split, not pruned, and a split child still over
 * the world bound lives until the next event.  The two products are taken in float.  GS_ERR_INVALID_ARG: a negative or NaN
 * threshold, scene_extent not positive and finite, scale_stride < 3, a NULL buffer with N > 0. */
int gs_adc_classify(gs_ctx* ctx, int N, const float* grad_sum, const float* count, const float* max_radius,
                    const float* scales, int scale_stride, const float* opacity, const gs_adc_params* params /*HOST*/,
                    int allow_densify, int size_prune, int* actions, int* output_counts);
/* gs_densify_gather's sibling, on the same gather_indices / noise_mode (gs_build_densify_output_map) and a noise[total,3]
 * standard normal (gs_densify_noise); replaces the gather of GaussianTrainer.swift:858-893.  out_X = X[gather_indices], and
 *   split children (modes 1, 2): xyz + R(q) (exp(scales) * noise[j]), each child with its own row's noise, q the source's
 *                                rotation over max(|q|, 1e-8) as the projection normalises it; scales + Float(-log 1.6);
 *   a clone's copy (mode 3):     every parameter copied exactly -- no noise.
 * revised_opacity (0 / 1; Bulo et al. 2024, gsplat's revised_opacity): every split child and both copies of a clone get the
 * raw opacity of alpha' with 1 - (1 - alpha')^2 = alpha.  Outputs must not alias inputs.  GS_ERR_INVALID_ARG: total < 0,
 * K < 1, revised_opacity not 0 or 1, a NULL buffer with total > 0. */
int gs_adc_gather(gs_ctx* ctx, int total, int K, const float* xyz, const float* features_dc, const float* features_rest,
                  const float* scales, const float* rotation, const float* opacity, const int* gather_indices,
                  const int* noise_mode, const float* noise, int revised_opacity, float* out_xyz, float* out_features_dc,
                  float* out_features_rest, float* out_scales, float* out_rotation, float* out_opacity);
/* The Adam moments through the event (Inria's _prune_optimizer / cat_tensors_to_optimizer; the reference re-creates the
 * optimizer state instead, GaussianTrainer.swift:1104-1109): for each of the six tensors t of one moment arena, in the order
 * xyz, features_dc, features_rest, scales, rotation, opacity (rows of 3, 3, 3 (K - 1), 3, 4, 1 floats),
 *   out[t][j,:] = noise_mode[j] == 0 && actions[gather_indices[j]] != 1 ? in[t][gather_indices[j],:] : 0
 * -- a kept Gaussian and a clone's original keep their rows bit for bit, both children of a split and a clone's copy start at
 * zero.  Called once for the first and once for the second moments.  in / out: HOST arrays of six DEVICE pointers (entry 2
 * may be NULL when K = 1).  GS_ERR_INVALID_ARG: total < 0, K < 1, a NULL table, a NULL buffer with total > 0. */
int gs_adc_gather_moments(gs_ctx* ctx, int total, int K, const int* gather_indices, const int* noise_mode, const int* actions,
                          const float* const in[6] /*HOST*/, float* const out[6] /*HOST*/);
/* The opacity reset (Inria's reset_opacity): opacity[i] = min(opacity[i], logit(reset_value)) on the raw values -- which is
 * inverse_sigmoid(min(sigmoid(o), reset_value)) --, and the opacity segment's two moments m_opacity, v_opacity set to 0.
 * GS_ERR_INVALID_ARG: N < 0, reset_value not in (0, 1), a NULL buffer with N > 0. */
int gs_adc_reset_opacity(gs_ctx* ctx, int N, float* opacity, float* m_opacity, float* v_opacity, float reset_value);

/* ---- next row: snapshot format ---------------------------------------------------------------
 * Data/PlyWriter.swift: binary little-endian PLY, header comment `features_rest_shape M 3`, vertex = x y z,
 * f_dc_0..2, f_rest_0..3M-1 (coefficient-major, channel-minor: [M][3] flattened, NOT INRIA's channel-major),
 * opacity, scale_0..2, rot_0..3 -- all raw (pre-activation) float32.  Tensors are DEVICE pointers; the file is
 * byte-identical to the reference writer's for the same values. [sync] */

/* PlyWriter.writeGaussianBinary (:22-113, :116-146).  Creates missing parent directories (:106-111). */
int gs_ply_write(gs_ctx* ctx, const char* path, int N, int K, const float* xyz, const float* features_dc,
                 const float* features_rest, const float* opacity, const float* scales, const float* rotation);
/* Header of loadGaussianBinaryPLY (:149-183): vertex count and the features_rest_shape comment. */
int gs_ply_probe(gs_ctx* ctx, const char* path, long long* N, int* M, int* D);
/* loadGaussianBinaryPLY (:149-233) into caller buffers sized from gs_ply_probe (K = M + 1; D must be 3).  Fields
 * are found by name, in whatever order the header lists its `property float` lines (:171-176, :189). */
int gs_ply_load(gs_ctx* ctx, const char* path, int N, int K, float* xyz, float* features_dc, float* features_rest,
                float* opacity, float* scales, float* rotation);
/* The device half of the writer alone: rows[N, 14 + 3(K-1)] in the file's vertex layout (for callers with their own
 * IO, e.g. streaming a snapshot to a viewer). */
int gs_ply_pack_rows(gs_ctx* ctx, int N, int K, const float* xyz, const float* features_dc,
                     const float* features_rest, const float* opacity, const float* scales, const float* rotation,
                     float* rows);

/* ---- next row: point-cloud initialisation -----------------------------------------------------
 * distTopK (Trainer/GaussianModel.swift:11-31): for the query points [q_begin, q_begin + q_count) of xyz[N,3], the
 * mean of the k (1..8) smallest squared distances to all N points, the point itself included; other entries of
 * out[N] are left untouched.  The reference's loop visits only the 256-point chunks starting at multiples of 256
 * below N/256 + 1 (stride bug, :13-18) and leaves the rest 0; the host mirror (model_init.py) reproduces that by
 * choosing the query ranges, or covers every point on request. */
int gs_dist_topk(gs_ctx* ctx, int N, int k, int q_begin, int q_count, const float* xyz, float* out);

/* ---- instrumentation ----------------------------------------------------------------------------------- */

/* Per-stage device time, measured with HIP events recorded on the ctx stream around each stage. */
typedef enum gs_stage {
    GS_STAGE_PROJ_FWD = 0,
    GS_STAGE_BIN = 1,
    GS_STAGE_BLEND_FWD = 2,
    GS_STAGE_LOSS = 3,
    GS_STAGE_BLEND_BWD = 4,
    GS_STAGE_PROJ_BWD = 5,
    GS_STAGE_ADAM = 6,
    GS_STAGE_DISTORTION_BWD = 7,   /* the armed distortion backward (gs_arm_distortion); it runs inside GS_STAGE_BLEND_BWD's
                                      interval, which then includes it */
    GS_STAGE_COUNT = 8
} gs_stage;
/* stage_mask: bit s set = record stage s (clears what was recorded); 0 = stop.  Each recorded stage costs two
 * event packets on the stream (a few microseconds of serialisation each), so time only what is needed. */
int gs_profile_enable(gs_ctx* ctx, unsigned stage_mask);
/* Sum of elapsed ms and number of recorded calls per stage since gs_profile_enable(1). [sync] */
int gs_profile_read(gs_ctx* ctx, float ms[GS_STAGE_COUNT] /*HOST*/, int calls[GS_STAGE_COUNT] /*HOST*/);

/* Last forward's workload statistics, read back from the device. [sync]
 * stats[0]=N_visible stats[1]=M stats[2]=max tile list stats[3]=sum over pixels of nContrib (low 32 bits)
 * stats[4]=high 32 bits of that sum, stats[5]=overflow flag. */
int gs_last_stats(gs_ctx* ctx, uint32_t stats[8] /*HOST*/);
/* Per-view block-work buffer for the following gs_render_forward calls (16x16 tiles and block lists; ignored otherwise).
 * The forward's time is set by its longest serial lists, and where a block's list stops cannot be predicted from
 * its length -- but a previous forward of (nearly) the same view has measured it.  buf: DEVICE u32
 * [gs_block_count], caller-owned, zero-filled before its first use, one per training view, valid until replaced or
 * cleared (NULL = the ctx's own scratch, no hint).  Each forward first reads it as the hint (deepest blocks are
 * started first) and then overwrites it with its own measurement (max nContrib per block), which the matching
 * backward consumes.  Changes the launch order only, never a result. */
int gs_set_block_work_buffer(gs_ctx* ctx, uint32_t* buf);
/* The same buffer with room for per-tile DEPTH CUTS behind the block-work words: buf DEVICE u32
 * [gs_view_hint_words], zero-filled before its first use, one per training view.  With 16x16 tiles the backward
 * then records, per tile, the depth key up to which this view's forward needed the tile's list (sweep length + 25 %
 * + 64 entries), and the next forward of the view bins a (Gaussian, tile) pair only if the Gaussian's key does not
 * exceed it.  Tile lists are in key order, so what is binned is a prefix of the reference's list
 * (GaussianRenderer.swift:333-490 bins everything; most of it is never reached once a tile saturates).
 * Exactness: a tile under a cut whose pixels have not all reached T < 1e-4 at the end of its list marks the forward
 * as MISSED.  The caller must ask gs_forward_missed after each gs_render_forward under cuts and, when it says 1,
 * repeat the forward with gs_set_depth_cuts(ctx, 0) (then re-enable) before using any output: a forward that did not
 * miss is identical to the uncut one, output for output.  Block lists (gs_ctx_create): the same per block.  Tile sizes
 * that are multiples of 16 other than 16x16: work hint only, no cuts. */
int gs_view_hint_words(gs_ctx* ctx, int* n);
int gs_set_view_hints(gs_ctx* ctx, uint32_t* buf, int words);
/* Forgets the cuts kept in a view's hint buffer (its work hint stays): call it for every view after the model was
 * rebuilt (densify / prune) -- a stale cut costs a repeated forward, a missing one only a full binning pass. */
int gs_clear_depth_cuts(gs_ctx* ctx, uint32_t* buf, int words);
/* Depth cuts on (default) / off for the following forwards; without a gs_set_view_hints buffer there are none. */
int gs_set_depth_cuts(gs_ctx* ctx, int enable);
/* *missed = 1 if the last gs_render_forward ran under cuts and has to be repeated without them.  Waits for that
 * forward (not for anything queued behind it) when it ran under cuts; immediate otherwise. [sync on the forward] */
int gs_forward_missed(gs_ctx* ctx, int* missed /*HOST*/);
/* After gs_forward_missed on a forward under cuts: out[0] = pairs binned, out[1] = pairs a full binning would have
 * made (both 0 when the forward ran without cuts).  For the caller's policy: the cuts cost a fixed ~40 us per forward
 * (second expansion pass, the wait above, an occasional repeat) and save ~13 us per million pairs left out. */
int gs_cut_stats(gs_ctx* ctx, uint32_t out[2] /*HOST*/);
/* Densification statistic fused into the backward (GaussianTrainer.swift:724-742, accum_grad_norm): when set,
 * gs_render_backward / _dp_finish add |grad_xyz[i,:]| to accum[i] (DEVICE f32 [N], caller-owned; NULL = off).
 * Same arithmetic as gs_accum_grad_norm, one launch fewer per step. */
int gs_set_grad_norm_accum(gs_ctx* ctx, float* accum);
/* The overflow word of the last forward (1 = its pairs exceeded the reserve), copied to a caller device word on the
 * stream: for hosts that make a decision collective, e.g. data-parallel ranks that all-reduce (max) the words of a
 * step so that every replica skips the same optimizer steps. */
int gs_copy_overflow_flag(gs_ctx* ctx, uint32_t* out /*DEVICE*/);
/* The word the optimizer kernels test before they touch anything (non-zero = skip).  NULL (default) = the ctx's own
 * overflow word of the last forward.  The word must stay valid while set. */
int gs_set_update_gate(gs_ctx* ctx, const uint32_t* gate /*DEVICE*/);
/* ABI 5 -- a data-parallel step's gate WITHOUT a collective of its own (what gs_dp_step does inside; these three are for
 * hosts that issue the collectives themselves, e.g. trainer.py over torch.distributed):
 * gs_set_overflow_rider: the first kernel of the following gs_render_backward / gs_render_backward_dp[_begin] calls also
 *   stores the last forward's overflow word at dst as 0.0f / 1.0f -- e.g. at color_cot + 3 N (the word of this rank's
 *   gather block, gs_dp_cc_floats) or at grads + n_arena (summed by the all-reduce: non-zero bits = gated, so the same
 *   address serves as gs_set_update_gate's word).  NULL = off.
 * gs_set_gathered_gate: the following gs_sh_grad_from_views[_adam] calls read color_cot_all as `count` blocks of
 *   block_floats floats (rank r's cotangents at color_cot_all + r * block_floats), take the OR of the blocks' words at
 *   [3 N] as their gate and store it to reduced_out (DEVICE; typically gs_set_update_gate's word, so that the optimizer
 *   kernels queued behind them test the same).  block_floats = 0: off (blocks of 3 N floats, gs_set_update_gate's word).
 * gs_set_gate_seen: every gs_adam_step / gs_sh_grad_from_views* kernel that finds its gate raised sets *seen = 1 (a host
 *   that looks every 16th step learns that some step of the window was skipped).  NULL = off. */
int gs_set_overflow_rider(gs_ctx* ctx, float* dst /*DEVICE*/);
int gs_set_gathered_gate(gs_ctx* ctx, long long block_floats, int count, uint32_t* reduced_out /*DEVICE*/);
int gs_set_gate_seen(gs_ctx* ctx, uint32_t* seen /*DEVICE*/);

/* Launch tuning, per context (defaults are the measured optima on MI355X; results never depend on these -- GS_TUNE_FWD_FOUR_WAVES alone
 * moves them, by rounding: see there). */
typedef enum gs_tuning {
    GS_TUNE_FWD_WAVES_PER_SIMD = 0, /* persistent waves per SIMD of the fused blend forward (default 4) */
    GS_TUNE_BWD_WAVES_PER_CU = 1,   /* persistent waves per CU of the fused blend backward (default 16) */
    GS_TUNE_FWD_QUADRANTS = 2,      /* the fused forward's items are always 8x8 quadrants (the 16x8 variant of ABI 2 that 0 once
                                     * selected was 25 % slower and is gone); what is left of the knob: 0 forces the
                                     * one-wave-per-quadrant kernel where the staging-wave or the four-wave kernel would run
                                     * (as GS_TUNE_FWD_PAIR 0 and GS_TUNE_FWD_FOUR_WAVES 0 together); default 1 */
    GS_TUNE_OP_FWD_PPL = 3,         /* pixels per lane (1, 2, 4) of the op-level gs_blend_forward */
    GS_TUNE_OP_BWD_PPL = 4,         /* ... and gs_blend_backward */
    GS_TUNE_FWD_TRACE_BUFFER = 5,   /* DEVICE u64 [4 * items] (as an integer) receiving per-item start/end clocks, 0 = off */
    GS_TUNE_WIDE_TILE_SORT = 7,     /* 1 (default): the pairs are sorted by tile in one pass when the image has <= 4096 tiles;
                                     * 0: two 8-bit radix passes + range kernel (same lists, bit for bit) */
    GS_TUNE_HOST_OVERFLOW_ERRORS = 8, /* 1 (default): entry points that continue a step return GS_ERR_WORKSPACE_OVERFLOW as soon as
                                     * the host sees the flag of an overflowed forward ("Overflow" above).  0: only gs_sync
                                     * reports it -- for data-parallel hosts, where a rank that bailed out of a step on its own
                                     * would leave the others waiting in a collective: the device gate (gs_set_update_gate on
                                     * the max-reduced flags) skips the step on every rank, and the ranks decide TOGETHER when
                                     * to look (gs_sync), reserve and carry on */
    GS_TUNE_SPLITTER_DEPTH_SORT = 9, /* 1 (default): the depth sort of 16385 .. 655 k Gaussians buckets the records between 127 splitters
                                     * kept from the context's previous depth sort and sorts every bucket locally (three launches);
                                     * 0: four least-significant-digit passes (eight); 2 means 1 (it once asked for splitter buckets
                                     * above 655 k Gaussians too; those sizes always take their LSD passes).  Same order, bit for bit,
                                     * whatever the splitters are -- they only balance the buckets */
    GS_TUNE_COLOUR_RIDERS = 10,     /* 1 (default): a K = 25 forward computes its SH colours in workgroups that ride along in the binning
                                     * kernels' launches (they leave most CUs idle) instead of in the projection kernel; 0: one
                                     * projection kernel with the SH loads interleaved (rounds 1-2); 2: split, but no riders (all colours in a
                                     * kernel of their own in front of the blend); 3: one kernel, geometry first, then the wave's own
                                     * colours (what 1 does where no binning kernel can host riders).  Same colours, bit for bit */
    GS_TUNE_FWD_QUEUES = 11,        /* work queues of the fused blend forward: 8 (default) = one per XCD, the four quadrant waves of a pixel
                                     * block on one XCD so that its records are fetched into one L2; 1 = one queue for the chip,
                                     * a block's quadrants on four XCDs (rounds 1-3); 2, 4 in between */
    GS_TUNE_FWD_FOUR_WAVES = 12,    /* fused blend forward with four waves per 8x8 quadrant, each sweeping every fourth 64-entry chunk of the
                                     * list (three of them from T = 1, composed in LDS): -1 (default) = where the image has fewer
                                     * quadrants than the chip has wave slots (<= 512x512 on MI355X; there a quadrant's list is a serial
                                     * chain on a half-empty chip), 1 / 0 = always / never.  Image and gradients within the same bars,
                                     * not the same bits as the one-wave kernel (sums are composed, not accumulated, across chunks) */
    GS_TUNE_FWD_FOLD_TEST_SCALE = 13, /* TEST knob, permille (default 1000 = exactly 1): factor on the composed transmittance in the
                                     * four-wave forward's test "did this pixel cross T < 1e-4 inside the part"; a value below 1000
                                     * sends pixels that are still live through a second, sequential take of their part and the fold's
                                     * continuation behind it (the path a pixel within rounding of the threshold takes once in ~1e7).
                                     * Results stay within the bars of GS_TUNE_FWD_FOUR_WAVES (sequential instead of composed sums) */
    GS_TUNE_RENDER_ONLY = 15,       /* 1: the fused forwards of this context render and keep nothing for a backward -- no checkpoints
                                     * (a third to a half of the blend forward's bytes on deep lists), no backward preparation riding in
                                     * the loss.  gs_render_backward* of such a forward return GS_ERR_NO_FORWARD.  For previews, snapshots
                                     * of a training run, and the forward-only config of BASELINE (the reference's own forward custom
                                     * function saves nothing either: its VJP walks the lists backwards).  Same image, bit for bit */
    GS_TUNE_FWD_PAIR = 16,          /* fused blend forward with a STAGING wave beside every sweeping wave (two-wave workgroups: one loads,
                                     * culls and compacts chunk c + 1 into LDS while the other blends chunk c; one barrier per chunk):
                                     * -1 (default) = where the lists are deep (>= 4500 pairs per 16 x 16 block in the context's previous
                                     * forward: a scene grown to the schedule's cap, 0.89 -> 0.80 ms), 0 = never, 1 = always (12
                                     * workgroups per CU), 2..16 = always, with that many workgroups per CU.  The arithmetic and its order are the one-wave kernel's: same image, nContrib and
                                     * checkpoints, bit for bit.  Images small enough for GS_TUNE_FWD_FOUR_WAVES keep that kernel */
    GS_TUNE_FWD_SLOW_SLOT = 17,     /* the one-wave blend forward's persistent waves that sit in a hardware wave slot >= this value take their
                                     * static first item and nothing from the work queues (default 3; 16 = every wave pops).  gfx950's
                                     * SIMD arbiter favours its lower slots (measured: slot 3 runs at half slot 0's pace), and the launch
                                     * used to end with the slow slots' second items.  Same bits (who blends an item changes nothing) */
    GS_TUNE_TRIM_RECTS = 18,        /* 2 (default) / 1: at 16 x 16 tiles the fused forward bins a Gaussian on the tiles of the reference's 3-sigma
                                     * square (GaussianRenderer.swift get_rect, tile_rect) that the axis-aligned box of its ellipse
                                     * q <= 40.3 reaches -- beyond it the blend's staging drops the entry for every quadrant anyway
                                     * (weight < 2^-29): alpha is the untrimmed forward's bit for bit (one-wave forward), colour and depth to the rounding of
                                     * their per-chunk sums (a chunk is 64 list positions: the kept entries group differently; <= 4e-7
                                     * relative), gradients to the noise of their float atomics.  11.5 % fewer pairs to sort on the bench
                                     * scene (step 0.786 -> 0.776 ms, the scene grown to 1 M 3.02 -> 2.87).  What changes is what the fused path
                                     * reports about its lists: M (gs_last_stats), nContrib (gs_copy_last_contrib), gs_copy_block_work
                                     * and gs_tile_bin_export of a fused forward count positions in the TRIMMED lists, as they already
                                     * do under block lists.  2 cuts the box further: its tile rows in four groups, each with the columns
                                     * the ellipse reaches on the group's pixel rows (an elongated, tilted splat never sees the box's
                                     * corners: 14 % fewer pairs again on the bench scene); 1 keeps the box.  0: the reference's lists,
                                     * position for position (tests that hold M and nContrib to the oracle run with 0).  The op-level
                                     * gs_tile_bin is always the reference's */
    GS_TUNE_SH_BAND_SKIP = 19,      /* 1 (default): gs_render_backward_adam below the degree K allows takes the band-limited form of the
                                     * fused projection backward + Adam (gs_set_sh_degree).  0: the full-row form at every degree (A/B,
                                     * tests): the same active columns to the noise of the blend backward's float atomics; inactive
                                     * columns with zero moments the same bits */
    GS_TUNE_POISON_CHECKPOINTS = 14, /* TEST knob: 1 = the checkpoint arena is filled with NaN in front of every fused forward, so a
                                     * backward that reads a checkpoint lane its forward did not write shows up as NaN gradients */
    GS_TUNE_DEPTH_GRADIENT = 6      /* 1 (default): gs_render_backward* may get a cot_depth.  0: the caller promises NULL (the
                                     * default training case, GaussianTrainer.swift:280, 949: lambda_depth = 0); the forward
                                     * then saves 4 instead of 5 floats per pixel and 64 list entries, and a backward that
                                     * does bring a cot_depth is refused with GS_ERR_INVALID_ARG */
} gs_tuning;
int gs_ctx_set_tuning(gs_ctx* ctx, int knob, long long value);

/* Number of 16x16 pixel blocks of the fused path (block lists: the blocks enumerated per tile, gs_ctx_create). */
int gs_block_count(gs_ctx* ctx, int* n);
/* Copies the last fused forward's per-block sweep length (max nContrib over the block's pixels) to a device buffer. */
int gs_copy_block_work(gs_ctx* ctx, uint32_t* out);
/* Copies the last fused forward's per-pixel nContrib (u32 [H*W], the reference's lastContrib) to a device buffer. */
int gs_copy_last_contrib(gs_ctx* ctx, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_H */
