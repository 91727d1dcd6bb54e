// gs_proj_fwd_kernel.h -- the fused projection forward (projection.hip).
// POSE: the camera is *dcam, the one pose_camera_kernel composed on the device (pose refinement, gs_set_pose_correction), instead of
// the kernel argument hostCam; with COLOUR only -- no riders: the binning kernels and colour_rest_kernel see only the host camera.
// dcam is the last argument, so that the others keep the offsets they had: the unposed forms compile to the registers they did.
// AA: the anti-aliased mode (gs_set_antialiasing): the packed opacity is sigma(o) rho (aa_opacity_scale, gs_math.h).
// F3D: the 3-D smoothing filter (gs_set_filter3d): the scales are sqrt(s^2 + f^2), f = filter3d[p], and the opacity gains kappa
// (filter3d_activate, gs_math.h).  The other instantiations never read filter3d, the argument before dcam.
// FISHEYE: the equidistant camera model (gs_set_camera_model; project_geometry's FISHEYE, gs_math.h); never with POSE or F3D.
// The forms that exist: {riders' geometry, SELF, one kernel in one or two phases, the same posed} x AA x F3D (24);
// fisheye: {riders' geometry, SELF, one kernel in one or two phases} x AA (8)
constexpr bool proj_fwd_form_exists(bool TWO_PHASE, bool COLOUR, bool SELF, bool POSE, bool F3D = false, bool FISHEYE = false)
{
    return (COLOUR ? !SELF : (TWO_PHASE && !POSE)) && (!FISHEYE || (!POSE && !F3D));
}

template <bool TWO_PHASE, bool COLOUR, bool SELF, bool AA, bool F3D, bool POSE, bool FISHEYE = false>
__global__ __launch_bounds__(PROJ_FUSED_THREADS) void proj_fwd_fused_kernel(
    int N, int K, int degree, CamParams hostCam, int tileW, int tileH, int gridW, int gridH,
    const float* __restrict__ xyz, const float* __restrict__ fdc, const float* __restrict__ frest,
    const float* __restrict__ scalesRaw, const float* __restrict__ rotRaw, const float* __restrict__ opacityRaw,
    float* __restrict__ packed12, float* __restrict__ radiiOut, ushort4* __restrict__ tileRect,
    uint32_t* __restrict__ tilesTouched, uint32_t* __restrict__ depthKey, uint32_t* __restrict__ depthVal,
    uint32_t* __restrict__ visPerBlock, uint32_t* __restrict__ counters, int flags, ColourRider self,
    GsVirtGeom vg, GsCutCoarse cc, uint4* __restrict__ tilePieces, const float* __restrict__ filter3d,
    const CamParams* __restrict__ dcam)
{
    static_assert(proj_fwd_form_exists(TWO_PHASE, COLOUR, SELF, POSE, F3D, FISHEYE), "no such form of the fused projection forward");
    CamParams posed;
    if constexpr (POSE) posed = *dcam;
    const CamParams& cam = POSE ? posed : hostCam;
    const int noKeyForUntouched = flags & 1;
    const bool trimRects = (flags & 2) && !vg.nbx && tileW == 16 && tileH == 16;
    extern __shared__ float shLds[];
    __shared__ uint32_t sDropped;
    if (cc.superCut) {           // (uniform)
        if (threadIdx.x == 0) sDropped = 0u;
        __syncthreads();
    }
    // first kernel of a forward: clears the ctx counters for the kernels behind it (no memset launch)
    if (blockIdx.x == 0 && threadIdx.x < GS_CNT_COUNT) counters[threadIdx.x] = 0;
    const int p = blockIdx.x * PROJ_FUSED_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = (K - 1) * 3;
    // K = 25 (L = 72): the rows go through LDS in two halves of 12 coefficients (see sh_half_load); otherwise whole
    const bool twoPhase = TWO_PHASE;
    const int LH = L >> 1, kSplit = 1 + (K - 1) / 2;          // second half starts at coefficient kSplit
    const int rowW = twoPhase ? LH + 1 : L + 1;
    float* myRows = shLds + wv * 64 * rowW;
    const int row0 = blockIdx.x * PROJ_FUSED_THREADS + wv * 64;
    const int rows = min(64, N - row0);
    float4 halfB[SH_HALF_MAX4];
    if (COLOUR && rows > 0 && L > 0) {
        if (twoPhase) {
            float4 halfA[SH_HALF_MAX4];
            sh_half_load(frest + (size_t)row0 * L, rows, L, 0, LH, lane, halfA);
            sh_half_load(frest + (size_t)row0 * L, rows, L, LH, LH, lane, halfB);
            sh_half_to_lds(myRows, rows, LH, lane, halfA);
        } else {
            sh_rows_in(myRows, frest + (size_t)row0 * L, rows, L, lane);
        }
    }
    // each wave reads back only what it staged itself: DS operations of one wave complete in order
    bool visible = false;
    uint32_t myTouched = 0;       // (SELF)
    ProjOut o;
    float opacity = 0.f, colA[3] = {0.f, 0.f, 0.f}, dirv[3] = {0.f, 0.f, 0.f};
    if (p < N) {
        const float m[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
        const float s[3] = {expf(scalesRaw[3 * p]), expf(scalesRaw[3 * p + 1]), expf(scalesRaw[3 * p + 2])};
        const float r0 = rotRaw[4 * p], r1 = rotRaw[4 * p + 1], r2 = rotRaw[4 * p + 2], r3 = rotRaw[4 * p + 3];
        const float den = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3) + 1e-8f;
        const float q[4] = {r0 / den, r1 / den, r2 / den, r3 / den};
        opacity = 1.0f / (1.0f + expf(-opacityRaw[p]));
        if constexpr (F3D) {
            float se[3];
            opacity *= filter3d_activate(s, filter3d[p], se);
            project_geometry(m, se, q, cam, o);
        } else
        project_geometry<FISHEYE>(m, s, q, cam, o);
        // A 2-D covariance whose float32 determinant is not positive -- the true one always is (the +0.3 blur), so this is
        // cancellation: a needle tens of thousands of pixels long, cov2d = (4.2e7, -3.8e7; -3.8e7, 3.5e7) -- has a conic that is not
        // positive definite: q < 0 without bound, "weights" above 1, a 0.99-alpha blob over its whole 3-sigma square.  The reference's
        // training kernels have no guard (slang/gaussian_projection_screen_shared.slang:248-254; its viewer's shaders do:
        // Metal/GaussianRender.metal:153-154), and there the splat's gradients are 0 x inf = NaN, which takes it out of the picture for
        // good.  Here it is out of the picture while it is degenerate: radius 0, not binned, zero gradient (the fused path's second
        // deliberate deviation; the op-level gs_projection_forward keeps the 1:1 arithmetic).
        if (GS_DEGENERATE_INVISIBLE && !(o.cov2d[0] * o.cov2d[3] - o.cov2d[1] * o.cov2d[2] > 0.0f)) o.radius = 0.0f;
        if constexpr (AA) {     // (rho = 0: det Sigma not > 0 -- invisible while it is so, as above)
            const float rho = aa_opacity_scale(o.cov2dRaw, o.cov2d);
            opacity *= rho;
            if (!(rho > 0.0f)) o.radius = 0.0f;
        }

        const float x = m[0] - cam.cam[0], y = m[1] - cam.cam[1], z = m[2] - cam.cam[2];
        const float* d0 = fdc + (size_t)p * 3;
        const float* rest = myRows + lane * rowW;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (!COLOUR) {
        } else if (!twoPhase) {
            sh_foreach(degree, x, y, z, [&](int k, float b, float, float, float) {
                if (k == 0) { c0 = b * d0[0]; c1 = b * d0[1]; c2 = b * d0[2]; }
                else {
                    const float* r = rest + (k - 1) * 3;
                    c0 += b * r[0]; c1 += b * r[1]; c2 += b * r[2];
                }
            });
        } else {
            // same sum, same order (k ascending); coefficients 1 .. kSplit-1 are staged now
            sh_foreach(degree, x, y, z, [&](int k, float b, float, float, float) {
                if (k == 0) { c0 = b * d0[0]; c1 = b * d0[1]; c2 = b * d0[2]; }
                else if (k < kSplit) {
                    const float* r = rest + (k - 1) * 3;
                    c0 += b * r[0]; c1 += b * r[1]; c2 += b * r[2];
                }
            });
        }
        colA[0] = c0; colA[1] = c1; colA[2] = c2;
        dirv[0] = x; dirv[1] = y; dirv[2] = z;
        }
        if (COLOUR && twoPhase && rows > 0 && L > 0) sh_half_to_lds(myRows, rows, LH, lane, halfB);     // the wave's first half is consumed
        if (p < N) {
        float c0 = colA[0], c1 = colA[1], c2 = colA[2];
        if (COLOUR && twoPhase) {
            const float* rest = myRows + lane * rowW;
            sh_foreach(degree, dirv[0], dirv[1], dirv[2], [&](int k, float b, float, float, float) {
                if (k >= kSplit) {
                    const float* r = rest + (k - kSplit) * 3;
                    c0 += b * r[0]; c1 += b * r[1]; c2 += b * r[2];
                }
            });
        }
        // 12th float: per channel, which side of the max(., 0) the colour fell on (2 bits: 0 below, 1 tie, 2 above), so
        // that the colour cotangent can be gated right after the blend backward (color_cot_kernel)
        uint32_t gate = 0u;
        if (COLOUR) {
            c0 += 0.5f; c1 += 0.5f; c2 += 0.5f;
            gate = colour_gate(c0, c1, c2);
        }

        float4* out = reinterpret_cast<float4*>(packed12 + (size_t)p * 12);
        out[0] = make_float4(o.sx, o.sy, o.conic[0], o.conic[1]);
        out[1] = make_float4(o.conic[2], o.conic[3], c0, c1);
        out[2] = make_float4(c2, opacity, o.depth, __uint_as_float(gate));
        if (radiiOut) radiiOut[p] = o.radius;

        uint32_t touched = 0;
        ushort4 tr = make_ushort4(0, 0, 0, 0);
        uint32_t pc[4] = {0u, 0u, 0u, 0u};      // (trimmed rects: the rect's four row groups, first column | columns << 16)
        if (o.radius > 0.0f) {
            int x0, y0, x1, y1;
            if (vg.nbx)        // block lists: tileW .. gridH describe the grid of 16 x 16 blocks enumerated per tile
                block_rect_of_splat(o.rect, o.sx, o.sy, o.cov2d[0], o.cov2d[3], vg.nbx, vg.nby, vg.tw, vg.th, gridW / vg.nbx,
                                    gridH / vg.nby, (int)cam.W, (int)cam.H, x0, y0, x1, y1);
            else if (trimRects)   // 16 x 16 tiles, GS_TUNE_TRIM_RECTS: the reference's 3-sigma square cut by the box of q <= 40.3, beyond
                                  // which the blend's staging drops the entry for every quadrant anyway (block_rect_of_splat)
                block_rect_of_splat(o.rect, o.sx, o.sy, o.cov2d[0], o.cov2d[3], 1, 1, 16, 16, gridW, gridH, (int)cam.W, (int)cam.H,
                                    x0, y0, x1, y1);
            else
                tile_rect(o.rect[0], o.rect[1], o.rect[2], o.rect[3], tileW, tileH, gridW, gridH, x0, y0, x1, y1);
            touched = (uint32_t)((x1 - x0) * (y1 - y0));
            // ... and inside that box only the columns the ellipse reaches, row group by row group (rect_row_groups4)
            if (trimRects && tilePieces && touched)
                touched = rect_row_groups4(o.sx, o.sy, o.cov2d[0], o.cov2d[1], o.cov2d[3], x0, y0, x1, y1, (int)cam.H, pc);
            tr = make_ushort4((unsigned short)x0, (unsigned short)y0, (unsigned short)x1, (unsigned short)y1);
            visible = true;
            // A view under depth cuts: a Gaussian that lies beyond the deepest cut of every 4 x 4 tiles its rect touches would
            // lose all its pairs in the cut expansion one by one (binning.hip, cut_super_kernel).  Dropped here it touches no
            // tile at all: no SH rows fetched for its colour, no candidates enumerated, its depth key sorted behind the rest.
            // Exact as the cuts are: a forward that needed more is detected and repeated without them.
            if (cc.superCut && touched) {
                const uint32_t key = __float_as_uint(o.depth);
                bool reach = false;
                const int sx1 = (x1 - 1) / GS_CUT_SUPER, sy1 = (y1 - 1) / GS_CUT_SUPER;
                for (int sy = y0 / GS_CUT_SUPER; sy <= sy1 && !reach; sy++)
                    for (int sx = x0 / GS_CUT_SUPER; sx <= sx1; sx++)
                        if (key <= 0xFFFFFFFFu - cc.superCut[sy * cc.superW + sx]) { reach = true; break; }
                if (!reach) { atomicAdd(&sDropped, touched); touched = 0; tr = make_ushort4(0, 0, 0, 0); pc[0] = pc[1] = pc[2] = pc[3] = 0u; }
            }
        }
        tileRect[p] = tr;
        if (trimRects && tilePieces) tilePieces[p] = make_uint4(pc[0], pc[1], pc[2], pc[3]);
        tilesTouched[p] = touched;
        myTouched = touched;
        depthKey[p] = (touched || !noKeyForUntouched) ? __float_as_uint(o.depth) : GS_SORT_NO_KEY;     // binning.hip, bin_prep_kernel
        depthVal[p] = (uint32_t)p;
    }
    // visible count: one plain store per block, summed when somebody asks (gs_last_stats).  A same-address atomic per
    // wave here cost a third of the kernel (4700 atomics on one counter: 82 -> 55 us).
    const int nvis = __syncthreads_count(visible);
    if (threadIdx.x == 0) visPerBlock[blockIdx.x] = (uint32_t)nvis;
    if (cc.superCut && threadIdx.x == 0) cc.dropPerBlock[blockIdx.x] = sDropped;       // (behind the barrier of the count above)
    // (every lane reads tilesTouched / writes the colour floats of ITS OWN record: program order is all that is needed)
    if (SELF) colour_rider_wave(self, blockIdx.x * (PROJ_FUSED_THREADS / 64) + wv, shLds + wv * 64 * GS_RIDER_ROW, lane, (int)myTouched);
}
