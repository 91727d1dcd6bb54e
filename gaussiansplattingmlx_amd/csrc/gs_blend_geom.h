// gs_blend_geom.h -- what the op-level blend kernels (blend.hip), the contribution pass (contrib.hip) and the feature pass
// (features.hip) share: the enumeration of the 16x16 pixel blocks, the forward's exponential and the alpha of a Gaussian on a pixel
#pragma once
#include <hip/hip_runtime.h>
#include "gs_ctx.h"

namespace gs {

constexpr int TILE = 16;

// Which 16x16 pixel block is work item `blk`, which tile's list does it sweep, and where do its pixels end?
// Tile sizes that are multiples of 16: the blocks of the image grid, row-major (blocksX per row); every block lies in
// one tile.  Any other tile size (the reference app's W/4 x H/4 = 200 x 200, Data/ColmapDataLoader.swift:495-498): the
// blocks are enumerated PER TILE -- bptX x bptY of them, clipped at the tile's right and bottom edge -- so that a
// block never straddles two tiles and the same LDS-staged kernels serve every tile size (the first builds ran these
// sizes one thread per pixel from global memory with per-pixel atomics: 425 ms per backward at 800x800 / 200x200).
struct BlockGeom {
    int W, H, tileW, tileH, gridW, blocksX, bptX, bptY;      // bptX == 0: image-grid enumeration
};
struct BlockRect {
    int tile, x0, y0, xEnd, yEnd;
};
__device__ __forceinline__ BlockRect block_rect(const BlockGeom& g, int blk)
{
    BlockRect r;
    if (g.bptX == 0) {
        const int by = blk / g.blocksX, bx = blk - by * g.blocksX;
        r.x0 = bx * TILE; r.y0 = by * TILE; r.xEnd = g.W; r.yEnd = g.H;
        r.tile = (r.y0 / g.tileH) * g.gridW + r.x0 / g.tileW;
    } else {
        const int per = g.bptX * g.bptY;
        r.tile = blk / per;
        const int rem = blk - r.tile * per, by = rem / g.bptX, bx = rem - by * g.bptX;
        const int ty = r.tile / g.gridW, tx = r.tile - ty * g.gridW;
        r.x0 = tx * g.tileW + bx * TILE; r.y0 = ty * g.tileH + by * TILE;
        r.xEnd = min(g.W, (tx + 1) * g.tileW); r.yEnd = min(g.H, (ty + 1) * g.tileH);
    }
    return r;
}

// The three ways the passes over the lists of the last binning (contrib.hip, features.hip) enumerate the 16x16 blocks: the
// op-level kernels' (block_rect: the image grid, or per tile for tile sizes that are not multiples of 16), and the fused path's
// block lists (gs_block_pixels: every block has a list of its own).
struct ContribGeom {
    BlockGeom g;
    GsVirtGeom virt;             // virt.nbx != 0: block lists (g.blocksX = g.gridW = blocks per row, g.tileW = g.tileH = 16)
};

__device__ __forceinline__ BlockRect contrib_rect(const ContribGeom& cg, int blk)
{
    if (cg.virt.nbx == 0) return block_rect(cg.g, blk);
    BlockRect r;
    const int by = blk / cg.g.blocksX, bx = blk - by * cg.g.blocksX;
    gs_block_pixels(cg.virt, bx, by, cg.g.W, cg.g.H, r.x0, r.y0, r.xEnd, r.yEnd);
    r.tile = by * cg.g.gridW + bx;
    return r;
}

// ... in the geometry the context describes at the time of the call (the caller's tile grid for the op-level form; the fused
// path's own -- block lists included -- behind a fused forward); the number of blocks (0: nothing to sweep)
inline int contrib_geom(const gs_ctx* c, ContribGeom& cg)
{
    cg.g.W = c->W; cg.g.H = c->H; cg.g.tileW = c->tileW; cg.g.tileH = c->tileH; cg.g.gridW = c->gridW;
    cg.g.blocksX = c->virt.nbx ? c->blocksX : gs_div_up(c->W, TILE);
    cg.g.bptX = c->fast16 ? 0 : gs_div_up(c->tileW, TILE);
    cg.g.bptY = c->fast16 ? 0 : gs_div_up(c->tileH, TILE);
    cg.virt = c->virt;
    return c->virt.nbx ? c->numPixBlocks : c->opBlocks;
}

// exp(x), x <= 0, for the FORWARD kernels: v_exp_f32 on the rounded product x log2(e) is off by |x log2 e| 2^-24 relative
// (3.4e-4 on rendered colours of magnitude ~27); carrying the product's rounding error and log2(e)'s tail along brings it
// to ~1 ulp at four more instructions (blend_v2.hip, gauss_alpha_raw).
__device__ __forceinline__ float comp_exp(float x)
{
    constexpr float L2E = 1.44269502162933349609375f, L2E_TAIL_LN2 = 1.3349758e-08f, LN2 = 0.69314718055994531f;
    const float hi = x * L2E;
    const float lo = fmaf(x, L2E, -hi);
    const float d = fmaf(x, L2E_TAIL_LN2, lo * LN2);
    const float g = __builtin_amdgcn_exp2f(hi);
    return fmaf(g, d, g);
}

// alpha of one Gaussian on one pixel (tileGlobalAlphaFromGaussian), with the terms the backward step needs again.
// a: mx my c00 c01, b: c10 c11 .. of the record.  COMP: comp_exp (the forwards, the contribution pass) or __expf (the backward step).
struct SplatAlpha {
    float dx, dy, dxdy, ex, raw, alpha;
};
template <bool COMP>
__device__ __forceinline__ SplatAlpha splat_alpha(float px, float py, const float4& a, const float4& b, float opacity)
{
    SplatAlpha s;
    s.dx = px - a.x; s.dy = py - a.y;
    s.dxdy = s.dx * s.dy;
    const float e = -0.5f * (s.dx * s.dx * a.z + s.dy * s.dy * b.y + s.dxdy * a.w + s.dxdy * b.x);
    s.ex = COMP ? comp_exp(e) : __expf(e);
    s.raw = s.ex * opacity;
    s.alpha = s.raw > 0.99f ? 0.99f : s.raw;
    return s;
}

}  // namespace gs
