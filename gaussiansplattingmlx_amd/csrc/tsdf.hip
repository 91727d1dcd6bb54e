// tsdf.hip -- mesh extraction (include/gsplat.h gs_tsdf_*): depth images fused into a truncated signed
// distance volume, and marching tetrahedra on the Kuhn split.  Compiled with -ffp-contract=off: voxel membership and the pixel a
// voxel reads are integer decisions taken from float arithmetic, and every product and sum below rounds where it is written,
// the order tests/tsdf_numpy.py restates in float32.
//
//   tsdf_integrate_kernel   one lane per lattice point, consecutive lanes along x (a wave loads and stores 256 contiguous bytes
//                           of tsdf and of weight); the voxel's state stays in registers across the call's views, which travel
//                           by value in the kernel's arguments.  No LDS, no atomics, no data-dependent loop.
//   tsdf_mark_kernel        one lane per cell: marks the lattice edges its valid tetrahedra cross (same-valued byte stores into
//                           a zeroed array -- several cells share an edge) and counts its triangles
//   tsdf_compact_kernel     a lattice point's 7 flags -> one mask byte and its vertex count
//   tsdf_tile_sums / tsdf_tile_scan / tsdf_scan_apply    exclusive scan in densify.hip's shape: per-tile sums, one block over
//                           the tiles carrying a 64-bit total, per-tile apply
//   tsdf_vertices_kernel    one lane per lattice point: the vertices on the edges it owns
//   tsdf_faces_kernel       one lane per cell: its triangles, vertex ids looked up through the owners' masks and offsets
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gs_ctx.h"

namespace gs {

constexpr int TSDF_THREADS = 256;
constexpr int TSDF_SCAN_ITEMS = 4;
constexpr int TSDF_SCAN_TILE = TSDF_THREADS * TSDF_SCAN_ITEMS;      // tests/test_gpu_tsdf.py restates these two
constexpr long long TSDF_MAX_POINTS = 1ll << 28;
constexpr int TSDF_MAX_DIM = 1024;

struct TsdfGrid {
    float ox, oy, oz, voxel;
    int nx, ny, nz, n;
    float trunc;
};

struct TsdfView {
    float Rt[12];
    float fx, fy, cx, cy;
    float uMax, vMax;      // width - 1, height - 1
    int width;
    const float* depth;
    const float* color;
};

struct TsdfIntegrateArgs {
    TsdfGrid g;
    int nViews;
    TsdfView v[GS_TSDF_MAX_VIEWS];
};

__device__ __forceinline__ void tsdf_ijk(const TsdfGrid& g, int n, int& i, int& j, int& k)
{
    const int r = n / g.nx;
    i = n - r * g.nx;
    k = r / g.ny;
    j = r - k * g.ny;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(const TsdfIntegrateArgs A, float* __restrict__ tsdf,
                                                                      float* __restrict__ weight, float* __restrict__ rgb,
                                                                      float* __restrict__ cweight)
{
    const int n = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= A.g.n) return;
    int i, j, k;
    tsdf_ijk(A.g, n, i, j, k);
    const float px = A.g.ox + A.g.voxel * (float)i, py = A.g.oy + A.g.voxel * (float)j, pz = A.g.oz + A.g.voxel * (float)k;
    float f = tsdf[n], w = weight[n];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cw = 0.0f;
    if (rgb) { c0 = rgb[3 * (size_t)n]; c1 = rgb[3 * (size_t)n + 1]; c2 = rgb[3 * (size_t)n + 2]; cw = cweight[n]; }
    bool touched = false, coloured = false;
    const float trunc = A.g.trunc;
    for (int vi = 0; vi < A.nViews; vi++) {
        const TsdfView& V = A.v[vi];
        const float x = ((V.Rt[0] * px + V.Rt[1] * py) + V.Rt[2] * pz) + V.Rt[3];
        const float y = ((V.Rt[4] * px + V.Rt[5] * py) + V.Rt[6] * pz) + V.Rt[7];
        const float z = ((V.Rt[8] * px + V.Rt[9] * py) + V.Rt[10] * pz) + V.Rt[11];
        if (!(z > 0.0f && z < INFINITY)) continue;
        const float u = V.fx * (x / z) + V.cx, v = V.fy * (y / z) + V.cy;
        const float fu = floorf(u), fv = floorf(v);
        // (compared as floats, before any conversion: a NaN or an out-of-range position fails a test and reads nothing)
        if (!(fu >= 0.0f && fu <= V.uMax && fv >= 0.0f && fv <= V.vMax)) continue;
        const size_t pix = (size_t)(int)fv * V.width + (int)fu;
        const float d = V.depth[pix];
        if (!(d > 0.0f && d < INFINITY)) continue;
        const float s = d - z;
        if (s < -trunc) continue;
        const float val = fminf(1.0f, s / trunc);
        f = (f * w + val) / (w + 1.0f);
        w = w + 1.0f;
        touched = true;
        if (rgb && V.color && s <= trunc) {
            const float* c = V.color + 3 * pix;
            c0 = (c0 * cw + c[0]) / (cw + 1.0f);
            c1 = (c1 * cw + c[1]) / (cw + 1.0f);
            c2 = (c2 * cw + c[2]) / (cw + 1.0f);
            cw = cw + 1.0f;
            coloured = true;
        }
    }
    if (touched) { tsdf[n] = f; weight[n] = w; }
    if (coloured) { rgb[3 * (size_t)n] = c0; rgb[3 * (size_t)n + 1] = c1; rgb[3 * (size_t)n + 2] = c2; cweight[n] = cw; }
}

// ---- the Kuhn split ---------------------------------------------------------------------------------------------------------
// A cell corner is a 3-bit code (x = 1, y = 2, z = 4).  Tetrahedron t is the path 0 -> 7 adding the axes in the t-th permutation
// (lexicographic); path corners 0 .. 3.  Tetrahedra 1, 2 and 5 are the odd permutations.
__device__ constexpr int TET_CODE[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ constexpr bool TET_ODD[6] = {false, true, true, false, false, true};
__device__ constexpr int SLOT_OF_BITS[8] = {-1, 0, 1, 3, 2, 4, 5, 6};      // the slot of the edge towards a direction code
__device__ constexpr int DIR_OF_SLOT[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ constexpr int TET_EDGE_A[6] = {0, 0, 0, 1, 1, 2}, TET_EDGE_B[6] = {1, 2, 3, 2, 3, 3};   // edge ids 0 .. 5
// The triangles of an even tetrahedron per case (bit c = path corner c inside), as edge ids, 3 bits each, triangle 0 in the low 9
// bits; an odd tetrahedron takes case ^ 15.  Derived from the rule in include/gsplat.h; tests/tsdf_numpy.py derives it again
// from that rule (case_table) and the GPU tests compare the meshes index for index.
constexpr uint32_t tet_case(int a, int b, int c, int d = 0, int e = 0, int f = 0)
{
    return (uint32_t)(a | (b << 3) | (c << 6) | (d << 9) | (e << 12) | (f << 15));
}
__device__ constexpr uint32_t TET_CASES[16] = {
    0u, tet_case(0, 1, 2), tet_case(0, 4, 3), tet_case(1, 2, 4, 1, 4, 3), tet_case(1, 3, 5), tet_case(0, 3, 5, 0, 5, 2),
    tet_case(0, 4, 5, 0, 5, 1), tet_case(4, 5, 2), tet_case(2, 5, 4), tet_case(0, 1, 5, 0, 5, 4), tet_case(0, 2, 5, 0, 5, 3),
    tet_case(5, 3, 1), tet_case(1, 3, 4, 1, 4, 2), tet_case(3, 4, 0), tet_case(2, 1, 0), 0u};

__device__ __forceinline__ int tsdf_code_offset(const TsdfGrid& g, int code)
{
    return (code & 1) + g.nx * (((code >> 1) & 1) + g.ny * ((code >> 2) & 1));
}

__device__ __forceinline__ bool tsdf_is_cell(const TsdfGrid& g, int n)
{
    int i, j, k;
    tsdf_ijk(g, n, i, j, k);
    return i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
}

// bit c of `inside`: corner code c has tsdf < 0; of `seen`: weight >= minWeight
__device__ __forceinline__ void tsdf_cell_bits(const TsdfGrid& g, int n, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                               float minWeight, int& inside, int& seen)
{
    inside = 0; seen = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int m = n + tsdf_code_offset(g, c);
        inside |= (tsdf[m] < 0.0f ? 1 : 0) << c;
        seen |= (weight[m] >= minWeight ? 1 : 0) << c;
    }
}

// the case of tetrahedron t (0 or 15: no triangle; also for one that is not emitted)
template <int t>
__device__ __forceinline__ int tsdf_tet_case(int inside, int seen)
{
    constexpr int all = (1 << TET_CODE[t][0]) | (1 << TET_CODE[t][1]) | (1 << TET_CODE[t][2]) | (1 << TET_CODE[t][3]);
    if ((seen & all) != all) return 0;
    return ((inside >> TET_CODE[t][0]) & 1) | (((inside >> TET_CODE[t][1]) & 1) << 1) | (((inside >> TET_CODE[t][2]) & 1) << 2) |
           (((inside >> TET_CODE[t][3]) & 1) << 3);
}

template <int t>
__device__ __forceinline__ int tsdf_mark_tet(const TsdfGrid& g, int n, int inside, int seen, unsigned char* __restrict__ flags)
{
    const int m = tsdf_tet_case<t>(inside, seen);
    if (m == 0 || m == 15) return 0;
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const int a = TET_EDGE_A[e], b = TET_EDGE_B[e];
        if (((m >> a) ^ (m >> b)) & 1) {
            const int owner = n + tsdf_code_offset(g, TET_CODE[t][a]);
            flags[(size_t)owner * 7 + SLOT_OF_BITS[TET_CODE[t][b] ^ TET_CODE[t][a]]] = 1;
        }
    }
    return __popc((unsigned)m) == 2 ? 2 : 1;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_mark_kernel(const TsdfGrid g, const float* __restrict__ tsdf,
                                                                 const float* __restrict__ weight, float minWeight,
                                                                 unsigned char* __restrict__ flags, int* __restrict__ triCount)
{
    const int n = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= g.n) return;
    int count = 0;
    if (tsdf_is_cell(g, n)) {
        int inside, seen;
        tsdf_cell_bits(g, n, tsdf, weight, minWeight, inside, seen);
        if (inside != 0 && inside != 255) {
            count += tsdf_mark_tet<0>(g, n, inside, seen, flags);
            count += tsdf_mark_tet<1>(g, n, inside, seen, flags);
            count += tsdf_mark_tet<2>(g, n, inside, seen, flags);
            count += tsdf_mark_tet<3>(g, n, inside, seen, flags);
            count += tsdf_mark_tet<4>(g, n, inside, seen, flags);
            count += tsdf_mark_tet<5>(g, n, inside, seen, flags);
        }
    }
    triCount[n] = count;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_compact_kernel(int n, const unsigned char* __restrict__ flags,
                                                                    unsigned char* __restrict__ edgeMask, int* __restrict__ vertCount)
{
    const int p = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (p >= n) return;
    int m = 0;
#pragma unroll
    for (int s = 0; s < 7; s++) m |= (flags[(size_t)p * 7 + s] ? 1 : 0) << s;
    edgeMask[p] = (unsigned char)m;
    vertCount[p] = __popc((unsigned)m);
}

// ---- exclusive scan of an int array, in place -----------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T tsdf_wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = block sum
template <typename T>
__device__ __forceinline__ T tsdf_block_excl_scan(T v, T* total)
{
    __shared__ T waveSum[TSDF_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T incl = tsdf_wave_incl_scan(v, lane);
    if (lane == 63) waveSum[wv] = incl;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < TSDF_THREADS / 64; q++) {
        if (q < wv) base += waveSum[q];
        tot += waveSum[q];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_tile_sums_kernel(int n, const int* __restrict__ v, long long* __restrict__ tileSums)
{
    const long long base = (long long)blockIdx.x * TSDF_SCAN_TILE + threadIdx.x * TSDF_SCAN_ITEMS;
    int s = 0;
#pragma unroll
    for (int q = 0; q < TSDF_SCAN_ITEMS; q++)
        if (base + q < n) s += v[base + q];
    int tot;
    tsdf_block_excl_scan(s, &tot);
    if (threadIdx.x == 0) tileSums[blockIdx.x] = tot;
}

// one block: exclusive scan of the tile sums in place, TSDF_THREADS tiles per pass with a 64-bit carry; the total -> *total
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_tile_scan_kernel(int nTiles, long long* tileSums, long long* total)
{
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < nTiles; t0 += TSDF_THREADS) {
        const int t = t0 + threadIdx.x;
        const long long v = t < nTiles ? tileSums[t] : 0;
        long long tot;
        const long long ex = tsdf_block_excl_scan(v, &tot);
        const long long c = carry;
        if (t < nTiles) tileSums[t] = c + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// (offsets are kept as int: a plan whose totals do not fit one is refused before anything reads them)
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_scan_apply_kernel(int n, int* __restrict__ v, const long long* __restrict__ tileOffsets)
{
    const long long base = (long long)blockIdx.x * TSDF_SCAN_TILE + threadIdx.x * TSDF_SCAN_ITEMS;
    int x[TSDF_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int q = 0; q < TSDF_SCAN_ITEMS; q++) { x[q] = base + q < n ? v[base + q] : 0; s += x[q]; }
    int tot;
    long long run = tileOffsets[blockIdx.x] + tsdf_block_excl_scan(s, &tot);
#pragma unroll
    for (int q = 0; q < TSDF_SCAN_ITEMS; q++) {
        if (base + q < n) v[base + q] = (int)run;
        run += x[q];
    }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_vertices_kernel(const TsdfGrid g, const float* __restrict__ tsdf,
                                                                     const float* __restrict__ rgb, const float* __restrict__ cweight,
                                                                     const unsigned char* __restrict__ edgeMask,
                                                                     const int* __restrict__ vertOff, long long V,
                                                                     float* __restrict__ vertices, float* __restrict__ colors)
{
    const int n = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= g.n) return;
    const int mask = edgeMask[n];
    if (!mask) return;
    int i, j, k;
    tsdf_ijk(g, n, i, j, k);
    const float fa = tsdf[n];
    const float pax = g.ox + g.voxel * (float)i, pay = g.oy + g.voxel * (float)j, paz = g.oz + g.voxel * (float)k;
    long long id = vertOff[n];
#pragma unroll
    for (int s = 0; s < 7; s++) {
        if (!((mask >> s) & 1)) continue;
        const int dir = DIR_OF_SLOT[s];
        const int di = dir & 1, dj = (dir >> 1) & 1, dk = (dir >> 2) & 1;
        // (a marked edge's far end is a corner of the cell that marked it: inside the lattice; the clamp guards a workspace
        // that was overwritten between plan and emit)
        const int m = min(n + di + g.nx * (dj + g.ny * dk), g.n - 1);
        const float fb = tsdf[m];
        const float t = fa / (fa - fb);
        const float pbx = g.ox + g.voxel * (float)(i + di), pby = g.oy + g.voxel * (float)(j + dj), pbz = g.oz + g.voxel * (float)(k + dk);
        if (id >= 0 && id < V) {
            float* o = vertices + 3 * id;
            o[0] = pax + t * (pbx - pax);
            o[1] = pay + t * (pby - pay);
            o[2] = paz + t * (pbz - paz);
            if (colors) {
                const bool ha = cweight[n] != 0.0f, hb = cweight[m] != 0.0f;
                float* c = colors + 3 * id;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const float ca = rgb[3 * (size_t)n + q], cb = rgb[3 * (size_t)m + q];
                    c[q] = ha && hb ? ca + t * (cb - ca) : ha ? ca : hb ? cb : 0.5f;
                }
            }
        }
        id++;
    }
}

template <int t>
__device__ __forceinline__ void tsdf_emit_tet(int inside, int seen, const int (&cornerMask)[8], const int (&cornerOff)[8], long long& at,
                                              long long V, long long F, int* __restrict__ faces)
{
    const int m = tsdf_tet_case<t>(inside, seen);
    if (m == 0 || m == 15) return;
    int id[6];
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const int a = TET_CODE[t][TET_EDGE_A[e]], b = TET_CODE[t][TET_EDGE_B[e]];
        const int slot = SLOT_OF_BITS[a ^ b];
        id[e] = cornerOff[a] + __popc((unsigned)(cornerMask[a] & ((1 << slot) - 1)));     // (read only for a crossed edge)
    }
    const uint32_t entry = TET_CASES[TET_ODD[t] ? m ^ 15 : m];
    const int ntri = __popc((unsigned)m) == 2 ? 2 : 1;
    for (int q = 0; q < ntri; q++) {
        int tri[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int e = (entry >> (9 * q + 3 * c)) & 7;
            tri[c] = e == 0 ? id[0] : e == 1 ? id[1] : e == 2 ? id[2] : e == 3 ? id[3] : e == 4 ? id[4] : id[5];
        }
        const bool ok = at >= 0 && at < F && tri[0] >= 0 && tri[0] < V && tri[1] >= 0 && tri[1] < V && tri[2] >= 0 && tri[2] < V;
        if (ok) { faces[3 * at] = tri[0]; faces[3 * at + 1] = tri[1]; faces[3 * at + 2] = tri[2]; }
        at++;
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_faces_kernel(const TsdfGrid g, const float* __restrict__ tsdf,
                                                                  const float* __restrict__ weight, float minWeight,
                                                                  const unsigned char* __restrict__ edgeMask,
                                                                  const int* __restrict__ vertOff, const int* __restrict__ triOff,
                                                                  long long V, long long F, int* __restrict__ faces)
{
    const int n = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= g.n || !tsdf_is_cell(g, n)) return;
    int inside, seen;
    tsdf_cell_bits(g, n, tsdf, weight, minWeight, inside, seen);
    if (inside == 0 || inside == 255) return;
    int cornerMask[8], cornerOff[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int m = n + tsdf_code_offset(g, c);
        cornerMask[c] = edgeMask[m];
        cornerOff[c] = vertOff[m];
    }
    long long at = triOff[n];
    tsdf_emit_tet<0>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
    tsdf_emit_tet<1>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
    tsdf_emit_tet<2>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
    tsdf_emit_tet<3>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
    tsdf_emit_tet<4>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
    tsdf_emit_tet<5>(inside, seen, cornerMask, cornerOff, at, V, F, faces);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
namespace {

int tsdf_fail(gs_ctx* c, int code, const char* msg)
{
    if (c) c->err = msg;
    return code;
}

bool tsdf_grid_ok(const gs_tsdf_grid* g)
{
    if (!g) return false;
    const int d[3] = {g->nx, g->ny, g->nz};
    for (int x : d)
        if (x < 2 || x > TSDF_MAX_DIM) return false;
    if ((long long)g->nx * g->ny * g->nz > TSDF_MAX_POINTS) return false;
    if (!(g->voxel > 0.0f) || !isfinite(g->voxel) || !(g->trunc > 0.0f) || !isfinite(g->trunc)) return false;
    return isfinite(g->origin[0]) && isfinite(g->origin[1]) && isfinite(g->origin[2]);
}

TsdfGrid tsdf_grid_args(const gs_tsdf_grid& g)
{
    TsdfGrid a;
    a.ox = g.origin[0]; a.oy = g.origin[1]; a.oz = g.origin[2]; a.voxel = g.voxel;
    a.nx = g.nx; a.ny = g.ny; a.nz = g.nz; a.n = g.nx * g.ny * g.nz;
    a.trunc = g.trunc;
    return a;
}

size_t tsdf_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the plan's workspace: flags [7 n] bytes | edge masks [n] bytes | vertex offsets [n] int | triangle offsets [n] int |
// tile offsets of the two scans [nTiles] int64 each | the two totals
struct TsdfWorkspace {
    unsigned char* flags;
    unsigned char* edgeMask;
    int* vertOff;
    int* triOff;
    long long* vertTiles;
    long long* triTiles;
    long long* totals;
    size_t bytes;
};

TsdfWorkspace tsdf_workspace(void* base, long long n)
{
    const int nTiles = gs_div_up(n, TSDF_SCAN_TILE);
    unsigned char* p = (unsigned char*)base;
    size_t o = 0;
    TsdfWorkspace w;
    w.flags = p + o; o += tsdf_align((size_t)n * 7);
    w.edgeMask = p + o; o += tsdf_align((size_t)n);
    w.vertOff = (int*)(p + o); o += tsdf_align((size_t)n * sizeof(int));
    w.triOff = (int*)(p + o); o += tsdf_align((size_t)n * sizeof(int));
    w.vertTiles = (long long*)(p + o); o += tsdf_align((size_t)nTiles * sizeof(long long));
    w.triTiles = (long long*)(p + o); o += tsdf_align((size_t)nTiles * sizeof(long long));
    w.totals = (long long*)(p + o); o += tsdf_align(2 * sizeof(long long));
    w.bytes = o;
    return w;
}

int tsdf_scan(gs_ctx* c, int n, int* v, long long* tiles, long long* total)
{
    const int nTiles = gs_div_up(n, TSDF_SCAN_TILE);
    hipLaunchKernelGGL(tsdf_tile_sums_kernel, dim3(nTiles), dim3(TSDF_THREADS), 0, c->stream, n, v, tiles);
    hipLaunchKernelGGL(tsdf_tile_scan_kernel, dim3(1), dim3(TSDF_THREADS), 0, c->stream, nTiles, tiles, total);
    hipLaunchKernelGGL(tsdf_scan_apply_kernel, dim3(nTiles), dim3(TSDF_THREADS), 0, c->stream, n, v, tiles);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace
}  // namespace gs

using namespace gs;

#pragma GCC visibility push(default)
extern "C" {

int gs_tsdf_integrate(gs_ctx* c, const gs_tsdf_grid* grid, int n_views, const gs_tsdf_view* views, float* tsdf, float* weight,
                      float* rgb, float* cweight)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!tsdf_grid_ok(grid))
        return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: grid dimensions are 2 .. 1024 with at most 2^28 points, voxel and trunc finite and > 0");
    if (n_views < 1 || n_views > GS_TSDF_MAX_VIEWS) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: n_views in 1 .. 8");
    if (!views || !tsdf || !weight) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: null pointer");
    if (!rgb != !cweight) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: rgb and cweight are both given or both NULL");
    TsdfIntegrateArgs A;
    memset(&A, 0, sizeof(A));
    A.g = tsdf_grid_args(*grid);
    A.nViews = n_views;
    for (int i = 0; i < n_views; i++) {
        const gs_tsdf_view& v = views[i];
        if (!v.depth) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: a view without a depth image");
        if (v.width < 1 || v.height < 1 || (long long)v.width * v.height > (1ll << 28))
            return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: image sizes are positive, at most 2^28 pixels");
        if (!(v.fx > 0.0f) || !isfinite(v.fx) || !(v.fy > 0.0f) || !isfinite(v.fy))
            return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: focal lengths are finite and > 0");
        bool finite = isfinite(v.cx) && isfinite(v.cy);
        for (float r : v.Rt) finite = finite && isfinite(r);
        if (!finite) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_integrate: principal points and poses are finite");
        TsdfView& o = A.v[i];
        memcpy(o.Rt, v.Rt, sizeof(o.Rt));
        o.fx = v.fx; o.fy = v.fy; o.cx = v.cx; o.cy = v.cy;
        o.uMax = (float)(v.width - 1); o.vMax = (float)(v.height - 1);
        o.width = v.width;
        o.depth = v.depth; o.color = v.color;
    }
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(gs_div_up(A.g.n, TSDF_THREADS)), dim3(TSDF_THREADS), 0, c->stream, A, tsdf,
                       weight, rgb, cweight);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

size_t gs_tsdf_mesh_workspace_bytes(const gs_tsdf_grid* grid)
{
    if (!tsdf_grid_ok(grid)) return 0;
    return tsdf_workspace(nullptr, (long long)grid->nx * grid->ny * grid->nz).bytes;
}

int gs_tsdf_mesh_plan(gs_ctx* c, const gs_tsdf_grid* grid, const float* tsdf, const float* weight, float min_weight, void* workspace,
                      size_t workspace_bytes, long long* counts)
{
    if (!c) return GS_ERR_INVALID_ARG;
    c->tsdfPlan.ws = nullptr;
    if (!tsdf_grid_ok(grid))
        return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: grid dimensions are 2 .. 1024 with at most 2^28 points, voxel and trunc finite and > 0");
    if (!tsdf || !weight || !workspace || !counts) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: null pointer");
    if (!isfinite(min_weight)) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: min_weight is finite");
    if (((uintptr_t)workspace & 255) != 0) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: the workspace is 256-byte aligned");
    const TsdfGrid g = tsdf_grid_args(*grid);
    const TsdfWorkspace w = tsdf_workspace(workspace, g.n);
    if (workspace_bytes < w.bytes)
        return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: the workspace is smaller than gs_tsdf_mesh_workspace_bytes");
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    GS_HIP_CHECK(c, hipMemsetAsync(w.flags, 0, (size_t)g.n * 7, c->stream));
    const dim3 blocks(gs_div_up(g.n, TSDF_THREADS)), threads(TSDF_THREADS);
    hipLaunchKernelGGL(tsdf_mark_kernel, blocks, threads, 0, c->stream, g, tsdf, weight, min_weight, w.flags, w.triOff);
    hipLaunchKernelGGL(tsdf_compact_kernel, blocks, threads, 0, c->stream, g.n, w.flags, w.edgeMask, w.vertOff);
    GS_HIP_CHECK(c, hipGetLastError());
    int rc = tsdf_scan(c, g.n, w.vertOff, w.vertTiles, w.totals);
    if (rc) return rc;
    rc = tsdf_scan(c, g.n, w.triOff, w.triTiles, w.totals + 1);
    if (rc) return rc;
    GS_HIP_CHECK(c, hipMemcpyAsync(counts, w.totals, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (counts[0] > INT32_MAX || counts[1] > INT32_MAX)
        return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_plan: more than INT32_MAX vertices or triangles");
    c->tsdfPlan.ws = workspace;
    c->tsdfPlan.grid = *grid;
    c->tsdfPlan.minWeight = min_weight;
    c->tsdfPlan.V = counts[0];
    c->tsdfPlan.F = counts[1];
    return GS_OK;
}

int gs_tsdf_mesh_emit(gs_ctx* c, const gs_tsdf_grid* grid, const float* tsdf, const float* weight, const float* rgb,
                      const float* cweight, float min_weight, void* workspace, float* vertices, float* colors, int32_t* faces)
{
    if (!c) return GS_ERR_INVALID_ARG;
    if (!c->tsdfPlan.ws) return tsdf_fail(c, GS_ERR_NO_FORWARD, "gs_tsdf_mesh_emit: no gs_tsdf_mesh_plan on this context");
    if (!grid || workspace != c->tsdfPlan.ws || memcmp(grid, &c->tsdfPlan.grid, sizeof(gs_tsdf_grid)) != 0 ||
        !(min_weight == c->tsdfPlan.minWeight))
        return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_emit: workspace, grid and min_weight are the last gs_tsdf_mesh_plan's");
    const long long V = c->tsdfPlan.V, F = c->tsdfPlan.F;
    if (V == 0 && F == 0) return GS_OK;
    if (!tsdf || !weight || !vertices || !faces) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_emit: null pointer");
    if (colors && (!rgb || !cweight)) return tsdf_fail(c, GS_ERR_INVALID_ARG, "gs_tsdf_mesh_emit: colors need rgb and cweight");
    const TsdfGrid g = tsdf_grid_args(*grid);
    const TsdfWorkspace w = tsdf_workspace(workspace, g.n);
    GS_HIP_CHECK(c, hipSetDevice(c->device));
    const dim3 blocks(gs_div_up(g.n, TSDF_THREADS)), threads(TSDF_THREADS);
    hipLaunchKernelGGL(tsdf_vertices_kernel, blocks, threads, 0, c->stream, g, tsdf, rgb, cweight, w.edgeMask, w.vertOff, V, vertices,
                       colors);
    hipLaunchKernelGGL(tsdf_faces_kernel, blocks, threads, 0, c->stream, g, tsdf, weight, min_weight, w.edgeMask, w.vertOff, w.triOff,
                       V, F, faces);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
