// mcmc.hip -- the MCMC densification strategy (include/gsplat.h gs_set_mcmc): the stand-alone forms of
// the per-step part (regularisers, noise; the fused form is projection.hip's proj_bwd_fused_*mcmc_kernel) and the event's
// kernels.  Compiled with -ffp-contract=off, as projection.hip is: the noise and the regularisers then round exactly as the
// fused kernel's do.
//
// An event (relocation or growth) is a handful of small launches over N: weights and block sums, their float64 exclusive scan in
// one thread (fixed order), the compaction of the candidate rows with their inclusive float64 prefix, one read of the counts,
// the sampler (binary search), the per-source counts (integer atomics), the float64 formula on the sources, the row copy.  No
// float atomics: two runs from the same state give the same bits.
#include <math.h>

#include "gs_ctx.h"
#include "gs_mcmc.h"

namespace gs {

constexpr int MC_THREADS = 256;
constexpr int MC_ITEMS = 4;                        // consecutive rows per thread in the scan kernels
constexpr int MC_TILE = MC_THREADS * MC_ITEMS;

// ---- per step --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcmc_reg_kernel(int N, const float* __restrict__ scales, const float* __restrict__ opacity,
                                                       float* __restrict__ gScales, float* __restrict__ gOpacity, McmcFuse mc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    gOpacity[i] = gOpacity[i] + mc.oCoef * mcmc_sigmoid_slope(opacity[i]);
#pragma unroll
    for (int a = 0; a < 3; a++) gScales[3 * i + a] = gScales[3 * i + a] + mc.sCoef * expf(scales[3 * i + a]);
}

__global__ __launch_bounds__(256) void mcmc_noise_kernel(int N, float* __restrict__ xyz, const float* __restrict__ scales,
                                                         const float* __restrict__ rot, const float* __restrict__ opacity,
                                                         McmcFuse mc, const uint32_t* __restrict__ gate)
{
    if (*gate) return;      // the step's forward overflowed its reserved pairs: its update was skipped, so is its noise
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float sr[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float rr[4] = {rot[4 * i], rot[4 * i + 1], rot[4 * i + 2], rot[4 * i + 3]};
    float d[3];
    mcmc_noise(mc, (uint32_t)i, sr, rr, opacity[i], d);
#pragma unroll
    for (int a = 0; a < 3; a++) xyz[3 * i + a] = xyz[3 * i + a] + d[a];
}

__device__ __forceinline__ uint32_t mcmc_stream_tag(int stream)
{
    return stream == 0 ? MCMC_TAG_NOISE : stream == 1 ? MCMC_TAG_RELOCATE : MCMC_TAG_GROW;
}

__global__ __launch_bounds__(256) void mcmc_random_kernel(unsigned long long seed, uint32_t t, int stream, int n,
                                                          uint32_t* __restrict__ words, float* __restrict__ normals,
                                                          double* __restrict__ uniforms)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4];
    mcmc_philox((uint32_t)i, t, mcmc_stream_tag(stream), seed, w);
    if (words) {
#pragma unroll
        for (int k = 0; k < 4; k++) words[4 * (size_t)i + k] = w[k];
    }
    if (normals) {
        float z[3];
        mcmc_normals(w, z);
#pragma unroll
        for (int k = 0; k < 3; k++) normals[3 * (size_t)i + k] = z[k];
    }
    if (uniforms) uniforms[i] = mcmc_uniform(w);
}

// ---- the event ---------------------------------------------------------------------------------------------------
// A row's weight: relocation (mode 0) draws from the live rows, o > min_opacity with a finite opacity_raw, and refills the
// others (dead); growth (mode 1) draws from every row whose opacity_raw is finite, weight o.
__device__ __forceinline__ void mcmc_weight(int mode, float raw, double minOp, double& w, int& cand, int& dead)
{
    const double o = 1.0 / (1.0 + exp(-(double)raw));
    const bool fin = (raw - raw) == 0.0f;
    cand = fin && (mode == 0 ? o > minOp : o > 0.0);
    dead = mode == 0 && !cand;
    w = cand ? o : 0.0;
}

// block scan of one value per thread (Hillis-Steele in LDS: the same order on every run): the inclusive value; excl = the
// previous thread's inclusive value, bit for bit
template <class T>
__device__ __forceinline__ T mcmc_block_scan(T v, T* lds, T& excl)
{
    lds[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < MC_THREADS; o <<= 1) {
        const T add = threadIdx.x >= (unsigned)o ? lds[threadIdx.x - o] : T(0);
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    excl = threadIdx.x > 0 ? lds[threadIdx.x - 1] : T(0);
    return lds[threadIdx.x];
}

struct McmcThreadSums {
    double w[MC_ITEMS];
    int cand[MC_ITEMS], dead[MC_ITEMS];
    double sw;
    int sc, sd;
};

__device__ __forceinline__ void mcmc_thread_rows(int N, const float* opacity, int mode, double minOp, McmcThreadSums& t)
{
    const int base = blockIdx.x * MC_TILE + threadIdx.x * MC_ITEMS;
    t.sw = 0.0; t.sc = 0; t.sd = 0;
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const int i = base + k;
        t.w[k] = 0.0; t.cand[k] = 0; t.dead[k] = 0;
        if (i < N) mcmc_weight(mode, opacity[i], minOp, t.w[k], t.cand[k], t.dead[k]);
        t.sw += t.w[k]; t.sc += t.cand[k]; t.sd += t.dead[k];
    }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_block_sums_kernel(int N, const float* __restrict__ opacity, int mode, double minOp,
                                                                     double* __restrict__ bW, int* __restrict__ bC, int* __restrict__ bD)
{
    __shared__ double sW[MC_THREADS];
    __shared__ int sI[MC_THREADS];
    McmcThreadSums t;
    mcmc_thread_rows(N, opacity, mode, minOp, t);
    double we;
    int ce, de;
    const double w = mcmc_block_scan(t.sw, sW, we);
    const int c = mcmc_block_scan(t.sc, sI, ce);
    __syncthreads();
    const int d = mcmc_block_scan(t.sd, sI, de);
    if (threadIdx.x == MC_THREADS - 1) { bW[blockIdx.x] = w; bC[blockIdx.x] = c; bD[blockIdx.x] = d; }
}

// exclusive scan of the block sums in place, in index order; counts[0] = dead rows, counts[1] = candidate rows
__global__ void mcmc_block_offsets_kernel(int nb, double* bW, int* bC, int* bD, long long* counts)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double w = 0.0;
    long long c = 0, d = 0;
    for (int b = 0; b < nb; b++) {
        const double bw = bW[b];
        const int bc = bC[b], bd = bD[b];
        bW[b] = w; bC[b] = (int)c; bD[b] = (int)d;
        w += bw; c += bc; d += bd;
    }
    counts[0] = d;
    counts[1] = c;
}

// the candidate rows in index order with their inclusive float64 prefix, and the dead rows in index order
__global__ __launch_bounds__(MC_THREADS) void mcmc_compact_kernel(int N, const float* __restrict__ opacity, int mode, double minOp,
                                                                  const double* __restrict__ bW, const int* __restrict__ bC,
                                                                  const int* __restrict__ bD, double* __restrict__ cdf,
                                                                  int* __restrict__ candRows, int* __restrict__ deadRows)
{
    __shared__ double sW[MC_THREADS];
    __shared__ int sI[MC_THREADS];
    McmcThreadSums t;
    mcmc_thread_rows(N, opacity, mode, minOp, t);
    double wEx;
    int cEx, dEx;
    (void)mcmc_block_scan(t.sw, sW, wEx);
    (void)mcmc_block_scan(t.sc, sI, cEx);
    __syncthreads();
    (void)mcmc_block_scan(t.sd, sI, dEx);
    double run = bW[blockIdx.x] + wEx;
    int cp = bC[blockIdx.x] + cEx, dp = bD[blockIdx.x] + dEx;
    const int base = blockIdx.x * MC_TILE + threadIdx.x * MC_ITEMS;
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        if (t.cand[k]) { run += t.w[k]; cdf[cp] = run; candRows[cp] = base + k; cp++; }
        if (t.dead[k] && deadRows) { deadRows[dp] = base + k; dp++; }
    }
}

// draw j: u from the stream, the first candidate whose inclusive prefix exceeds u * total (the last one if none does)
__global__ __launch_bounds__(256) void mcmc_sample_kernel(int nDraw, unsigned long long seed, uint32_t t, uint32_t tag, int nCand,
                                                          const double* __restrict__ cdf, const int* __restrict__ candRows,
                                                          int* __restrict__ samples, int* __restrict__ counts)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nDraw) return;
    uint32_t w[4];
    mcmc_philox((uint32_t)j, t, tag, seed, w);
    const double target = mcmc_uniform(w) * cdf[nCand - 1];
    int lo = 0, hi = nCand - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int src = candRows[lo];
    samples[j] = src;
    atomicAdd(&counts[src], 1);
}

struct McmcDevRows {
    float* t[6];
    long long mOff[6];       // element offset of each tensor from the parameter base: its moments lie there in m and v
    float* m;
    float* v;
    int len[6];
};

// a source drawn c times: n = min(c + 1, n_max); o' and s' in float64 (include/gsplat.h gs_mcmc_relocate); its moments zeroed
__global__ __launch_bounds__(256) void mcmc_formula_kernel(int N, const int* __restrict__ counts, int nMax, double minOp,
                                                           McmcDevRows r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = counts[i];
    if (c == 0) return;
    const int n = min(c + 1, nMax);
    float* opacity = r.t[5];
    float* scales = r.t[3];
    const double o = 1.0 / (1.0 + exp(-(double)opacity[i]));
    double on = 1.0 - pow(1.0 - o, 1.0 / (double)n);
    on = fmin(fmax(on, minOp), 1.0 - 1.1920928955078125e-07);
    double den = 0.0;
    for (int a = 1; a <= n; a++) {
        double binom = 1.0, pw = on;                 // C(a-1, k), o'^(k+1)
        for (int k = 0; k < a; k++) {
            const double term = binom * pw / sqrt((double)(k + 1));
            den += (k & 1) ? -term : term;
            binom = binom * (double)(a - 1 - k) / (double)(k + 1);
            pw *= on;
        }
    }
    const double ratio = o / den;
    opacity[i] = (float)log(on / (1.0 - on));
#pragma unroll
    for (int a = 0; a < 3; a++) scales[3 * i + a] = (float)log(exp((double)scales[3 * i + a]) * ratio);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const long long e0 = r.mOff[k] + (long long)i * r.len[k];
        for (int e = 0; e < r.len[k]; e++) { r.m[e0 + e] = 0.0f; r.v[e0 + e] = 0.0f; }
    }
}

// element e of draw j's row: the source's value into the destination (the j-th dead row, or row N + j), moments zeroed
__global__ __launch_bounds__(256) void mcmc_copy_kernel(long long total, int F, const int* __restrict__ samples,
                                                        const int* __restrict__ deadRows, int N, McmcDevRows r)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx / F);
    int e = (int)(idx - (long long)j * F);
    const int src = samples[j];
    const int dst = deadRows ? deadRows[j] : N + j;
    float* T = r.t[0];
    long long mo = r.mOff[0];
    int L = r.len[0];
#pragma unroll
    for (int k = 1; k < 6; k++)
        if (e >= L) { e -= L; T = r.t[k]; mo = r.mOff[k]; L = r.len[k]; }
    const long long s = (long long)src * L + e, d = (long long)dst * L + e;
    T[d] = T[s];
    r.m[mo + d] = 0.0f;
    r.v[mo + d] = 0.0f;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
static int grid(long long n, int threads) { return (int)((n + threads - 1) / threads); }

int launch_mcmc_regularizer(gs_ctx* c, int N, const float* scales, const float* opacity, float* gScales, float* gOpacity,
                            const gs_mcmc_params& p)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(mcmc_reg_kernel, dim3(grid(N, 256)), dim3(256), 0, c->stream, N, scales, opacity, gScales, gOpacity,
                       mcmc_fuse(p, N, 0.0f));
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_mcmc_noise(gs_ctx* c, int N, float* xyz, const float* scales, const float* rot, const float* opacity, float lrXyz,
                      const gs_mcmc_params& p)
{
    if (N == 0) return GS_OK;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(grid(N, 256)), dim3(256), 0, c->stream, N, xyz, scales, rot, opacity,
                       mcmc_fuse(p, N, lrXyz), c->adamGate);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

int launch_mcmc_random(gs_ctx* c, unsigned long long seed, int iteration, int stream, int n, uint32_t* words, float* normals,
                       double* uniforms)
{
    if (n == 0) return GS_OK;
    hipLaunchKernelGGL(mcmc_random_kernel, dim3(grid(n, 256)), dim3(256), 0, c->stream, seed, (uint32_t)iteration, stream, n,
                       words, normals, uniforms);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

namespace {

struct McmcWs {
    double* cdf;
    int* cand;
    int* dead;
    int* samples;
    int* counts;
    double* bW;
    int* bC;
    int* bD;
    long long* counters;     // [0] dead rows, [1] candidate rows
    int nb;
};

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// the scratch of an event over N rows (<= N draws): grown on demand, kept with the context
int mcmc_ws(gs_ctx* c, int N, McmcWs& w)
{
    const int nb = grid(N, MC_TILE);
    const size_t n = (size_t)N;
    const size_t sz[9] = {align16(8 * n), align16(4 * n), align16(4 * n), align16(4 * n), align16(4 * n),
                          align16(8 * (size_t)nb), align16(4 * (size_t)nb), align16(4 * (size_t)nb), 16};
    size_t total = 0;
    for (size_t s : sz) total += s;
    if (total > c->mcmcWsBytes) {
        if (const int rc = ctx_grow(c, &c->mcmcWs, &c->mcmcWsBytes, (long long)(total + total / 2))) return rc;
    }
    if (!c->mcmcHost) { if (const int rc = ctx_alloc_pinned(c, &c->mcmcHost, 4)) return rc; }
    char* b = c->mcmcWs;
    w.cdf = reinterpret_cast<double*>(b); b += sz[0];
    w.cand = reinterpret_cast<int*>(b); b += sz[1];
    w.dead = reinterpret_cast<int*>(b); b += sz[2];
    w.samples = reinterpret_cast<int*>(b); b += sz[3];
    w.counts = reinterpret_cast<int*>(b); b += sz[4];
    w.bW = reinterpret_cast<double*>(b); b += sz[5];
    w.bC = reinterpret_cast<int*>(b); b += sz[6];
    w.bD = reinterpret_cast<int*>(b); b += sz[7];
    w.counters = reinterpret_cast<long long*>(b);
    w.nb = nb;
    return GS_OK;
}

McmcDevRows dev_rows(const McmcRows& rows, int K)
{
    McmcDevRows r;
    const int len[6] = {3, 3, 3 * (K - 1), 3, 4, 1};
    for (int k = 0; k < 6; k++) {
        r.t[k] = rows.t[k];
        r.len[k] = len[k];
        r.mOff[k] = (long long)(rows.t[k] - rows.pBase);
    }
    r.m = rows.mBase; r.v = rows.vBase;
    return r;
}

// weights, scan, compaction; then the one read of the two counts
int mcmc_scan(gs_ctx* c, int N, const float* opacity, int mode, double minOp, const McmcWs& w, long long& nDead, long long& nCand)
{
    hipLaunchKernelGGL(mcmc_block_sums_kernel, dim3(w.nb), dim3(MC_THREADS), 0, c->stream, N, opacity, mode, minOp, w.bW, w.bC, w.bD);
    hipLaunchKernelGGL(mcmc_block_offsets_kernel, dim3(1), dim3(64), 0, c->stream, w.nb, w.bW, w.bC, w.bD, w.counters);
    hipLaunchKernelGGL(mcmc_compact_kernel, dim3(w.nb), dim3(MC_THREADS), 0, c->stream, N, opacity, mode, minOp, w.bW, w.bC, w.bD,
                       w.cdf, w.cand, mode == 0 ? w.dead : nullptr);
    GS_HIP_CHECK(c, hipGetLastError());
    GS_HIP_CHECK(c, hipMemcpyAsync(c->mcmcHost, w.counters, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    nDead = c->mcmcHost[0];
    nCand = c->mcmcHost[1];
    return GS_OK;
}

// draws, counts, the formula on the sources, the copy of their rows into the destinations
int mcmc_draw_and_copy(gs_ctx* c, int N, int K, const McmcRows& rows, const gs_mcmc_params& p, const McmcWs& w, int nDraw,
                       int nCand, uint32_t tag, bool intoDead)
{
    const McmcDevRows r = dev_rows(rows, K);
    GS_HIP_CHECK(c, hipMemsetAsync(w.counts, 0, sizeof(int) * (size_t)N, c->stream));
    hipLaunchKernelGGL(mcmc_sample_kernel, dim3(grid(nDraw, 256)), dim3(256), 0, c->stream, nDraw, p.seed, (uint32_t)p.iteration,
                       tag, nCand, w.cdf, w.cand, w.samples, w.counts);
    hipLaunchKernelGGL(mcmc_formula_kernel, dim3(grid(N, 256)), dim3(256), 0, c->stream, N, w.counts, p.n_max, p.min_opacity, r);
    const int F = 14 + 3 * (K - 1);
    const long long total = (long long)nDraw * F;
    hipLaunchKernelGGL(mcmc_copy_kernel, dim3(grid(total, 256)), dim3(256), 0, c->stream, total, F, w.samples,
                       intoDead ? w.dead : nullptr, N, r);
    GS_HIP_CHECK(c, hipGetLastError());
    return GS_OK;
}

}  // namespace

int mcmc_relocate(gs_ctx* c, int N, int K, const McmcRows& rows, const gs_mcmc_params& p, long long stats[4])
{
    stats[0] = stats[1] = stats[2] = 0;
    stats[3] = N;
    if (N == 0) return GS_OK;
    McmcWs w;
    int rc = mcmc_ws(c, N, w);
    if (rc) return rc;
    long long nDead = 0, nLive = 0;
    if ((rc = mcmc_scan(c, N, rows.t[5], 0, p.min_opacity, w, nDead, nLive))) return rc;
    stats[0] = nDead;
    stats[2] = nLive;
    if (nDead == 0 || nLive == 0) return GS_OK;
    if ((rc = mcmc_draw_and_copy(c, N, K, rows, p, w, (int)nDead, (int)nLive, MCMC_TAG_RELOCATE, true))) return rc;
    stats[1] = nDead;
    return GS_OK;
}

int mcmc_grow(gs_ctx* c, int N, int capacity, int K, const McmcRows& rows, const gs_mcmc_params& p, int* nOut)
{
    *nOut = N;
    const long long grown = (long long)floor((1.0 + p.grow_rate) * (double)N);
    const long long target = grown < p.cap_max ? grown : p.cap_max;
    const long long nAdd = target - N;
    if (N == 0 || nAdd <= 0) return GS_OK;
    if (N + nAdd > capacity) {
        c->err = "gs_mcmc_grow: the grown count exceeds the capacity of the tensors";
        return GS_ERR_SIZE_MISMATCH;
    }
    McmcWs w;
    int rc = mcmc_ws(c, N, w);
    if (rc) return rc;
    long long nDead = 0, nCand = 0;
    if ((rc = mcmc_scan(c, N, rows.t[5], 1, p.min_opacity, w, nDead, nCand))) return rc;
    if (nCand == 0) return GS_OK;
    if ((rc = mcmc_draw_and_copy(c, N, K, rows, p, w, (int)nAdd, (int)nCand, MCMC_TAG_GROW, false))) return rc;
    *nOut = (int)(N + nAdd);
    return GS_OK;
}

}  // namespace gs
