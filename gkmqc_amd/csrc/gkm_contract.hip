/*
 * gkm_contract.hip -- an l-mer weight table or panel contracted with position weight windows.  A window
 * P is L rows of four doubles, P[i][b] for l-mer position i (0: the first base, the highest bit pair of a code) and base
 * b; its value is the multilinear form
 *
 *   a(P) = sum over all 4^L codes u of W(u) prod_i P[i][u_i]
 *
 * evaluated in ONE order, the last base first, every product and sum rounded (-ffp-contract=off):
 *
 *   T_L[u] = W[u]
 *   T_i[v] = ((T_{i+1}[4v] P[i][0] + T_{i+1}[4v+1] P[i][1]) + T_{i+1}[4v+2] P[i][2]) + T_{i+1}[4v+3] P[i][3]
 *   a(P)   = T_0[0]
 *
 * (level4 below is that expression, the only arithmetic of this file).  A tile is 4^t consecutive codes, t = min(L, 6):
 * the subtree of depth t under the code prefix `tile`.  The tile kernels write T_{L-t}[tile] per (window, tile) -- straight
 * to the output where L <= 6 -- and k_contract_fold applies the remaining L - t levels to those partials.  Which lane,
 * wave or launch evaluates a node does not enter its value.
 *
 * Kernels
 *   k_lmer_contract   a workgroup owns one tile and a run of windows.  Lane l holds the 16 weights of the codes 16 l ..
 *                     16 l + 15 of the tile in registers for all of them: the table is read once per run.  Per window
 *                     two levels in registers, the window's rows wave-uniform (scalar loads); then per batch of
 *                     CT_BATCH windows the up to four levels across lanes through LDS, two buffers taking turns.
 *   k_panel_contract  the lanes across models (§5n): lane = (group g, model m), a group owns one tile and walks it
 *                     serially, depth first (subtree): a leaf is 16 coalesced row reads that serve the PK_WIN windows whose
 *                     level accumulators the lane carries.  No lane needs another: no LDS, no shuffles.
 *   k_contract_fold   one lane per (window, column): the partials of its tiles in ascending order, the remaining levels
 *                     as a carry chain (a digit that reaches 3 completes a node, which enters the level above).
 *
 * No atomics, no workgroup waits for another; the fold is a launch.  The partials live in the context (contract_part),
 * grown on demand: calls on one context are serialised by their stream, as for the context's other scratch.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_T = 6;      /* depth of a tile: 4^6 codes = 256 lanes x 16 weights */
constexpr int CT_BATCH = 16; /* windows whose lane values share one pass through LDS */
constexpr int CT_RUN = 64;   /* windows per workgroup of k_lmer_contract */
constexpr int PK_WIN = 8;    /* windows a lane of k_panel_contract carries at once */
constexpr int PK_RUN = 64;   /* windows per workgroup of k_panel_contract */
constexpr int64_t CT_MAX_WINDOWS = GKMHIP_CONTRACT_MAX_WINDOWS;
constexpr int64_t CT_MAX_SCRATCH = (int64_t)1 << 32; /* bytes of partials one call may ask for */

/* one node: four children, one row of a window */
template <typename X, typename R>
__device__ __forceinline__ double level4(const X &x, const R &p)
{
    return ((x[0] * p[0] + x[1] * p[1]) + x[2] * p[2]) + x[3] * p[3];
}

/* the subtree of depth 2 over 16 weights: r1 the window's row L - 1, r2 its row L - 2 */
template <typename R>
__device__ __forceinline__ double leaf16(const double (&w)[16], R r1, R r2)
{
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double x[4] = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        t[q] = level4(x, r1);
    }
    return level4(t, r2);
}

__global__ __launch_bounds__(CT_THREADS) void k_lmer_contract(const double *__restrict__ W, const double *__restrict__ P,
                                                              int nwin, int L, int t, int ntiles, double *__restrict__ dst)
{
    __shared__ double sA[CT_BATCH * 256];
    __shared__ double sB[CT_BATCH * 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.y;
    const int w_begin = blockIdx.x * CT_RUN, w_end = min(nwin, w_begin + CT_RUN);
    const int nl = 1 << (2 * (t - 2)); /* lanes that hold weights: 4^(t-2) */
    double w[16];
    {
        const double *src = W + ((size_t)tile << (2 * t)) + (size_t)tid * 16;
#pragma unroll
        for (int c = 0; c < 16; c++) w[c] = tid < nl ? src[c] : 0.0;
    }
    const sgpr_doubles sp = (sgpr_doubles)P;
    for (int w0 = w_begin; w0 < w_end; w0 += CT_BATCH) {
        const int nb = min(CT_BATCH, w_end - w0);
        for (int k = 0; k < nb; k++) {
            const sgpr_doubles r1 = sp + ((size_t)(w0 + k) * L + (L - 1)) * 4;
            sA[k * 256 + tid] = leaf16(w, r1, r1 - 4);
        }
        __syncthreads();
        /* the levels across lanes: n values per window shrink to n / 4, from one buffer into the other */
        double *src = sA, *out = sB;
        int ss = 256, os = 64, pos = L - 3;
        for (int sh = 2 * (t - 2) - 2; sh >= 0; sh -= 2, pos--) { /* n / 4 = 1 << sh */
            for (int task = tid; task < (nb << sh); task += CT_THREADS) {
                const int k = task >> sh, j = task & ((1 << sh) - 1);
                out[k * os + j] = level4(src + k * ss + 4 * j, P + ((size_t)(w0 + k) * L + pos) * 4);
            }
            __syncthreads();
            double *const tmp = src;
            src = out;
            out = tmp;
            const int ts = ss;
            ss = os;
            os = ts;
        }
        if (tid < nb) dst[(size_t)(w0 + tid) * ntiles + tile] = src[tid * ss];
        __syncthreads(); /* the next batch writes sA */
    }
}

/* The subtree of depth D whose first code is `first`, for K windows at once, depth first.  leaf(first, out): the K
 * values of a subtree of depth 2.  row[k]: window k's rows, wave-uniform. */
template <int D, int K, typename Leaf>
__device__ __forceinline__ void subtree(uint32_t first, int L, const sgpr_doubles (&row)[K], Leaf leaf, double (&out)[K])
{
    if constexpr (D == 2) {
        leaf(first, out);
    } else {
#pragma unroll
        for (int k = 0; k < K; k++) out[k] = 0.0;
#pragma nounroll
        for (int b = 0; b < 4; b++) {
            double sub[K];
            subtree<D - 1, K>(first + ((uint32_t)b << (2 * (D - 1))), L, row, leaf, sub);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const double term = sub[k] * row[k][(L - D) * 4 + b];
                out[k] = b == 0 ? term : out[k] + term; /* (not 0.0 + term: that would turn a -0.0 into 0.0) */
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(CT_THREADS) void k_panel_contract(const double *__restrict__ rows, int nm, int ms, int mp_shift,
                                                               const double *__restrict__ P, int nwin, int L, int ntiles,
                                                               double *__restrict__ dst, size_t wstride, size_t tstride)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & ((1 << mp_shift) - 1), g = lane >> mp_shift, G = 64 >> mp_shift;
    const int tile = (blockIdx.y * (CT_THREADS / 64) + wave) * G + g;
    if (tile >= ntiles) return; /* nothing below waits for another lane */
    const int mr = min(m, ms - 1);
    const int w_begin = blockIdx.x * PK_RUN, w_end = min(nwin, w_begin + PK_RUN);
    const sgpr_doubles sp = (sgpr_doubles)P;
    const double *const base = rows + (size_t)mr;
    for (int w0 = w_begin; w0 < w_end; w0 += PK_WIN) {
        sgpr_doubles row[PK_WIN];
#pragma unroll
        for (int k = 0; k < PK_WIN; k++) row[k] = sp + (size_t)min(w0 + k, w_end - 1) * L * 4; /* (past the end: the last window again, not stored) */
        double v[PK_WIN];
        subtree<T, PK_WIN>((uint32_t)tile << (2 * T), L, row,
                           [&](uint32_t first, double (&out)[PK_WIN]) {
                               double x[16];
#pragma unroll
                               for (int c = 0; c < 16; c++) x[c] = base[(size_t)(first + c) * (size_t)ms];
#pragma unroll
                               for (int k = 0; k < PK_WIN; k++) out[k] = leaf16(x, row[k] + (L - 1) * 4, row[k] + (L - 2) * 4);
                           },
                           v);
        if (m < nm) {
#pragma unroll
            for (int k = 0; k < PK_WIN; k++)
                if (w0 + k < w_end) dst[(size_t)(w0 + k) * wstride + (size_t)tile * tstride + (size_t)m] = v[k];
        }
    }
}

/* R = L - t levels over the 4^R partials of (window, column), read at part[w wstride + s tstride + col] */
template <int R>
__global__ __launch_bounds__(CT_THREADS) void k_contract_fold(const double *__restrict__ part, size_t wstride, size_t tstride,
                                                              const double *__restrict__ P, int nwin, int ncol, int L,
                                                              double *__restrict__ out, int ld)
{
    const size_t idx = (size_t)blockIdx.x * CT_THREADS + threadIdx.x;
    if (idx >= (size_t)nwin * (size_t)ncol) return;
    const int w = (int)(idx / (size_t)ncol), col = (int)(idx % (size_t)ncol);
    const double *const src = part + (size_t)w * wstride + (size_t)col;
    const double *const p = P + (size_t)w * L * 4;
    double acc[R];
#pragma unroll
    for (int lev = 0; lev < R; lev++) acc[lev] = 0.0;
    double v = 0.0;
    for (int s = 0; s < (1 << (2 * R)); s++) {
        v = src[(size_t)s * tstride];
        bool go = true;
#pragma unroll
        for (int lev = 0; lev < R; lev++) { /* digit lev of s belongs to position R - 1 - lev */
            if (go) {
                const int b = (s >> (2 * lev)) & 3;
                const double term = v * p[(R - 1 - lev) * 4 + b];
                v = b == 0 ? term : acc[lev] + term;
                acc[lev] = v;
                go = b == 3;
            }
        }
    }
    out[(size_t)w * (size_t)ld + (size_t)col] = v; /* the last s is all threes: v has reached the root */
}

int launch_fold(int R, dim3 grid, hipStream_t stream, const double *part, size_t wstride, size_t tstride, const double *P,
                int nwin, int ncol, int L, double *out, int ld)
{
#define FOLD_CASE(r)                                                                                                      \
    case r:                                                                                                               \
        hipLaunchKernelGGL(k_contract_fold<r>, grid, dim3(CT_THREADS), 0, stream, part, wstride, tstride, P, nwin, ncol, L, \
                           out, ld);                                                                                      \
        break;
    switch (R) {
        FOLD_CASE(1)
        FOLD_CASE(2)
        FOLD_CASE(3)
        FOLD_CASE(4)
        FOLD_CASE(5)
        FOLD_CASE(6)
    default: return set_err_msg("gkm_contract: L - t outside 1..6", 3);
    }
#undef FOLD_CASE
    return 0;
}

int tile_depth(int L) { return std::min(L, CT_T); }

/* doubles of partials for nwin windows: 0 where one tile holds the table */
int64_t part_doubles(int L, int ms, int64_t nwin)
{
    const int t = tile_depth(L);
    return L == t ? 0 : nwin * ((int64_t)1 << (2 * (L - t))) * ms;
}

int64_t max_windows(int L, int ms)
{
    const int64_t per = part_doubles(L, ms, 1) * 8;
    return per ? std::max<int64_t>(1, std::min(CT_MAX_WINDOWS, CT_MAX_SCRATCH / per)) : CT_MAX_WINDOWS;
}

int window_check(const gkmhip_ctx *ctx, const void *P, int64_t nwin, const void *out, int ms, const char *what)
{
    if (!ctx || !P || !out) return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (ctx->L < 2 || ctx->L > 12) return set_err_msg(std::string(what) + ": L outside 2..12", 2);
    if (nwin < 0 || nwin > max_windows(ctx->L, ms))
        return set_err_msg(std::string(what) + ": the windows of one call must number 0.." +
                           std::to_string(max_windows(ctx->L, ms)) + " (gkmhip_contract_max_windows)", 2);
    return 0;
}

} /* namespace */

extern "C" int64_t gkmhip_contract_max_windows(int L, int nm)
{
    if (L < 2 || L > 12 || nm < 0 || nm > GKMHIP_PANEL_MAX) return -1;
    return max_windows(L, nm ? (nm + 7) / 8 * 8 : 1);
}

extern "C" int64_t gkmhip_contract_scratch_bytes(int L, int nm, int64_t nwin)
{
    const int64_t cap = gkmhip_contract_max_windows(L, nm);
    if (cap < 0 || nwin < 0 || nwin > cap) return -1;
    return part_doubles(L, nm ? (nm + 7) / 8 * 8 : 1, nwin) * 8;
}

extern "C" int gkmhip_lmer_contract(gkmhip_ctx *ctx, const double *W, const double *P, int64_t nwin, double *out, void *stream_)
{
    if (int rc = window_check(ctx, P, nwin, out, 1, "gkmhip_lmer_contract")) return rc;
    if (!W) return set_err_msg("gkmhip_lmer_contract: bad arguments", 2);
    if (nwin == 0) return 0;
    const int L = ctx->L, t = tile_depth(L), ntiles = 1 << (2 * (L - t));
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    double *dst = out;
    if (ntiles > 1) {
        if (ctx->contract_part.ensure((size_t)part_doubles(L, 1, nwin), true)) return 4;
        dst = ctx->contract_part.p;
    }
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_lmer_contract, dim3((unsigned)((nwin + CT_RUN - 1) / CT_RUN), (unsigned)ntiles), dim3(CT_THREADS), 0,
                       stream, W, P, (int)nwin, L, t, ntiles, dst);
    if (ntiles > 1)
        if (int rc = launch_fold(L - t, dim3((unsigned)((nwin + CT_THREADS - 1) / CT_THREADS)), stream, dst, (size_t)ntiles, 1, P,
                                 (int)nwin, 1, L, out, 1))
            return rc;
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_lmer_contract", (double)nwin * (double)((int64_t)1 << (2 * L)));
    return 0;
}

extern "C" int gkmhip_panel_contract(gkmhip_ctx *ctx, const double *rows, int nm, int ms, const double *P, int64_t nwin,
                                     double *out, int64_t ld, void *stream_)
{
    if (int rc = panel_check(rows, nm, ms, "gkmhip_panel_contract")) return rc;
    if (int rc = window_check(ctx, P, nwin, out, ms, "gkmhip_panel_contract")) return rc;
    if (ld < nm || ld > INT32_MAX) return set_err_msg("gkmhip_panel_contract: the leading dimension must be at least the number of models", 2);
    if (nwin == 0) return 0;
    const int L = ctx->L, t = tile_depth(L), ntiles = 1 << (2 * (L - t));
    const int sh = panel_shift(nm), G = 64 >> sh, per_block = (CT_THREADS / 64) * G;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    double *dst = out;
    size_t wstride = (size_t)ld, tstride = 0;
    if (ntiles > 1) {
        if (ctx->contract_part.ensure((size_t)part_doubles(L, ms, nwin), true)) return 4;
        dst = ctx->contract_part.p;
        wstride = (size_t)ntiles * (size_t)ms;
        tstride = (size_t)ms;
    }
    const dim3 grid((unsigned)((nwin + PK_RUN - 1) / PK_RUN), (unsigned)((ntiles + per_block - 1) / per_block));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
#define PANEL_CASE(T)                                                                                                      \
    case T:                                                                                                                \
        hipLaunchKernelGGL(k_panel_contract<T>, grid, dim3(CT_THREADS), 0, stream, rows, nm, ms, sh, P, (int)nwin, L, ntiles, \
                           dst, wstride, tstride);                                                                         \
        break;
    switch (t) {
        PANEL_CASE(2)
        PANEL_CASE(3)
        PANEL_CASE(4)
        PANEL_CASE(5)
        PANEL_CASE(6)
    }
#undef PANEL_CASE
    if (ntiles > 1) {
        const size_t cells = (size_t)nwin * (size_t)nm;
        if (int rc = launch_fold(L - t, dim3((unsigned)((cells + CT_THREADS - 1) / CT_THREADS)), stream, dst, wstride, tstride, P,
                                 (int)nwin, nm, L, out, (int)ld))
            return rc;
    }
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_contract", (double)nwin * (double)nm * (double)((int64_t)1 << (2 * L)));
    return 0;
}
