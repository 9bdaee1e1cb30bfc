/*
 * gkm_wsim.hip -- windowed kernel matrices between two long sequences: the gkm kernel between every window
 * of W bases of a record x (stride sx) and every window of a record y (stride sy), each pair as if the two windows were
 * sequences of their own.  With n = W - L + 1 l-mers per window, window i of x starting at l-mer a_i = i sx and window j
 * of y at b_j = j sy, f the forward l-mers of x and g those of y,
 *
 *   P_m(i, j) = sum_{p in [a_i, a_i + n)} sum_{q in [b_j, b_j + n)} ([m(f_p, g_q) = m] + [m(f_p, rc g_q) = m])     exact
 *   G(i, j)   = ((0.0 + c_0 P_0) + c_1 P_1) + ... + c_d P_d                  the Gram epilogue's order, no contraction
 *   K(i, j)   = G(i, j) / (sq_x(i) sq_y(j)), RBF: exp(gamma (K - 1))         k_normalize_full's arithmetic
 *
 * Only the unweighted kernel types are served: with positional weights a hit's value would depend on the window.  Like
 * the scan the kernels take the context for L, d, the coefficients and gamma only, and plain device pointers: the words
 * of gkmhip_scan_lmers of either record.
 *
 * Kernels
 *   k_wsim_profiles   HOT.  One workgroup owns a tile of gx x gy window pairs.  It stages the Sy = n + (gy - 1) sy words
 *                     of y the tile's columns cover in LDS, and beside each the interval of the tile's columns that hold
 *                     it.  Each lane holds f_p and rc f_p of two of the Sx = n + (gx - 1) sx l-mers of x in registers
 *                     with the interval of the tile's rows that hold p.  Wave w walks its quarter of the words of y (a
 *                     broadcast read) and compares: every (p, q) once per strand for the whole tile, not once per window
 *                     pair.  A hit with m mismatches adds 1 to the rectangle [i_lo, i_hi] x [j_lo, j_hi] of window pairs:
 *                     four integer LDS atomics on the corners of a signed difference array D[m][gx + 1][gy + 1], which an
 *                     inclusive 2-D prefix sum per class turns into P_m at the end of the tile.  Integer adds commute, so
 *                     the bytes are the same on every run; 2 n^2 <= 8.4e6 never wraps 32 bits.  No float atomics, and no
 *                     workgroup waits for another.
 *   k_wsim_normalize  K = G / (sqx[i] sqy[j]), RBF fold, in place.  A NaN norm makes its row or column NaN: that is
 *                     how a window over an invalid base is marked, so no validity array reaches the kernels.
 *   k_wsim_best       per row the eligible column (|a_i - b_j| >= min_separation, in bases) with the largest K, the lower j
 *                     on a tie; a NaN never wins; index -1 and NaN where there is none.  One wave per row, shuffles.
 *
 * A flagged word (gkmhip_scan_lmers' bit 31) takes part in no pair.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_WAVES = WS_THREADS / 64;
constexpr int WS_GMAX = 32;       /* windows of a tile along either axis: D of 13 classes stays at 57 KB */
constexpr int WS_STRETCH = 4096;  /* l-mer words of a tile along either axis, at most (as the scan's stretch) */
constexpr int WS_R = 2;           /* l-mers of x a lane holds at a time */
constexpr int WB_THREADS = 256;   /* four rows per workgroup in k_wsim_best */

/* windows of a tile along one axis: a function of (n, s) -- that is of (L, W, s) -- only */
inline int wsim_group(int n, int s)
{
    if (s >= n) return 1; /* windows share no l-mer */
    return (int)std::min<int64_t>(WS_GMAX, 1 + (WS_STRETCH - n) / s);
}

/* sum over the tiles of an axis of their stretch lengths n + (windows - 1) s */
inline double axis_words(int n, int s, int g, int64_t nw)
{
    const int64_t tiles = (nw + g - 1) / g;
    const int last = (int)(nw - (tiles - 1) * g);
    return (double)(tiles - 1) * ((double)n + (double)(g - 1) * s) + (double)n + (double)(last - 1) * s;
}

__device__ __forceinline__ void wsim_credit(int *Dm, int rlo, int rhi, int jlo, int jhi)
{
    atomicAdd(Dm + rlo + jlo, 1);
    atomicAdd(Dm + rlo + jhi, -1);
    atomicAdd(Dm + rhi + jlo, -1);
    atomicAdd(Dm + rhi + jhi, 1);
}

/* lmx, lmy: the words from the launch's first window's first l-mer on.  Tile (ti, tj) = blockIdx.x / tiles_y, % tiles_y.
 * Dynamic LDS: D[d + 1][gx + 1][gy + 1] ints, the n + (gy - 1) sy words of y, their column intervals (16 bits each). */
__global__ __launch_bounds__(WS_THREADS) void k_wsim_profiles(const uint32_t *__restrict__ lmx, const uint32_t *__restrict__ lmy,
                                                              int n, int sx, int sy, int gx, int gy, int64_t nwx, int64_t nwy,
                                                              int64_t tiles_y, int L, int d, LmerCoef C, double *__restrict__ G,
                                                              int64_t ld, int32_t *__restrict__ prof)
{
    extern __shared__ int wsim_lds[];
    const int gy1 = gy + 1, plane = (gx + 1) * gy1;
    int *D = wsim_lds;
    uint32_t *sl = (uint32_t *)(D + (d + 1) * plane);
    uint16_t *jr = (uint16_t *)(sl + n + (gy - 1) * sy);
    const int64_t ti = (int64_t)blockIdx.x / tiles_y, tj = (int64_t)blockIdx.x - ti * tiles_y;
    const int64_t i0 = ti * gx, j0 = tj * gy;
    const int gxw = (int)min((int64_t)gx, nwx - i0), gyw = (int)min((int64_t)gy, nwy - j0);
    const int Sx = n + (gxw - 1) * sx, Sy = n + (gyw - 1) * sy;
    const uint32_t *srcx = lmx + i0 * sx, *srcy = lmy + j0 * sy;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < (d + 1) * plane; e += WS_THREADS) D[e] = 0;
    for (int q = tid; q < Sy; q += WS_THREADS) {
        sl[q] = srcy[q];
        /* the columns j with j sy <= q < j sy + n */
        const int jlo = q < n ? 0 : (q - n) / sy + 1, jhi = min(gyw, q / sy + 1);
        jr[q] = (uint16_t)(jlo | (jhi << 8));
    }
    __syncthreads();
    const int q0 = (int)((int64_t)Sy * wave / WS_WAVES), q1 = (int)((int64_t)Sy * (wave + 1) / WS_WAVES);
    for (int base = 0; base < Sx; base += 64 * WS_R) {
        uint32_t xf[WS_R], xr[WS_R];
        int dl[WS_R], rlo[WS_R], rhi[WS_R];
#pragma unroll
        for (int r = 0; r < WS_R; r++) {
            const int p = base + r * 64 + lane;
            const uint32_t xe = srcx[min(p, Sx - 1)];
            xf[r] = xe & LMER_CODE;
            xr[r] = lmer_rc(xf[r], L);
            dl[r] = (p < Sx && !(xe & LMER_BAD)) ? d : -1; /* no count is at most -1: the lane never hits */
            /* the rows i with i sx <= p < i sx + n */
            rlo[r] = (p < n ? 0 : (p - n) / sx + 1) * gy1;
            rhi[r] = min(gxw, p / sx + 1) * gy1;
        }
        for (int q = q0; q < q1; q++) {
            const uint32_t ye = sl[q]; /* (wave-uniform: a broadcast) */
            if (ye & LMER_BAD) continue;
            const uint32_t yc = ye & LMER_CODE;
#pragma unroll
            for (int r = 0; r < WS_R; r++) {
                const int mf = lmer_mm(xf[r], yc), mr = lmer_mm(xr[r], yc);
                if (min(mf, mr) <= dl[r]) {
                    const int jj = jr[q], jlo = jj & 0xFF, jhi = jj >> 8;
                    if (rlo[r] < rhi[r] && jlo < jhi) {
                        if (mf <= d) wsim_credit(D + mf * plane, rlo[r], rhi[r], jlo, jhi);
                        if (mr <= d) wsim_credit(D + mr * plane, rlo[r], rhi[r], jlo, jhi);
                    }
                }
            }
        }
    }
    __syncthreads();
    /* inclusive prefix sums: along j in every row, then along i in every column (the row and column beyond the tile's
     * windows only ever take the closing corners and are not read) */
    for (int e = tid; e < (d + 1) * gxw; e += WS_THREADS) {
        const int m = e / gxw, i = e - m * gxw;
        int *row = D + m * plane + i * gy1;
        int t = 0;
        for (int j = 0; j < gyw; j++) {
            t += row[j];
            row[j] = t;
        }
    }
    __syncthreads();
    for (int e = tid; e < (d + 1) * gyw; e += WS_THREADS) {
        const int m = e / gyw, j = e - m * gyw;
        int *col = D + m * plane + j;
        int t = 0;
        for (int i = 0; i < gxw; i++) {
            t += col[i * gy1];
            col[i * gy1] = t;
        }
    }
    __syncthreads();
    for (int e = tid; e < gxw * gyw; e += WS_THREADS) {
        const int i = e / gyw, j = e - i * gyw;
        const int *cell = D + i * gy1 + j;
        double g = 0.0;
        for (int m = 0; m <= d; m++) g = g + C.c[m] * (double)cell[m * plane];
        G[(i0 + i) * ld + (j0 + j)] = g;
        if (prof) {
            int32_t *o = prof + ((i0 + i) * nwy + (j0 + j)) * (d + 1);
            for (int m = 0; m <= d; m++) o[m] = cell[m * plane];
        }
    }
}

__global__ __launch_bounds__(256) void k_wsim_normalize(double *__restrict__ G, int64_t ld, int64_t nwx, int64_t nwy,
                                                        const double *__restrict__ sqx, const double *__restrict__ sqy,
                                                        int rbf, double gamma)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nwx * nwy) return;
    const int64_t i = e / nwy, j = e - i * nwy;
    double v = G[i * ld + j] / (sqx[i] * sqy[j]); /* product first, one division: k_normalize_full */
    if (rbf) v = exp(gamma * (v - 1));
    G[i * ld + j] = v;
}

/* (v, j) replaces (bv, bj): a column at all, a larger value, or the same value at a lower column.  Exact and associative;
 * a NaN is never offered (the callers test for it). */
__device__ __forceinline__ bool wsim_better(double v, int64_t j, double bv, int64_t bj)
{
    return j >= 0 && (bj < 0 || v > bv || (v == bv && j < bj));
}

__global__ __launch_bounds__(WB_THREADS) void k_wsim_best(const double *__restrict__ K, int64_t ld, int64_t nwx, int64_t nwy,
                                                          int64_t x0, int64_t sx, int64_t y0, int64_t sy, int64_t min_sep,
                                                          int64_t *__restrict__ best_j, double *__restrict__ best_k)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (WB_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nwx) return; /* a whole wave: nothing below waits for the workgroup */
    const int64_t a = x0 + i * sx;
    const double *row = K + i * ld;
    double bv = __builtin_nan("");
    int64_t bj = -1;
    for (int64_t j = lane; j < nwy; j += 64) {
        const int64_t b = y0 + j * sy, gap = a > b ? a - b : b - a;
        const double v = row[j];
        if (gap >= min_sep && v == v && wsim_better(v, j, bv, bj)) {
            bv = v;
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int64_t oj = (int64_t)__shfl_xor((long long)bj, o, 64);
        if (wsim_better(ov, oj, bv, bj)) {
            bv = ov;
            bj = oj;
        }
    }
    if (lane == 0) {
        best_j[i] = bj;
        best_k[i] = bv;
    }
}

/* the shape every launch over a block of window pairs checks: 0, or error 2 after set_err_msg */
int wsim_check_block(int64_t nwx, int64_t nwy, int64_t ld, const char *what)
{
    if (nwx < 1 || nwy < 1 || nwx > (int64_t)1 << 30 || nwy > (int64_t)1 << 30 || nwx * nwy > (int64_t)1 << 38)
        return set_err_msg(std::string(what) + ": needs 1..2^30 windows on each axis and at most 2^38 pairs", 2);
    if (ld < nwy) return set_err_msg(std::string(what) + ": leading dimension too small", 2);
    return 0;
}

} /* namespace */

extern "C" int gkmhip_wsim_group(int L, int d, int width, int stride_x, int stride_y, int *gx, int *gy)
{
    if (gx) *gx = 0;
    if (gy) *gy = 0;
    if (!gx || !gy || L < 1 || L > 12 || d < 0 || d >= GKM_MAXD1 || d > L || width < L || width > GKM_MAXLEN ||
        stride_x < 1 || stride_y < 1)
        return 2;
    *gx = wsim_group(width - L + 1, stride_x);
    *gy = wsim_group(width - L + 1, stride_y);
    return 0;
}

extern "C" int gkmhip_wsim_profiles(gkmhip_ctx *ctx, const uint32_t *lmx, int64_t nlmx, const uint32_t *lmy, int64_t nlmy,
                                    int width, int stride_x, int stride_y, int64_t nwx, int64_t nwy, double *G, int64_t ld,
                                    int32_t *prof, void *stream_)
{
    const char *what = "gkmhip_wsim_profiles";
    if (!ctx || !lmx || !lmy || !G) return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (width < ctx->L || width > GKM_MAXLEN)
        return set_err_msg(std::string(what) + ": the width must lie in L.." + std::to_string(GKM_MAXLEN), 2);
    if (stride_x < 1 || stride_y < 1) return set_err_msg(std::string(what) + ": the strides must be at least 1", 2);
    if (int rc = wsim_check_block(nwx, nwy, ld, what)) return rc;
    const int n = width - ctx->L + 1, d = ctx->d;
    if ((nwx - 1) * (int64_t)stride_x + n > nlmx || (nwy - 1) * (int64_t)stride_y + n > nlmy)
        return set_err_msg(std::string(what) + ": the windows must lie inside the l-mer words given", 2);
    const int gx = wsim_group(n, stride_x), gy = wsim_group(n, stride_y);
    const int64_t tiles_x = (nwx + gx - 1) / gx, tiles_y = (nwy + gy - 1) / gy;
    if (tiles_x * tiles_y > 0x7FFFFFFF) return set_err_msg(std::string(what) + ": more than 2^31 - 1 tiles in one launch", 2);
    const size_t sy_words = (size_t)n + (size_t)(gy - 1) * stride_y;
    const size_t lds = (size_t)(d + 1) * (gx + 1) * (gy + 1) * 4 + sy_words * 4 + ((sy_words * 2 + 3) & ~(size_t)3);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    /* at most 13 x 33 x 33 x 4 + 4096 x 6 = 81 204 bytes (d = 12, both axes at 32 windows and a full stretch) */
    HIPCHK(hipFuncSetAttribute((const void *)k_wsim_profiles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_wsim_profiles, dim3((unsigned)(tiles_x * tiles_y)), dim3(WS_THREADS), lds, stream, lmx, lmy, n,
                       stride_x, stride_y, gx, gy, nwx, nwy, tiles_y, ctx->L, d, lmer_coef(ctx->c, d), G, ld, prof);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_wsim_profiles", 2.0 * axis_words(n, stride_x, gx, nwx) * axis_words(n, stride_y, gy, nwy));
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: window pairs, %lld x %lld windows of %d l-mers at strides %d, %d -> k_wsim_profiles (%lld "
                        "tiles of %d x %d windows, %zu bytes of LDS, %.3g comparisons)\n", (long long)nwx, (long long)nwy, n,
                stride_x, stride_y, (long long)(tiles_x * tiles_y), gx, gy, lds, ctx->last_comparisons);
    return 0;
}

extern "C" int gkmhip_wsim_normalize(gkmhip_ctx *ctx, double *G, int64_t ld, int64_t nwx, int64_t nwy, const double *sqx,
                                     const double *sqy, void *stream_)
{
    if (!ctx || !G || !sqx || !sqy) return set_err_msg("gkmhip_wsim_normalize: bad arguments", 2);
    if (int rc = wsim_check_block(nwx, nwy, ld, "gkmhip_wsim_normalize")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_wsim_normalize, dim3((unsigned)((nwx * nwy + 255) / 256)), dim3(256), 0, stream, G, ld, nwx, nwy, sqx,
                       sqy, ctx->rbf, ctx->gamma);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_wsim_normalize", (double)nwx * (double)nwy); /* (values normalised) */
    return 0;
}

extern "C" int gkmhip_wsim_best(gkmhip_ctx *ctx, const double *K, int64_t ld, int64_t nwx, int64_t nwy, int64_t start_x,
                                int64_t stride_x, int64_t start_y, int64_t stride_y, int64_t min_separation, int64_t *best_j,
                                double *best_k, void *stream_)
{
    const int64_t far = (int64_t)1 << 40; /* starts, strides and separations stay far from 64-bit overflow */
    if (!ctx || !K || !best_j || !best_k) return set_err_msg("gkmhip_wsim_best: bad arguments", 2);
    if (int rc = wsim_check_block(nwx, nwy, ld, "gkmhip_wsim_best")) return rc;
    if (stride_x < 1 || stride_y < 1 || stride_x > GKM_MAXLEN * 4096 || stride_y > GKM_MAXLEN * 4096)
        return set_err_msg("gkmhip_wsim_best: the strides must be at least 1", 2);
    if (start_x < 0 || start_y < 0 || start_x > far || start_y > far || min_separation < 0 || min_separation > far)
        return set_err_msg("gkmhip_wsim_best: the starts and the separation must lie in 0..2^40", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const int per = WB_THREADS / 64;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_wsim_best, dim3((unsigned)((nwx + per - 1) / per)), dim3(WB_THREADS), 0, stream, K, ld, nwx, nwy,
                       start_x, stride_x, start_y, stride_y, min_separation, best_j, best_k);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_wsim_best", (double)nwx * (double)nwy); /* (values looked at) */
    return 0;
}
