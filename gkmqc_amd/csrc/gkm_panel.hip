/*
 * gkm_panel.hip -- l-mer weight panels: nm <= 64 weight tables that share (kernel_type, L, k, d, M, H),
 * interleaved so that one l-mer's weights for all models form one contiguous row,
 *
 *   P[u * ms + m] = W_m[u]        (ms = nm rounded up to a multiple of 8: rows of whole 64-byte lines; zero beyond nm)
 *
 * and the LANES ACROSS MODELS: one l-mer lookup serves the whole panel with one coalesced read where the single-table
 * kernels make one scattered 8-byte gather per model.  With mp = nm rounded up to 8, 16, 32 or 64, a wave holds G = 64 / mp
 * items (or groups of one item), lane = (group g, model m) = g * mp + m.
 *
 * The contract: for every model m the value written is what the single-table kernel writes for the table P[:, m], bit for
 * bit.  Each term is a rounded product followed by a rounded add (-ffp-contract=off), so only the order of the adds has to
 * match; an add of two operands is commutative, so which lane holds a partial sum does not matter, the tree's shape does.
 *
 * Kernels
 *   k_panel_score           one wave per query (gkm_lmer.hip k_lmer_score).  The single-table kernel keeps 64 partial sums,
 *                           residue l over p = l, l + 64, ... ascending from 0.0, and adds them in the butterfly o = 32 .. 1.
 *                           Here group g owns the residues r * G + g, r < mp, in mp accumulators indexed at compile time;
 *                           a butterfly level o >= G pairs two registers of the lane (r and r ^ o / G), a level o < G is a
 *                           __shfl_xor across groups (lane ^ o * mp).
 *   k_panel_scan_score      the same tree per window (gkm_scan.hip k_scan_score): the weight of position p from wt[p], the
 *                           l-mer from the window's words
 * The two share the tree's shape only (panel_tree); their lane mappings differ from the single-table kernels' on purpose
 * (lane = (group, model) against lane = residue), so they stay kernels of their own.  The two delta kernels of a panel,
 * k_panel_delta_variants and k_panel_delta_sat, are one lane's own chain per (item, model) and share their bodies with
 * the single-table kernels: they live in gkm_delta.hip, which uses panel_check and panel_shift below.
 *
 * Lanes m >= nm read inside the row (clamped to its last column) and never store.  No atomics; nothing depends on the
 * launch geometry.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int PN_THREADS = 256; /* four queries or windows per workgroup in the two tree kernels */
constexpr int PN_MAX = 64;      /* models of a panel */
constexpr int PT_BATCH = 8;     /* rows a lane keeps in flight in the two tree kernels */

/* The butterfly tree of one item for this lane's model.  fetch(p, u, w): the code and the weight of position p < n.
 * mr: the column this lane reads.  Every lane of the wave must call it (the cross-group levels are wave-wide). */
template <int MP, typename Fetch>
__device__ __forceinline__ double panel_tree(const double *__restrict__ P, int ms, int mr, int g, int n, Fetch fetch)
{
    constexpr int G = 64 / MP;
    constexpr int B = MP < PT_BATCH ? MP : PT_BATCH;
    double acc[MP];
#pragma unroll
    for (int r = 0; r < MP; r++) acc[r] = 0.0;
    int base = 0;
    /* whole blocks of 64 positions, residue r * G + g in acc[r]: nothing is conditional, so the B l-mer words of a batch
     * are fetched together and then their B rows */
    for (; base + 64 <= n; base += 64) {
#pragma unroll
        for (int r0 = 0; r0 < MP; r0 += B) {
            uint32_t u[B];
            double w[B];
#pragma unroll
            for (int r = 0; r < B; r++) fetch(base + (r0 + r) * G + g, u[r], w[r]);
            double x[B];
#pragma unroll
            for (int r = 0; r < B; r++) x[r] = P[(size_t)u[r] * (size_t)ms + (size_t)mr];
#pragma unroll
            for (int r = 0; r < B; r++) acc[r0 + r] += w[r] * x[r];
        }
    }
    /* the last n % 64 positions */
    if (base < n) {
#pragma unroll
        for (int r = 0; r < MP; r++) {
            const int p = base + r * G + g;
            if (p < n) {
                uint32_t u;
                double w;
                fetch(p, u, w);
                acc[r] += w * P[(size_t)u * (size_t)ms + (size_t)mr];
            }
        }
    }
    /* levels o = 32 .. G: residues r * G + g and (r ^ o / G) * G + g, both this lane's */
#pragma unroll
    for (int h = MP / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int r = 0; r < h; r++) acc[r] += acc[r + h];
    }
    double t = acc[0];
    /* levels o = G / 2 .. 1: group g ^ o, the same model */
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) t += __shfl_xor(t, o * MP, 64);
    return t;
}

template <int MP>
__global__ __launch_bounds__(PN_THREADS) void k_panel_score(const uint32_t *__restrict__ lmf,
                                                            const int64_t *__restrict__ lmoff,
                                                            const int *__restrict__ len, int L, int col_begin, int col_end,
                                                            const double *__restrict__ P, int nm, int ms,
                                                            double *__restrict__ out)
{
    const int lane = threadIdx.x & 63, m = lane & (MP - 1), g = lane / MP;
    const int j = col_begin + blockIdx.x * (PN_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= col_end) return; /* a whole wave: nothing below waits for the workgroup */
    const int n = len[j] - L + 1;
    const uint32_t *e = lmf + lmoff[j];
    const double t = panel_tree<MP>(P, ms, min(m, ms - 1), g, n, [e](int p, uint32_t &u, double &w) {
        const uint32_t x = e[p]; /* l-mer | weight << 24 (k_pack_lmers) */
        u = x & LMER_CODE;
        w = (double)(x >> LMER_WSHIFT);
    });
    if (g == 0 && m < nm) out[(size_t)(j - col_begin) * (size_t)nm + (size_t)m] = t;
}

template <int MP>
__global__ __launch_bounds__(PN_THREADS) void k_panel_scan_score(const uint32_t *__restrict__ lm,
                                                                 const uint8_t *__restrict__ wt, int n, int s, int64_t nwin,
                                                                 const double *__restrict__ P, int nm, int ms,
                                                                 double *__restrict__ out)
{
    const int lane = threadIdx.x & 63, m = lane & (MP - 1), g = lane / MP;
    const int64_t i = (int64_t)blockIdx.x * (PN_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nwin) return; /* a whole wave */
    const uint32_t *e = lm + i * s;
    const double t = panel_tree<MP>(P, ms, min(m, ms - 1), g, n, [e, wt](int p, uint32_t &u, double &w) {
        u = e[p] & LMER_CODE;
        w = (double)wt[p];
    });
    if (g == 0 && m < nm) out[(size_t)i * (size_t)nm + (size_t)m] = t;
}

} /* namespace */

/* what every panel entry refuses, gkm_delta.hip's two included; 0 or error 2 */
int panel_check(const void *P, int nm, int ms, const char *what)
{
    if (!P) return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (nm < 1 || nm > PN_MAX)
        return set_err_msg(std::string(what) + ": a panel holds 1.." + std::to_string(PN_MAX) + " models", 2);
    if (ms < nm || ms % 8 != 0)
        return set_err_msg(std::string(what) + ": the row stride must be a multiple of 8 and at least the number of models", 2);
    return 0;
}

/* log2 of mp: nm rounded up to 8, 16, 32 or 64 */
int panel_shift(int nm) { return nm <= 8 ? 3 : nm <= 16 ? 4 : nm <= 32 ? 5 : 6; }

#define PANEL_DISPATCH(sh, kernel, grid, stream, ...)                                                          \
    switch (sh) {                                                                                              \
    case 3: hipLaunchKernelGGL(kernel<8>, grid, dim3(PN_THREADS), 0, stream, __VA_ARGS__); break;              \
    case 4: hipLaunchKernelGGL(kernel<16>, grid, dim3(PN_THREADS), 0, stream, __VA_ARGS__); break;             \
    case 5: hipLaunchKernelGGL(kernel<32>, grid, dim3(PN_THREADS), 0, stream, __VA_ARGS__); break;             \
    default: hipLaunchKernelGGL(kernel<64>, grid, dim3(PN_THREADS), 0, stream, __VA_ARGS__); break;            \
    }

extern "C" int gkmhip_panel_score(gkmhip_ctx *ctx, int col_begin, int col_end, const double *P, int nm, int ms, double *out,
                                  void *stream_)
{
    if (!ctx || !out) return set_err_msg("gkmhip_panel_score: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_score")) return rc;
    if (int rc = check_range(ctx, col_begin, col_end, "gkmhip_panel_score")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    const int per = PN_THREADS / 64;
    const dim3 grid((unsigned)((col_end - col_begin + per - 1) / per));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    PANEL_DISPATCH(panel_shift(nm), k_panel_score, grid, stream, (const uint32_t *)ctx->lmf.p, (const int64_t *)ctx->lmoff.p,
                   (const int *)ctx->len.p, ctx->L, col_begin, col_end, P, nm, ms, out)
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_score", ctx->h_cum_n[(size_t)col_end] - ctx->h_cum_n[(size_t)col_begin]); /* (rows looked up) */
    return 0;
}

extern "C" int gkmhip_panel_scan_score(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width,
                                       int stride, int64_t nwin, const double *P, int nm, int ms, double *out, void *stream_)
{
    const int n = scan_check(ctx, lm, nlm, wt, width, stride, nwin, out, "gkmhip_panel_scan_score");
    if (n < 0) return -n;
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_scan_score")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const int per = PN_THREADS / 64;
    const dim3 grid((unsigned)((nwin + per - 1) / per));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    PANEL_DISPATCH(panel_shift(nm), k_panel_scan_score, grid, stream, lm, wt, n, stride, nwin, P, nm, ms, out)
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_scan_score", (double)nwin * n); /* (rows looked up) */
    return 0;
}
