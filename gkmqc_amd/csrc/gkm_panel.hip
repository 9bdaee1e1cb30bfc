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
 *   k_panel_delta_variants  lane = (variant, model), G variants per wave: k_delta_variants' two chains
 *   k_panel_delta_sat       lane = (position, model), G positions per wave: k_delta_sat's four chains
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

/* sh: log2(mp).  Thread (i << sh) + m is (variant i, model m); everything else as k_delta_variants. */
__global__ __launch_bounds__(PN_THREADS) void k_panel_delta_variants(const uint32_t *__restrict__ lm,
                                                                     const uint8_t *__restrict__ codes, int nbases, int L,
                                                                     const int4 *__restrict__ var, int nvar,
                                                                     const uint8_t *__restrict__ alt, int nalt,
                                                                     const double *__restrict__ P, int nm, int ms, int sh,
                                                                     double *__restrict__ out)
{
    const int64_t tid = (int64_t)blockIdx.x * PN_THREADS + threadIdx.x;
    const int64_t i = tid >> sh;
    const int m = (int)(tid & ((1 << sh) - 1));
    if (i >= nvar) return;
    const double *col = P + min(m, ms - 1);
    const size_t row = (size_t)ms;
    double *dst = out + (size_t)i * (size_t)nm + (size_t)m;
    const int4 v = var[i];
    const int pos = v.x, r = v.y, aoff = v.z, al = v.w;
    if (pos < 0 || r < 0 || pos > nbases - r || aoff < 0 || al < 0 || aoff > nalt - al) {
        if (m < nm) *dst = __builtin_nan("");
        return;
    }
    const int a = max(0, pos - (L - 1)), e = min(nbases, pos + r + (L - 1));
    double ref = 0.0;
    for (int p = a; p + L <= e; p++) ref += col[(size_t)(lm[p] & LMER_CODE) * row];
    const uint32_t mask = (uint32_t)((1ull << (2 * L)) - 1ull);
    uint32_t u = 0u;
    int have = 0; /* bases rolled in so far */
    double sum = 0.0;
    for (int q = a; q < pos; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += col[(size_t)u * row];
    }
    for (int q = 0; q < al; q++) {
        u = ((u << 2) | (uint32_t)(alt[aoff + q] & 3)) & mask;
        if (++have >= L) sum += col[(size_t)u * row];
    }
    for (int q = pos + r; q < e; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += col[(size_t)u * row];
    }
    if (m < nm) *dst = sum - ref;
}

/* Thread (i << sh) + m is (position t0 + i, model m) -> out[((t - t0) * 4 + b) * nm + m]; everything else as k_delta_sat. */
__global__ __launch_bounds__(PN_THREADS) void k_panel_delta_sat(const uint32_t *__restrict__ lm, int64_t nlm, int L,
                                                                int64_t t0, int64_t t1, const double *__restrict__ P,
                                                                int nm, int ms, int sh, double *__restrict__ out)
{
    const int64_t tid = (int64_t)blockIdx.x * PN_THREADS + threadIdx.x;
    const int64_t t = t0 + (tid >> sh);
    const int m = (int)(tid & ((1 << sh) - 1));
    if (t >= t1) return;
    const double *col = P + min(m, ms - 1);
    const size_t row = (size_t)ms;
    const int64_t p0 = max((int64_t)0, t - L + 1), p1 = min(t, nlm - 1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t flags = 0u, last = 0u;
    int shp = 2 * (L - 1 - (int)(t - p0)); /* the pair of base t in l-mer p0; two more per step */
#pragma unroll 2
    for (int64_t p = p0; p <= p1; p++, shp += 2) {
        const uint32_t e = lm[p];
        const uint32_t u = e & LMER_CODE;
        flags |= e;
        last = u;
        s0 += col[(size_t)u * row];
        s1 += col[(size_t)(u ^ (1u << shp)) * row];
        s2 += col[(size_t)(u ^ (2u << shp)) * row];
        s3 += col[(size_t)(u ^ (3u << shp)) * row];
    }
    if (m >= nm) return;
    const uint32_t xt = (last >> (shp - 2)) & 3u; /* (shp - 2: the pair of t in l-mer p1) */
    double c0, c1, c2, c3;
    if (flags & LMER_BAD) {
        c0 = c1 = c2 = c3 = __builtin_nan("");
    } else {
        const double d1 = s1 - s0, d2 = s2 - s0, d3 = s3 - s0;
        /* column b holds chain j = b ^ x_t */
        c0 = xt == 0 ? 0.0 : xt == 1 ? d1 : xt == 2 ? d2 : d3;
        c1 = xt == 1 ? 0.0 : xt == 0 ? d1 : xt == 3 ? d2 : d3;
        c2 = xt == 2 ? 0.0 : xt == 3 ? d1 : xt == 0 ? d2 : d3;
        c3 = xt == 3 ? 0.0 : xt == 2 ? d1 : xt == 1 ? d2 : d3;
    }
    double *dst = out + (size_t)(t - t0) * 4u * (size_t)nm + (size_t)m;
    dst[0] = c0;
    dst[(size_t)nm] = c1;
    dst[2 * (size_t)nm] = c2;
    dst[3 * (size_t)nm] = c3;
}

/* what every panel entry refuses; 0 or error 2 */
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
inline int panel_shift(int nm) { return nm <= 8 ? 3 : nm <= 16 ? 4 : nm <= 32 ? 5 : 6; }

/* sum over positions s < t of the l-mers (of nlm) that cover s (as gkm_delta.hip counts k_delta_sat's gathers) */
double panel_covered_below(int64_t t, int64_t nlm, int L)
{
    const int64_t whole = std::min(nlm, std::max<int64_t>(0, t - L + 1));
    double g = (double)whole * L;
    for (int64_t p = whole; p < std::min(nlm, t); p++) g += (double)(t - p);
    return g;
}

/* as gkm_scan.hip's scan_check: n, or a negative value after set_err_msg */
int panel_scan_check(const gkmhip_ctx *ctx, const void *lm, int64_t nlm, const void *wt, int width, int stride, int64_t nwin,
                     const void *out, const char *what)
{
    if (!ctx || !lm || !wt || !out) return -set_err_msg(std::string(what) + ": bad arguments", 2);
    if (width < ctx->L || width > GKM_MAXLEN)
        return -set_err_msg(std::string(what) + ": the width must lie in L.." + std::to_string(GKM_MAXLEN), 2);
    if (stride < 1) return -set_err_msg(std::string(what) + ": the stride must be at least 1", 2);
    const int n = width - ctx->L + 1;
    if (nwin < 1 || nwin > (int64_t)1 << 30 || (nwin - 1) * (int64_t)stride + n > nlm)
        return -set_err_msg(std::string(what) + ": the windows must lie inside the l-mer words given", 2);
    return n;
}

} /* namespace */

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
    const int n = panel_scan_check(ctx, lm, nlm, wt, width, stride, nwin, out, "gkmhip_panel_scan_score");
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

extern "C" int gkmhip_panel_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end,
                                      const double *P, int nm, int ms, double *out, void *stream_)
{
    if (!ctx || !lm || !out) return set_err_msg("gkmhip_panel_delta_sat: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_delta_sat")) return rc;
    if (nlm < 1 || t_begin < 0 || t_begin >= t_end || t_end > nlm + ctx->L - 1)
        return set_err_msg("gkmhip_panel_delta_sat: the positions must satisfy 0 <= t_begin < t_end <= nlm + L - 1", 2);
    const int sh = panel_shift(nm);
    const int per = PN_THREADS >> sh; /* positions per workgroup */
    const int64_t blocks = (t_end - t_begin + per - 1) / per;
    if (blocks > 0x7FFFFFFF)
        return set_err_msg("gkmhip_panel_delta_sat: at most 2^31 - 1 workgroups of positions per launch", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_panel_delta_sat, dim3((unsigned)blocks), dim3(PN_THREADS), 0, stream, lm, nlm, ctx->L, t_begin, t_end,
                       P, nm, ms, sh, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_delta_sat",
                    4.0 * (panel_covered_below(t_end, nlm, ctx->L) - panel_covered_below(t_begin, nlm, ctx->L)));
    return 0;
}

extern "C" int gkmhip_panel_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases,
                                           const int32_t *var, int nvar, const uint8_t *alt, int64_t nalt, const double *P,
                                           int nm, int ms, double *out, void *stream_)
{
    if (!ctx || !codes || !var || nvar < 1 || nvar > (1 << 28) || nalt < 0 || (nalt > 0 && !alt) || !out)
        return set_err_msg("gkmhip_panel_delta_variants: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_delta_variants")) return rc;
    const int L = ctx->L;
    if (nbases < 1 || nbases > 0x7FFFFFFF - 2 * L || nalt > 0x7FFFFFFF)
        return set_err_msg("gkmhip_panel_delta_variants: needs 1 .. 2^31 - 1 - 2 L bases and fewer than 2^31 alternate bases", 2);
    if (nbases >= L && !lm) return set_err_msg("gkmhip_panel_delta_variants: needs the l-mer words of L bases or more", 2);
    double gathers = 0.0;
    for (int i = 0; i < nvar; i++) {
        const int64_t pos = var[4 * i], r = var[4 * i + 1], aoff = var[4 * i + 2], al = var[4 * i + 3];
        if (pos < 0 || r < 0 || r > GKMHIP_DELTA_MAX_ALLELE || pos + r > nbases || aoff < 0 || al < 0 ||
            al > GKMHIP_DELTA_MAX_ALLELE || aoff + al > nalt)
            return set_err_msg("gkmhip_panel_delta_variants: variant " + std::to_string(i) + " lies outside the bases or the "
                               "alternate bases given, or an allele is longer than " +
                               std::to_string(GKMHIP_DELTA_MAX_ALLELE), 2);
        const int64_t a = std::max<int64_t>(0, pos - (L - 1)), e = std::min<int64_t>(nbases, pos + r + (L - 1));
        gathers += (double)std::max<int64_t>(0, e - a - L + 1) + (double)std::max<int64_t>(0, e - a - r + al - L + 1);
    }
    const int sh = panel_shift(nm);
    const int per = PN_THREADS >> sh; /* variants per workgroup */
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    /* var and alt are the caller's host arrays: on the device before this returns (upload_rows waits) */
    if (ctx->delta_alt.ensure((size_t)nalt, true)) return 4;
    if (nalt) HIPCHK(hipMemcpyAsync(ctx->delta_alt.p, alt, (size_t)nalt, hipMemcpyHostToDevice, stream));
    if (upload_rows(ctx, (const int *)var, 4 * nvar, stream)) return 4;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_panel_delta_variants, dim3((unsigned)(((int64_t)nvar + per - 1) / per)), dim3(PN_THREADS), 0, stream,
                       lm, codes, (int)nbases, L, (const int4 *)ctx->blk_rows.p, nvar, (const uint8_t *)ctx->delta_alt.p,
                       (int)nalt, P, nm, ms, sh, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_delta_variants", gathers);
    return 0;
}
