/*
 * gkm_delta.hip -- variant effects from an l-mer weight table or panel: deltaSVM, the change in the
 * summed weights of the l-mers a variant touches.  For a base string z with n = len(z) - L + 1 l-mers u_0 .. u_{n-1},
 *
 *   S(z) = ((0.0 + W[u_0]) + W[u_1]) + ... + W[u_{n-1}]          plain double additions, p ascending; 0.0 when n < 1
 *
 * and a variant (pos, r reference bases, the alternate bases alt) of a sequence x of T bases, with a = max(0, pos - (L-1))
 * and e = min(T, pos + r + (L-1)):
 *
 *   delta = S(x[a:pos] + alt + x[pos+r:e]) - S(x[a:e])
 *
 * No positional weights enter: a variant has no window.  Like the scan kernels these take the context for L only, and
 * plain device pointers; the long sequence never goes through gkmhip_set_sequences.
 *
 * The two computations exist once, as device functions over a weight accessor w(u): a table's W[u] (TableWeights) or one
 * model's column of a panel, P[u * ms + m] (PanelColumn, gkm_panel.hip's layout).  A panel value is therefore the table
 * value of that column bit for bit: the same chain of additions (-ffp-contract=off).
 *   delta_sat_chains  every SNV of one position t.  The l-mers over t are the words lm[p], p in [max(0, t-L+1),
 *                     min(t, nlm-1)]; the l-mer with x_t replaced by x_t ^ j is lm[p] ^ (j << the pair of t in it).  Four
 *                     independent chains (j = 0 is the reference sum) keep four gathers in flight per lane and step;
 *                     D[t][x_t ^ j] = chain j - chain 0, +0.0 at j = 0; NaN where a word of the context is flagged.
 *   delta_variant     one variant.  The reference sum reads lm; the alternate sum rolls a 2-bit code over the left flank,
 *                     the alternate bases and the right flank and looks an l-mer up once L bases are in.  A variant
 *                     whose fields point outside the arrays (the launch checks them on the host) gets NaN and reads
 *                     nothing.
 *
 * Kernels: each works out its item (and model), calls the body and stores
 *   k_delta_sat             LANE = POSITION t.  Neighbouring lanes read neighbouring words and write neighbouring 32-byte
 *                           rows; only the W gathers are random.
 *   k_delta_variants        LANE = VARIANT
 *   k_panel_delta_sat       lane = (position, model), 64 / mp positions per wave (mp: nm rounded up to 8, 16, 32 or 64)
 *   k_panel_delta_variants  lane = (variant, model), 64 / mp variants per wave
 * Panel lanes m >= nm read inside the row (clamped to its last column) and never store.
 *
 * Every value is one lane's own chain of additions in the order above: no atomics, no cross-lane sums, nothing that
 * depends on the launch geometry.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int DELTA_THREADS = 256;

/* the weight of l-mer u: of a table, or of one model of a panel whose rows are `row` doubles apart */
struct TableWeights {
    const double *__restrict__ W;
    __device__ __forceinline__ double operator()(uint32_t u) const { return W[u]; }
};
struct PanelColumn {
    const double *__restrict__ col;
    size_t row;
    __device__ __forceinline__ double operator()(uint32_t u) const { return col[(size_t)u * row]; }
};

/* the model of this thread's column: the clamped column for the lanes m >= nm */
__device__ __forceinline__ PanelColumn panel_column(const double *__restrict__ P, int ms, int m)
{
    return PanelColumn{P + min(m, ms - 1), (size_t)ms};
}

/* lm: the nlm l-mer words of the bases given (so nlm + L - 1 bases) -> the row of position t: columns A, C, G, T */
template <typename Weights>
__device__ __forceinline__ void delta_sat_chains(const uint32_t *__restrict__ lm, int64_t nlm, int L, int64_t t, Weights w,
                                                 double &c0, double &c1, double &c2, double &c3)
{
    const int64_t p0 = max((int64_t)0, t - L + 1), p1 = min(t, nlm - 1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t flags = 0u, last = 0u;
    int sh = 2 * (L - 1 - (int)(t - p0)); /* the pair of base t in l-mer p0; two more per step */
#pragma unroll 2
    for (int64_t p = p0; p <= p1; p++, sh += 2) {
        const uint32_t e = lm[p];
        const uint32_t u = e & LMER_CODE;
        flags |= e;
        last = u;
        s0 += w(u);
        s1 += w(u ^ (1u << sh));
        s2 += w(u ^ (2u << sh));
        s3 += w(u ^ (3u << sh));
    }
    const uint32_t xt = (last >> (sh - 2)) & 3u; /* (sh - 2: the pair of t in l-mer p1) */
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
}

/* positions [t0, t1) -> out[(t - t0) * 4 + b] */
__global__ __launch_bounds__(DELTA_THREADS) void k_delta_sat(const uint32_t *__restrict__ lm, int64_t nlm, int L, int64_t t0,
                                                             int64_t t1, const double *__restrict__ W,
                                                             double *__restrict__ out)
{
    const int64_t t = t0 + (int64_t)blockIdx.x * DELTA_THREADS + threadIdx.x;
    if (t >= t1) return;
    double c0, c1, c2, c3;
    delta_sat_chains(lm, nlm, L, t, TableWeights{W}, c0, c1, c2, c3);
    double2 *row = (double2 *)(out + (t - t0) * 4);
    row[0] = make_double2(c0, c1);
    row[1] = make_double2(c2, c3);
}

/* sh: log2(mp).  Thread (i << sh) + m is (position t0 + i, model m) -> out[((t - t0) * 4 + b) * nm + m] */
__global__ __launch_bounds__(DELTA_THREADS) void k_panel_delta_sat(const uint32_t *__restrict__ lm, int64_t nlm, int L,
                                                                   int64_t t0, int64_t t1, const double *__restrict__ P,
                                                                   int nm, int ms, int sh, double *__restrict__ out)
{
    const int64_t tid = (int64_t)blockIdx.x * DELTA_THREADS + threadIdx.x;
    const int64_t t = t0 + (tid >> sh);
    const int m = (int)(tid & ((1 << sh) - 1));
    if (t >= t1) return;
    double c0, c1, c2, c3;
    delta_sat_chains(lm, nlm, L, t, panel_column(P, ms, m), c0, c1, c2, c3);
    if (m >= nm) return;
    double *dst = out + (size_t)(t - t0) * 4u * (size_t)nm + (size_t)m;
    dst[0] = c0;
    dst[(size_t)nm] = c1;
    dst[2 * (size_t)nm] = c2;
    dst[3 * (size_t)nm] = c3;
}

/* v: (pos, ref_len, alt_off, alt_len); alt: nalt base codes; codes: nbases base codes; lm: their l-mer words (read only
 * where nbases >= L) */
template <typename Weights>
__device__ __forceinline__ double delta_variant(const uint32_t *__restrict__ lm, const uint8_t *__restrict__ codes,
                                                int nbases, int L, const int4 v, const uint8_t *__restrict__ alt, int nalt,
                                                Weights w)
{
    const int pos = v.x, r = v.y, aoff = v.z, al = v.w;
    if (pos < 0 || r < 0 || pos > nbases - r || aoff < 0 || al < 0 || aoff > nalt - al) return __builtin_nan("");
    const int a = max(0, pos - (L - 1)), e = min(nbases, pos + r + (L - 1));
    double ref = 0.0;
    for (int p = a; p + L <= e; p++) ref += w(lm[p] & LMER_CODE);
    const uint32_t mask = (uint32_t)((1ull << (2 * L)) - 1ull);
    uint32_t u = 0u;
    int have = 0; /* bases rolled in so far */
    double sum = 0.0;
    for (int q = a; q < pos; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += w(u);
    }
    for (int q = 0; q < al; q++) {
        u = ((u << 2) | (uint32_t)(alt[aoff + q] & 3)) & mask;
        if (++have >= L) sum += w(u);
    }
    for (int q = pos + r; q < e; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += w(u);
    }
    return sum - ref;
}

/* var: nvar variants -> out[i] */
__global__ __launch_bounds__(DELTA_THREADS) void k_delta_variants(const uint32_t *__restrict__ lm,
                                                                  const uint8_t *__restrict__ codes, int nbases, int L,
                                                                  const int4 *__restrict__ var, int nvar,
                                                                  const uint8_t *__restrict__ alt, int nalt,
                                                                  const double *__restrict__ W, double *__restrict__ out)
{
    const int i = blockIdx.x * DELTA_THREADS + threadIdx.x;
    if (i >= nvar) return;
    out[i] = delta_variant(lm, codes, nbases, L, var[i], alt, nalt, TableWeights{W});
}

/* sh: log2(mp).  Thread (i << sh) + m is (variant i, model m) -> out[i * nm + m] */
__global__ __launch_bounds__(DELTA_THREADS) void k_panel_delta_variants(const uint32_t *__restrict__ lm,
                                                                        const uint8_t *__restrict__ codes, int nbases, int L,
                                                                        const int4 *__restrict__ var, int nvar,
                                                                        const uint8_t *__restrict__ alt, int nalt,
                                                                        const double *__restrict__ P, int nm, int ms, int sh,
                                                                        double *__restrict__ out)
{
    const int64_t tid = (int64_t)blockIdx.x * DELTA_THREADS + threadIdx.x;
    const int64_t i = tid >> sh;
    const int m = (int)(tid & ((1 << sh) - 1));
    if (i >= nvar) return;
    const double delta = delta_variant(lm, codes, nbases, L, var[i], alt, nalt, panel_column(P, ms, m));
    if (m < nm) out[(size_t)i * (size_t)nm + (size_t)m] = delta;
}

/* sum over positions s < t of the l-mers (of nlm) that cover s */
double covered_below(int64_t t, int64_t nlm, int L)
{
    /* l-mer p covers clamp(t - p, 0, L) positions below t */
    const int64_t whole = std::min(nlm, std::max<int64_t>(0, t - L + 1));
    double g = (double)whole * L;
    for (int64_t p = whole; p < std::min(nlm, t); p++) g += (double)(t - p);
    return g;
}

/* the positions of a saturation launch with `per` of them per workgroup: 0 with *blocks and *gathers, or error 2 */
int sat_check(const gkmhip_ctx *ctx, int64_t nlm, int64_t t_begin, int64_t t_end, int per, const char *what, int64_t *blocks,
              double *gathers)
{
    if (nlm < 1 || t_begin < 0 || t_begin >= t_end || t_end > nlm + ctx->L - 1)
        return set_err_msg(std::string(what) + ": the positions must satisfy 0 <= t_begin < t_end <= nlm + L - 1", 2);
    *blocks = (t_end - t_begin + per - 1) / per;
    if (*blocks > 0x7FFFFFFF)
        return set_err_msg(std::string(what) + ": at most 2^31 - 1 workgroups of positions per launch", 2);
    *gathers = 4.0 * (covered_below(t_end, nlm, ctx->L) - covered_below(t_begin, nlm, ctx->L));
    return 0;
}

/* the bases and the host's variant rows of a variant launch: 0 with the gathers of one model in *gathers, or error 2 */
int variants_check(const gkmhip_ctx *ctx, const void *lm, int64_t nbases, const int32_t *var, int nvar, int64_t nalt,
                   const char *what, double *gathers)
{
    const int L = ctx->L;
    if (nbases < 1 || nbases > 0x7FFFFFFF - 2 * L || nalt > 0x7FFFFFFF)
        return set_err_msg(std::string(what) + ": needs 1 .. 2^31 - 1 - 2 L bases and fewer than 2^31 alternate bases", 2);
    if (nbases >= L && !lm) return set_err_msg(std::string(what) + ": needs the l-mer words of L bases or more", 2);
    *gathers = 0.0;
    for (int i = 0; i < nvar; i++) {
        const int64_t pos = var[4 * i], r = var[4 * i + 1], aoff = var[4 * i + 2], al = var[4 * i + 3];
        if (pos < 0 || r < 0 || r > GKMHIP_DELTA_MAX_ALLELE || pos + r > nbases || aoff < 0 || al < 0 ||
            al > GKMHIP_DELTA_MAX_ALLELE || aoff + al > nalt)
            return set_err_msg(std::string(what) + ": variant " + std::to_string(i) + " lies outside the bases or the "
                               "alternate bases given, or an allele is longer than " +
                               std::to_string(GKMHIP_DELTA_MAX_ALLELE), 2);
        const int64_t a = std::max<int64_t>(0, pos - (L - 1)), e = std::min<int64_t>(nbases, pos + r + (L - 1));
        *gathers += (double)std::max<int64_t>(0, e - a - L + 1) + (double)std::max<int64_t>(0, e - a - r + al - L + 1);
    }
    return 0;
}

/* var and alt are the caller's host arrays: in ctx->blk_rows and ctx->delta_alt before this returns (upload_rows waits) */
int variants_stage(gkmhip_ctx *ctx, const int32_t *var, int nvar, const uint8_t *alt, int64_t nalt, hipStream_t stream)
{
    if (ctx->delta_alt.ensure((size_t)nalt, true)) return 4;
    if (nalt) HIPCHK(hipMemcpyAsync(ctx->delta_alt.p, alt, (size_t)nalt, hipMemcpyHostToDevice, stream));
    if (upload_rows(ctx, (const int *)var, 4 * nvar, stream)) return 4;
    return 0;
}

} /* namespace */

extern "C" int gkmhip_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end,
                                const double *W, double *out, void *stream_)
{
    if (!ctx || !lm || !W || !out) return set_err_msg("gkmhip_delta_sat: bad arguments", 2);
    int64_t blocks;
    double gathers;
    if (int rc = sat_check(ctx, nlm, t_begin, t_end, DELTA_THREADS, "gkmhip_delta_sat", &blocks, &gathers)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_delta_sat, dim3((unsigned)blocks), dim3(DELTA_THREADS), 0, stream, lm, nlm, ctx->L, t_begin, t_end,
                       W, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_delta_sat", gathers);
    return 0;
}

extern "C" int gkmhip_panel_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end,
                                      const double *P, int nm, int ms, double *out, void *stream_)
{
    if (!ctx || !lm || !out) return set_err_msg("gkmhip_panel_delta_sat: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_delta_sat")) return rc;
    const int sh = panel_shift(nm);
    int64_t blocks;
    double gathers; /* (rows looked up) */
    if (int rc = sat_check(ctx, nlm, t_begin, t_end, DELTA_THREADS >> sh, "gkmhip_panel_delta_sat", &blocks, &gathers))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_panel_delta_sat, dim3((unsigned)blocks), dim3(DELTA_THREADS), 0, stream, lm, nlm, ctx->L, t_begin,
                       t_end, P, nm, ms, sh, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_delta_sat", gathers);
    return 0;
}

extern "C" int gkmhip_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases,
                                     const int32_t *var, int nvar, const uint8_t *alt, int64_t nalt, const double *W,
                                     double *out, void *stream_)
{
    if (!ctx || !codes || !var || nvar < 1 || nvar > (1 << 28) || nalt < 0 || (nalt > 0 && !alt) || !W || !out)
        return set_err_msg("gkmhip_delta_variants: bad arguments", 2);
    double gathers;
    if (int rc = variants_check(ctx, lm, nbases, var, nvar, nalt, "gkmhip_delta_variants", &gathers)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = variants_stage(ctx, var, nvar, alt, nalt, stream)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_delta_variants, dim3((unsigned)((nvar + DELTA_THREADS - 1) / DELTA_THREADS)), dim3(DELTA_THREADS), 0,
                       stream, lm, codes, (int)nbases, ctx->L, (const int4 *)ctx->blk_rows.p, nvar,
                       (const uint8_t *)ctx->delta_alt.p, (int)nalt, W, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_delta_variants", gathers);
    return 0;
}

extern "C" int gkmhip_panel_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases,
                                           const int32_t *var, int nvar, const uint8_t *alt, int64_t nalt, const double *P,
                                           int nm, int ms, double *out, void *stream_)
{
    if (!ctx || !codes || !var || nvar < 1 || nvar > (1 << 28) || nalt < 0 || (nalt > 0 && !alt) || !out)
        return set_err_msg("gkmhip_panel_delta_variants: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_delta_variants")) return rc;
    double gathers; /* (rows looked up) */
    if (int rc = variants_check(ctx, lm, nbases, var, nvar, nalt, "gkmhip_panel_delta_variants", &gathers)) return rc;
    const int sh = panel_shift(nm);
    const int per = DELTA_THREADS >> sh; /* variants per workgroup */
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = variants_stage(ctx, var, nvar, alt, nalt, stream)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_panel_delta_variants, dim3((unsigned)(((int64_t)nvar + per - 1) / per)), dim3(DELTA_THREADS), 0,
                       stream, lm, codes, (int)nbases, ctx->L, (const int4 *)ctx->blk_rows.p, nvar,
                       (const uint8_t *)ctx->delta_alt.p, (int)nalt, P, nm, ms, sh, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_delta_variants", gathers);
    return 0;
}
