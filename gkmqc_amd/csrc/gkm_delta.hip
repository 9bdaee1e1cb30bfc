/*
 * gkm_delta.hip -- variant effects from an l-mer weight table: deltaSVM, the change in the summed weights
 * of the l-mers a variant touches.  For a base string z with n = len(z) - L + 1 l-mers u_0 .. u_{n-1},
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
 * Kernels
 *   k_delta_sat       every SNV of every position: LANE = POSITION t.  The l-mers over t are the words lm[p], p in
 *                     [max(0, t-L+1), min(t, nlm-1)]; the l-mer with x_t replaced by x_t ^ j is lm[p] ^ (j << the pair of t
 *                     in it).  Four independent chains (j = 0 is the reference sum) keep four gathers in flight per
 *                     lane and step; D[t][x_t ^ j] = chain j - chain 0, +0.0 at j = 0.  Neighbouring lanes read
 *                     neighbouring words and write neighbouring 32-byte rows; only the W gathers are random.
 *   k_delta_variants  LANE = VARIANT.  The reference sum reads lm; the alternate sum rolls a 2-bit code over the left
 *                     flank, the alternate bases and the right flank and looks an l-mer up once L bases are in.  A
 *                     variant whose fields point outside the arrays (the launch checks them on the host) gets NaN and
 *                     reads nothing.
 *
 * Every value is one lane's own chain of additions in the order above: no atomics, no cross-lane sums, nothing that
 * depends on the launch geometry.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int DS_THREADS = 256;
constexpr int DV_THREADS = 256;

/* lm: the nlm l-mer words of the bases given (so nlm + L - 1 bases); positions [t0, t1) of them -> out[(t - t0) * 4 + b] */
__global__ __launch_bounds__(DS_THREADS) void k_delta_sat(const uint32_t *__restrict__ lm, int64_t nlm, int L, int64_t t0,
                                                          int64_t t1, const double *__restrict__ W,
                                                          double *__restrict__ out)
{
    const int64_t t = t0 + (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (t >= t1) return;
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
        s0 += W[u];
        s1 += W[u ^ (1u << sh)];
        s2 += W[u ^ (2u << sh)];
        s3 += W[u ^ (3u << sh)];
    }
    const uint32_t xt = (last >> (sh - 2)) & 3u; /* (sh - 2: the pair of t in l-mer p1) */
    double2 lo, hi;
    if (flags & LMER_BAD) {
        const double nan = __builtin_nan("");
        lo = make_double2(nan, nan);
        hi = lo;
    } else {
        const double d1 = s1 - s0, d2 = s2 - s0, d3 = s3 - s0;
        /* column b holds chain j = b ^ x_t */
        const double c0 = xt == 0 ? 0.0 : xt == 1 ? d1 : xt == 2 ? d2 : d3;
        const double c1 = xt == 1 ? 0.0 : xt == 0 ? d1 : xt == 3 ? d2 : d3;
        const double c2 = xt == 2 ? 0.0 : xt == 3 ? d1 : xt == 0 ? d2 : d3;
        const double c3 = xt == 3 ? 0.0 : xt == 2 ? d1 : xt == 1 ? d2 : d3;
        lo = make_double2(c0, c1);
        hi = make_double2(c2, c3);
    }
    double2 *row = (double2 *)(out + (t - t0) * 4);
    row[0] = lo;
    row[1] = hi;
}

/* var: nvar x (pos, ref_len, alt_off, alt_len); alt: nalt base codes; codes: nbases base codes; lm: their l-mer words
 * (read only where nbases >= L) */
__global__ __launch_bounds__(DV_THREADS) void k_delta_variants(const uint32_t *__restrict__ lm,
                                                               const uint8_t *__restrict__ codes, int nbases, int L,
                                                               const int4 *__restrict__ var, int nvar,
                                                               const uint8_t *__restrict__ alt, int nalt,
                                                               const double *__restrict__ W, double *__restrict__ out)
{
    const int i = blockIdx.x * DV_THREADS + threadIdx.x;
    if (i >= nvar) return;
    const int4 v = var[i];
    const int pos = v.x, r = v.y, aoff = v.z, al = v.w;
    if (pos < 0 || r < 0 || pos > nbases - r || aoff < 0 || al < 0 || aoff > nalt - al) {
        out[i] = __builtin_nan("");
        return;
    }
    const int a = max(0, pos - (L - 1)), e = min(nbases, pos + r + (L - 1));
    double ref = 0.0;
    for (int p = a; p + L <= e; p++) ref += W[lm[p] & LMER_CODE];
    const uint32_t mask = (uint32_t)((1ull << (2 * L)) - 1ull);
    uint32_t u = 0u;
    int have = 0; /* bases rolled in so far */
    double sum = 0.0;
    for (int q = a; q < pos; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += W[u];
    }
    for (int q = 0; q < al; q++) {
        u = ((u << 2) | (uint32_t)(alt[aoff + q] & 3)) & mask;
        if (++have >= L) sum += W[u];
    }
    for (int q = pos + r; q < e; q++) {
        u = ((u << 2) | (uint32_t)(codes[q] & 3)) & mask;
        if (++have >= L) sum += W[u];
    }
    out[i] = sum - ref;
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

} /* namespace */

extern "C" int gkmhip_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end,
                                const double *W, double *out, void *stream_)
{
    if (!ctx || !lm || !W || !out) return set_err_msg("gkmhip_delta_sat: bad arguments", 2);
    if (nlm < 1 || t_begin < 0 || t_begin >= t_end || t_end > nlm + ctx->L - 1)
        return set_err_msg("gkmhip_delta_sat: the positions must satisfy 0 <= t_begin < t_end <= nlm + L - 1", 2);
    const int64_t blocks = (t_end - t_begin + DS_THREADS - 1) / DS_THREADS;
    if (blocks > 0x7FFFFFFF) return set_err_msg("gkmhip_delta_sat: at most 2^31 - 1 workgroups of positions per launch", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_delta_sat, dim3((unsigned)blocks), dim3(DS_THREADS), 0, stream, lm, nlm, ctx->L, t_begin, t_end, W,
                       out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_delta_sat", 4.0 * (covered_below(t_end, nlm, ctx->L) - covered_below(t_begin, nlm, ctx->L)));
    return 0;
}

extern "C" int gkmhip_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases,
                                     const int32_t *var, int nvar, const uint8_t *alt, int64_t nalt, const double *W,
                                     double *out, void *stream_)
{
    if (!ctx || !codes || !var || nvar < 1 || nvar > (1 << 28) || nalt < 0 || (nalt > 0 && !alt) || !W || !out)
        return set_err_msg("gkmhip_delta_variants: bad arguments", 2);
    const int L = ctx->L;
    if (nbases < 1 || nbases > 0x7FFFFFFF - 2 * L || nalt > 0x7FFFFFFF)
        return set_err_msg("gkmhip_delta_variants: needs 1 .. 2^31 - 1 - 2 L bases and fewer than 2^31 alternate bases", 2);
    if (nbases >= L && !lm) return set_err_msg("gkmhip_delta_variants: needs the l-mer words of L bases or more", 2);
    double gathers = 0.0;
    for (int i = 0; i < nvar; i++) {
        const int64_t pos = var[4 * i], r = var[4 * i + 1], aoff = var[4 * i + 2], al = var[4 * i + 3];
        if (pos < 0 || r < 0 || r > GKMHIP_DELTA_MAX_ALLELE || pos + r > nbases || aoff < 0 || al < 0 ||
            al > GKMHIP_DELTA_MAX_ALLELE || aoff + al > nalt)
            return set_err_msg("gkmhip_delta_variants: variant " + std::to_string(i) + " lies outside the bases or the "
                               "alternate bases given, or an allele is longer than " +
                               std::to_string(GKMHIP_DELTA_MAX_ALLELE), 2);
        const int64_t a = std::max<int64_t>(0, pos - (L - 1)), e = std::min<int64_t>(nbases, pos + r + (L - 1));
        gathers += (double)std::max<int64_t>(0, e - a - L + 1) + (double)std::max<int64_t>(0, e - a - r + al - L + 1);
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    /* var and alt are the caller's host arrays: on the device before this returns (upload_rows waits) */
    if (ctx->delta_alt.ensure((size_t)nalt, true)) return 4;
    if (nalt) HIPCHK(hipMemcpyAsync(ctx->delta_alt.p, alt, (size_t)nalt, hipMemcpyHostToDevice, stream));
    if (upload_rows(ctx, (const int *)var, 4 * nvar, stream)) return 4;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_delta_variants, dim3((unsigned)((nvar + DV_THREADS - 1) / DV_THREADS)), dim3(DV_THREADS), 0, stream,
                       lm, codes, (int)nbases, L, (const int4 *)ctx->blk_rows.p, nvar, (const uint8_t *)ctx->delta_alt.p,
                       (int)nalt, W, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_delta_variants", gathers);
    return 0;
}
