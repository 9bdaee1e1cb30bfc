/*
 * gkm_limp.hip -- per-base importance tables of a trained gkm-SVM: the explanation is as linear in the
 * query's l-mers as the score is, and which bases of a hit pair matched depends on the two l-mers only, so the
 * support-vector side folds once into one value per (l-mer, offset),
 *
 *   V(u, i) = sum_j cv[j] (share[m(u, v_j)] [u[i] == v_j[i]] + share[m(u, rc v_j)] [u[i] == rc(v_j)[i]])
 *
 * over the canonical l-mer classes (v_j, cv_j) of gkm_lmer.hip (share[m] = c[m] / (L - m), 0 for m > d; offset i counts
 * from the l-mer's first base, which sits in the highest pair), and a query's explanation and hypothetical table are
 * gathers: E(x)[t] = sum_i w_x[t - i] V(u_{t-i}, i) / sq_x.
 *
 * Kernels
 *   k_lmer_importance  one lane per code u of [u_begin, u_end); the classes stream through the wave as scalars, eight per
 *                      request, each compared with u on both strands exactly as k_lmer_weights compares them; a hit
 *                      adds cv[j] * (tf_i + tr_i) to L per-offset accumulators in registers, in ascending j
 *   k_lmer_explain     one thread per base t of a query: the L covering l-mers of the context's forward l-mer table, in
 *                      ascending offset
 *   k_lmer_hyp         one thread per (t, b): the same sum with base t of every covering l-mer set to b
 *
 * None uses atomics or scratch, or depends on the launch geometry: V[u][i] is a function of u, share and (v, cv) only,
 * V[rc(u)][L-1-i] is bit for bit V[u][i] (the two strands swap roles; their terms meet in one commutative add before
 * the multiply), and a query's values are functions of the query and V only.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int LI_THREADS = 256;
constexpr int LI_QB = 8;  /* classes per scalar request */
constexpr int LI_MAXL = 12;
constexpr int LG_THREADS = 256;

/* One class against one code.  The miss path is k_lmer_weights': XOR, fold, popcount on both strands and one compare.
 * On a hit the strands' terms are added first and multiplied once (no contraction: the add must stay commutative, so
 * that rc(u) forms the same product from the swapped strands). */
template <int L>
__device__ __forceinline__ void limp_class(uint32_t u, uint32_t x, double w, int d, const double *sh, double (&acc)[L])
{
#pragma clang fp contract(off)
    const uint32_t kf = lmer_mask(u, x), kr = lmer_mask(u, lmer_rc(x, L));
    const int mf = __builtin_popcount(kf), mr = __builtin_popcount(kr);
    if (min(mf, mr) <= d) {
        const double sf = sh[mf], sr = sh[mr];
#pragma unroll
        for (int i = 0; i < L; i++) {
            const uint32_t bit = 1u << (2 * (L - 1 - i));
            const double tf = (kf & bit) ? 0.0 : sf;
            const double tr = (kr & bit) ? 0.0 : sr;
            const double both = tf + tr;
            acc[i] += w * both;
        }
    }
}

template <int L>
__global__ __launch_bounds__(LI_THREADS) void k_lmer_importance(const uint32_t *v, const double *cv, int nv, uint32_t u_begin,
                                                                 uint32_t u_end, const LmerCoef S, int d, double *V)
{
    __shared__ double sh[LMER_NC];
    if (threadIdx.x < LMER_NC) sh[threadIdx.x] = S.c[threadIdx.x];
    __syncthreads();
    /* lanes past the range compare the range's last code and write nothing */
    const uint32_t me = u_begin + blockIdx.x * (uint32_t)LI_THREADS + threadIdx.x;
    const uint32_t u = min(me, u_end - 1u);
    const sgpr_words sv = (sgpr_words)v;
    const sgpr_doubles scv = (sgpr_doubles)cv;
    double acc[L];
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = 0.0;
    int j = 0;
    for (; j + LI_QB <= nv; j += LI_QB) {
        uint32_t x[LI_QB];
        double w[LI_QB];
#pragma unroll
        for (int t = 0; t < LI_QB; t++) {
            x[t] = sv[j + t];
            w[t] = scv[j + t];
        }
#pragma unroll
        for (int t = 0; t < LI_QB; t++) limp_class<L>(u, x[t], w[t], d, sh, acc);
    }
    /* the last nv % 8 classes one by one: the arrays are the caller's, with nothing behind their end */
    for (; j < nv; j++) limp_class<L>(u, sv[j], scv[j], d, sh, acc);
    if (me < u_end) {
        double *row = V + (size_t)(me - u_begin) * L;
#pragma unroll
        for (int i = 0; i < L; i++) row[i] = acc[i];
    }
}

/* sum_i w[t - i] V[u_{t-i} (base i set to b if b >= 0)][i] over the l-mers of e[0, n) that cover base t, ascending i */
__device__ __forceinline__ double limp_gather(const uint32_t *__restrict__ e, int n, int L, int t, int b,
                                              const double *__restrict__ V)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < L; i++) {
        const int p = t - i;
        if (p < 0 || p >= n) continue;
        const uint32_t x = e[p]; /* l-mer | weight << 24 (k_pack_lmers) */
        uint32_t u = x & LMER_CODE;
        if (b >= 0) {
            const int sft = 2 * (L - 1 - i);
            u = (u & ~(3u << sft)) | ((uint32_t)b << sft);
        }
        const double term = (double)(x >> LMER_WSHIFT) * V[(size_t)u * L + i];
        acc += term;
    }
    return acc;
}

/* grid: x = the query of the range, y = tiles of LG_THREADS bases */
__global__ __launch_bounds__(LG_THREADS) void k_lmer_explain(const uint32_t *__restrict__ lmf, const int64_t *__restrict__ lmoff,
                                                             const int64_t *__restrict__ off, const int *__restrict__ len,
                                                             int L, int col_begin, const double *__restrict__ V,
                                                             const double *__restrict__ xscale, double *__restrict__ E)
{
    const int j = col_begin + blockIdx.x;
    const int T = len[j], t = blockIdx.y * LG_THREADS + threadIdx.x;
    if (t >= T) return;
    const double sum = limp_gather(lmf + lmoff[j], T - L + 1, L, t, -1, V);
    E[off[j] - off[col_begin] + t] = sum * xscale[blockIdx.x];
}

/* grid: x = the query of the range, y = tiles of LG_THREADS (t, b) cells */
__global__ __launch_bounds__(LG_THREADS) void k_lmer_hyp(const uint32_t *__restrict__ lmf, const int64_t *__restrict__ lmoff,
                                                         const int64_t *__restrict__ off, const int *__restrict__ len, int L,
                                                         int col_begin, const double *__restrict__ V, double *__restrict__ R)
{
    const int j = col_begin + blockIdx.x;
    const int T = len[j], cell = blockIdx.y * LG_THREADS + threadIdx.x;
    if (cell >= 4 * T) return;
    R[4 * (off[j] - off[col_begin]) + cell] = limp_gather(lmf + lmoff[j], T - L + 1, L, cell >> 2, cell & 3, V);
}

template <int L>
void limp_launch(unsigned blocks, hipStream_t stream, const uint32_t *v, const double *cv, int nv, uint32_t u_begin,
                 uint32_t u_end, const LmerCoef &S, int d, double *V)
{
    hipLaunchKernelGGL(k_lmer_importance<L>, dim3(blocks), dim3(LI_THREADS), 0, stream, v, cv, nv, u_begin, u_end, S, d, V);
}

/* the prologue the two gather launches share: range check, the l-mer table, the longest query of the range */
int limp_gather_prologue(gkmhip_ctx *ctx, int col_begin, int col_end, const char *what, hipStream_t stream, int *tmax)
{
    if (int rc = check_range(ctx, col_begin, col_end, what)) return rc;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    int64_t bases = 0;
    scan_range(ctx, col_begin, col_end, tmax, &bases);
    return 0;
}

} /* namespace */

extern "C" int gkmhip_lmer_importance(gkmhip_ctx *ctx, const double *share, const uint32_t *v, const double *cv, int nv,
                                      uint32_t u_begin, uint32_t u_end, double *V, void *stream_)
{
    if (!ctx || !share || nv < 0 || (nv > 0 && (!v || !cv)) || !V)
        return set_err_msg("gkmhip_lmer_importance: bad arguments", 2);
    const int L = ctx->L, d = ctx->d;
    if (L < 1 || L > LI_MAXL) return set_err_msg("gkmhip_lmer_importance: L must lie in 1..12", 2);
    const uint32_t codes = 1u << (2 * L);
    if (u_begin >= u_end || u_end > codes)
        return set_err_msg("gkmhip_lmer_importance: the code range must satisfy 0 <= u_begin < u_end <= 4^L", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const LmerCoef S = lmer_coef(share, d);
    const unsigned blocks = (unsigned)((u_end - u_begin + LI_THREADS - 1) / LI_THREADS);
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    switch (L) {
#define LIMP_CASE(N) \
    case N: limp_launch<N>(blocks, stream, v, cv, nv, u_begin, u_end, S, d, V); break;
        LIMP_CASE(1) LIMP_CASE(2) LIMP_CASE(3) LIMP_CASE(4) LIMP_CASE(5) LIMP_CASE(6)
        LIMP_CASE(7) LIMP_CASE(8) LIMP_CASE(9) LIMP_CASE(10) LIMP_CASE(11) LIMP_CASE(12)
#undef LIMP_CASE
    }
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_lmer_importance", 2.0 * (double)nv * (double)(u_end - u_begin));
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: lmer importance, %d classes x codes [%u, %u) -> k_lmer_importance (%.3g comparisons)\n", nv,
                u_begin, u_end, ctx->last_comparisons);
    return 0;
}

extern "C" int gkmhip_lmer_explain(gkmhip_ctx *ctx, int col_begin, int col_end, const double *V, const double *xscale,
                                   double *E, void *stream_)
{
    if (!ctx || !V || !xscale || !E) return set_err_msg("gkmhip_lmer_explain: bad arguments", 2);
    hipStream_t stream = (hipStream_t)stream_;
    int tmax = 0;
    if (int rc = limp_gather_prologue(ctx, col_begin, col_end, "gkmhip_lmer_explain", stream, &tmax)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_lmer_explain, dim3((unsigned)(col_end - col_begin), (unsigned)((tmax + LG_THREADS - 1) / LG_THREADS)),
                       dim3(LG_THREADS), 0, stream, (const uint32_t *)ctx->lmf.p, (const int64_t *)ctx->lmoff.p,
                       (const int64_t *)ctx->off.p, (const int *)ctx->len.p, ctx->L, col_begin, V, xscale, E);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    /* (gathers: every l-mer is looked up once per base it covers) */
    gkm_launch_done(ctx, "k_lmer_explain", (double)ctx->L * (ctx->h_cum_n[(size_t)col_end] - ctx->h_cum_n[(size_t)col_begin]));
    return 0;
}

extern "C" int gkmhip_lmer_hyp(gkmhip_ctx *ctx, int col_begin, int col_end, const double *V, double *R, void *stream_)
{
    if (!ctx || !V || !R) return set_err_msg("gkmhip_lmer_hyp: bad arguments", 2);
    hipStream_t stream = (hipStream_t)stream_;
    int tmax = 0;
    if (int rc = limp_gather_prologue(ctx, col_begin, col_end, "gkmhip_lmer_hyp", stream, &tmax)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_lmer_hyp, dim3((unsigned)(col_end - col_begin), (unsigned)((4 * tmax + LG_THREADS - 1) / LG_THREADS)),
                       dim3(LG_THREADS), 0, stream, (const uint32_t *)ctx->lmf.p, (const int64_t *)ctx->lmoff.p,
                       (const int64_t *)ctx->off.p, (const int *)ctx->len.p, ctx->L, col_begin, V, R);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_lmer_hyp", 4.0 * (double)ctx->L * (ctx->h_cum_n[(size_t)col_end] - ctx->h_cum_n[(size_t)col_begin]));
    return 0;
}
