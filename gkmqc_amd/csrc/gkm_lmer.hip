/*
 * gkm_lmer.hip -- l-mer weight tables of a trained gkm-SVM: for every kernel type but RBF the decision
 * value is linear in the query's l-mers, so the support-vector side folds once into one weight per possible l-mer,
 *
 *   W(u) = sum_i cv[i] (c[m(u, v_i)] + c[m(u, rc(v_i))])      (c[m] = 0 for m > d)
 *
 * over the canonical l-mer classes v_i of the support vectors (cv[i]: the class's dual_coef_s / sq_s w_s[q], summed on
 * the host), and a query scores as T(x) = sum_p w_x[p] W(u_p), divided by its self norm.
 *
 * Kernels
 *   k_lmer_weights  one lane per code u of [u_begin, u_end); the classes stream through the wave as scalars, eight per
 *                   request (as k_gram_direct streams its column side), each compared with u on both strands; a hit
 *                   (either strand within d) adds cv[i] * (c[mf] + c[mr]) to the lane's accumulator in ascending i
 *   k_lmer_score    one wave per query: lane l gathers W at the query's l-mers l, l + 64, ... in ascending order, then a
 *                   fixed butterfly over the 64 lanes
 *
 * Neither uses atomics or depends on the launch geometry: W[u] is a function of u, c and (v, cv) only, and a query's T of
 * the query and W only, bit for bit.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int LW_THREADS = 256;
constexpr int LW_QB = 8;       /* classes per scalar request */
constexpr int LS_THREADS = 256; /* four queries per workgroup in k_lmer_score */

__global__ __launch_bounds__(LW_THREADS) void k_lmer_weights(const uint32_t *v, const double *cv, int nv, uint32_t u_begin,
                                                              uint32_t u_end, const LmerCoef C, int L, int d, double *W)
{
    __shared__ double cs[LMER_NC];
    if (threadIdx.x < LMER_NC) cs[threadIdx.x] = C.c[threadIdx.x];
    __syncthreads();
    /* lanes past the range compare the range's last code and write nothing */
    const uint32_t u = min(u_begin + blockIdx.x * (uint32_t)LW_THREADS + threadIdx.x, u_end - 1u);
    const sgpr_words sv = (sgpr_words)v;
    const sgpr_doubles scv = (sgpr_doubles)cv;
    double acc = 0.0;
    int i = 0;
    for (; i + LW_QB <= nv; i += LW_QB) {
        uint32_t x[LW_QB];
        double w[LW_QB];
#pragma unroll
        for (int t = 0; t < LW_QB; t++) {
            x[t] = sv[i + t];
            w[t] = scv[i + t];
        }
#pragma unroll
        for (int t = 0; t < LW_QB; t++) {
            const int mf = lmer_mm(u, x[t]), mr = lmer_mm(u, lmer_rc(x[t], L));
            if (min(mf, mr) <= d) acc += w[t] * (cs[mf] + cs[mr]);
        }
    }
    /* the last nv % 8 classes one by one: the arrays are the caller's, with nothing behind their end */
    for (; i < nv; i++) {
        const uint32_t x = sv[i];
        const int mf = lmer_mm(u, x), mr = lmer_mm(u, lmer_rc(x, L));
        if (min(mf, mr) <= d) acc += scv[i] * (cs[mf] + cs[mr]);
    }
    const uint32_t me = u_begin + blockIdx.x * (uint32_t)LW_THREADS + threadIdx.x;
    if (me < u_end) W[me - u_begin] = acc;
}

__global__ __launch_bounds__(LS_THREADS) void k_lmer_score(const uint32_t *__restrict__ lmf, const int64_t *__restrict__ lmoff,
                                                           const int *__restrict__ len, int L, int col_begin, int col_end,
                                                           const double *__restrict__ W, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int j = col_begin + blockIdx.x * (LS_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= col_end) return; /* a whole wave: nothing below waits for the workgroup */
    const int n = len[j] - L + 1;
    const uint32_t *e = lmf + lmoff[j];
    double acc = 0.0;
    for (int p = lane; p < n; p += 64) {
        const uint32_t x = e[p]; /* l-mer | weight << 24 (k_pack_lmers) */
        acc += (double)(x >> LMER_WSHIFT) * W[x & LMER_CODE];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[j - col_begin] = acc;
}

} /* namespace */

extern "C" int gkmhip_lmer_weights(gkmhip_ctx *ctx, const double *c, const uint32_t *v, const double *cv, int nv,
                                   uint32_t u_begin, uint32_t u_end, double *W, void *stream_)
{
    if (!ctx || !c || nv < 0 || (nv > 0 && (!v || !cv)) || !W) return set_err_msg("gkmhip_lmer_weights: bad arguments", 2);
    const int L = ctx->L, d = ctx->d;
    const uint32_t codes = 1u << (2 * L);
    if (u_begin >= u_end || u_end > codes)
        return set_err_msg("gkmhip_lmer_weights: the code range must satisfy 0 <= u_begin < u_end <= 4^L", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const LmerCoef C = lmer_coef(c, d);
    const unsigned blocks = (unsigned)((u_end - u_begin + LW_THREADS - 1) / LW_THREADS);
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_lmer_weights, dim3(blocks), dim3(LW_THREADS), 0, stream, v, cv, nv, u_begin, u_end, C, L, d, W);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_lmer_weights", 2.0 * (double)nv * (double)(u_end - u_begin));
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: lmer weights, %d classes x codes [%u, %u) -> k_lmer_weights (%.3g comparisons)\n", nv,
                u_begin, u_end, ctx->last_comparisons);
    return 0;
}

extern "C" int gkmhip_lmer_score(gkmhip_ctx *ctx, int col_begin, int col_end, const double *W, double *out, void *stream_)
{
    if (!ctx || !W || !out) return set_err_msg("gkmhip_lmer_score: bad arguments", 2);
    if (int rc = check_range(ctx, col_begin, col_end, "gkmhip_lmer_score")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    const int per = LS_THREADS / 64;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_lmer_score, dim3((unsigned)((col_end - col_begin + per - 1) / per)), dim3(LS_THREADS), 0, stream,
                       (const uint32_t *)ctx->lmf.p, (const int64_t *)ctx->lmoff.p, (const int *)ctx->len.p, ctx->L,
                       col_begin, col_end, W, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_lmer_score", ctx->h_cum_n[(size_t)col_end] - ctx->h_cum_n[(size_t)col_begin]); /* (l-mers looked up) */
    return 0;
}
