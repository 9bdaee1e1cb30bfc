/*
 * gkm_explain.hip -- per-base importance of a trained gkm-SVM: for every query x of a column range and
 * every support vector s of a row list, the raw kernel value G(x, s) is split over the query's bases.
 *
 *   An l-mer pair (u at query position p, v = forward or reverse-complement l-mer q of s) with m <= d mismatches credits
 *   each of its L - m matched bases of u, at query position p + i, with share[m] * w_x[p] * w_s[q].  A_s(x)[t] is the sum
 *   at position t; summed over t it is G(x, s) = sum_m c_m P_m(x, s) when share[m] = c_m / (L - m).
 *
 * Kernels
 *   k_explain         one workgroup per (query, chunk of support vectors): exact uint32 tallies H[m][t] of each support
 *                     vector in LDS (ds_add_u32: order-free), folded in ascending m into a per-position double, support
 *                     vectors in list order; one partial row per chunk
 *   k_explain_reduce  the partial rows summed in chunk order, times the query's scale
 *
 * Nothing depends on arrival order, so a query's values are bit-identical whatever the block it shares and however often
 * it runs: the chunking is a function of the number of support vectors only.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_R = 8;         /* query l-mers per thread: 256 x 8 = 2 048 >= 2 046, the most a 2 047-nt query has */
constexpr int EX_OWN = 8;       /* query positions per thread in the fold: 256 x 8 = 2 048 >= 2 047 */
constexpr int EX_MAX_CHUNKS = 16;

/* support vectors per chunk: at least 64, at most EX_MAX_CHUNKS chunks (the partial rows take chunks x bases doubles) */
int explain_chunk(int nrows) { return std::max(64, (nrows + EX_MAX_CHUNKS - 1) / EX_MAX_CHUNKS); }

struct ExplainArgs {
    const int *rows;
    int nrows, chunk;
    const int *len;
    const int64_t *off, *lmoff;
    const uint32_t *lmf, *lmr; /* l-mer | weight << 24 (k_pack_lmers) */
    const double *coef;        /* [nrows] */
    double share[GKM_MAXD1];
    int L, d, col_begin;
    double *part;              /* [chunk][bases of the range] */
    int64_t part_stride;
};

/* The matched bases of a hit (mm: one bit 2j per mismatched base, j = L - 1 - i for base i of the l-mer) each get w in row
 * m of the tallies.  Base i of u sits at query position p + i. */
__device__ __forceinline__ void explain_hit(uint32_t *H, int T, int m, int p, int L, uint32_t mm, uint32_t w)
{
    uint32_t mt = ~mm & (0x00555555u >> (24 - 2 * L));
    uint32_t *h = H + m * T + p + L - 1;
    while (mt) {
        const int j = __builtin_ctz(mt) >> 1;
        atomicAdd(h - j, w);
        mt &= mt - 1u;
    }
}

__global__ __launch_bounds__(EX_THREADS) void k_explain(const ExplainArgs A)
{
    extern __shared__ uint32_t H[]; /* [d + 1][T] */
    const int tid = threadIdx.x;
    const int j = A.col_begin + blockIdx.x;
    const int c = blockIdx.y;
    const int i0 = c * A.chunk, i1 = min(A.nrows, i0 + A.chunk);
    const int L = A.L, d = A.d;
    const int T = A.len[j];
    const int nx = T - L + 1;
    const int64_t ox = A.lmoff[j];
    /* the query's l-mers: slot r of thread tid is position r * 256 + tid; lim = -1 where there is none (never a hit) */
    uint32_t u[EX_R], wu[EX_R];
    int lim[EX_R];
#pragma unroll
    for (int r = 0; r < EX_R; r++) {
        const int p = r * EX_THREADS + tid;
        const uint32_t e = p < nx ? A.lmf[ox + p] : 0u;
        u[r] = e & LMER_CODE;
        wu[r] = e >> LMER_WSHIFT;
        lim[r] = p < nx ? d : -1;
    }
    /* slots in which this wave has any l-mer (wave-uniform) */
    const int w0 = (tid >> 6) * 64;
    const int rn = __builtin_amdgcn_readfirstlane(min(EX_R, max(0, (nx - w0 + EX_THREADS - 1) / EX_THREADS)));

    double acc[EX_OWN];
#pragma unroll
    for (int k = 0; k < EX_OWN; k++) acc[k] = 0.0;
    for (int e = tid; e < (d + 1) * T; e += EX_THREADS) H[e] = 0u;
    __syncthreads();

    for (int i = i0; i < i1; i++) {
        const int s = A.rows[i];
        const int ns = A.len[s] - L + 1;
        /* the support vector's l-mers as scalars, eight of each strand per request (as k_gram_direct; the table has 8
         * entries of padding behind its end) */
        constexpr int QB = 8;
        const sgpr_words lf = (sgpr_words)(A.lmf + A.lmoff[s]), lr = (sgpr_words)(A.lmr + A.lmoff[s]);
        for (int q0 = 0; q0 < ns; q0 += QB) {
            uint32_t xf[QB], xr[QB];
#pragma unroll
            for (int t = 0; t < QB; t++) {
                xf[t] = lf[q0 + t];
                xr[t] = lr[q0 + t];
            }
#pragma unroll
            for (int t = 0; t < QB; t++) {
                if (q0 + t >= ns) break;
#pragma unroll
                for (int r = 0; r < EX_R; r++) {
                    if (r >= rn) break;
                    /* (lmer_mask drops the weight byte of the column entry) */
                    const uint32_t tf = lmer_mask(u[r], xf[t]), tr = lmer_mask(u[r], xr[t]);
                    const int mf = __builtin_popcount(tf), mr = __builtin_popcount(tr);
                    const int p = r * EX_THREADS + tid;
                    if (mf <= lim[r]) explain_hit(H, T, mf, p, L, tf, wu[r] * (xf[t] >> LMER_WSHIFT));
                    if (mr <= lim[r]) explain_hit(H, T, mr, p, L, tr, wu[r] * (xr[t] >> LMER_WSHIFT));
                }
            }
        }
        __syncthreads();
        /* fold: A_s(x)[t] = sum_m share[m] H[m][t] in ascending m, then acc[t] += coef_s A_s(x)[t]; each thread clears the
         * tallies it has read, so the next support vector starts from zero after one barrier */
        const double cs = A.coef[i];
#pragma unroll
        for (int k = 0; k < EX_OWN; k++) {
            const int t = k * EX_THREADS + tid;
            if (t < T) {
                double a = 0.0;
                for (int m = 0; m <= d; m++) {
                    a += A.share[m] * (double)H[m * T + t];
                    H[m * T + t] = 0u;
                }
                acc[k] += cs * a;
            }
        }
        __syncthreads();
    }
    double *row = A.part + (int64_t)c * A.part_stride + (A.off[j] - A.off[A.col_begin]);
#pragma unroll
    for (int k = 0; k < EX_OWN; k++) {
        const int t = k * EX_THREADS + tid;
        if (t < T) row[t] = acc[k];
    }
}

/* out[off[j] - off[col_begin] + t] = (sum over the chunks, in order, of the partial rows) * xscale[j - col_begin] */
__global__ void k_explain_reduce(const double *__restrict__ part, int64_t part_stride, int nchunks,
                                 const int *__restrict__ len, const int64_t *__restrict__ off, int col_begin,
                                 const double *__restrict__ xscale, double *__restrict__ out)
{
    const int jl = blockIdx.x, j = col_begin + jl;
    const int T = len[j];
    const int64_t b = off[j] - off[col_begin];
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        double v = part[b + t];
        for (int c = 1; c < nchunks; c++) v += part[(int64_t)c * part_stride + b + t];
        if (xscale) v *= xscale[jl];
        out[b + t] = v;
    }
}

} /* namespace */

extern "C" int gkmhip_explain_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end,
                                    const double *share, const double *coef, const double *xscale, double *out,
                                    void *stream_)
{
    if (!ctx || !rows || nrows <= 0 || !share || !coef || !out) return set_err_msg("gkmhip_explain_block: bad arguments", 2);
    if (int rc = check_range(ctx, col_begin, col_end, "gkmhip_explain_block")) return rc;
    const int L = ctx->L, d = ctx->d;
    if (d >= L) return set_err_msg("gkmhip_explain_block: needs d < L (a pair with m = L has no matched base to credit)", 2);
    double row_lmers = 0;
    if (int rc = check_rows(ctx, rows, nrows, &row_lmers)) return rc;
    int tmax = 0;
    int64_t bases = 0;
    scan_range(ctx, col_begin, col_end, &tmax, &bases);
    const double comparisons = 2.0 * row_lmers * (ctx->h_cum_n[(size_t)col_end] - ctx->h_cum_n[(size_t)col_begin]);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    const int chunk = explain_chunk(nrows), nchunks = (nrows + chunk - 1) / chunk;
    if (ctx->blk_part.ensure((size_t)nchunks * (size_t)bases, true)) return 4;
    if (int rc = upload_rows(ctx, rows, nrows, stream)) return rc;
    ExplainArgs A;
    A.rows = ctx->blk_rows.p; A.nrows = nrows; A.chunk = chunk;
    A.len = ctx->len.p; A.off = ctx->off.p; A.lmoff = ctx->lmoff.p;
    A.lmf = ctx->lmf.p; A.lmr = ctx->lmf.p + ctx->lm_stride;
    A.coef = coef;
    for (int m = 0; m < GKM_MAXD1; m++) A.share[m] = m <= d ? share[m] : 0.0;
    A.L = L; A.d = d; A.col_begin = col_begin;
    A.part = ctx->blk_part.p; A.part_stride = bases;
    const size_t lds = (size_t)(d + 1) * (size_t)tmax * sizeof(uint32_t); /* at most 13 x 2 047 x 4 = 106 444 bytes */
    HIPCHK(hipFuncSetAttribute((const void *)k_explain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_explain, dim3((unsigned)(col_end - col_begin), (unsigned)nchunks), dim3(EX_THREADS), lds, stream, A);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc; /* (k_explain alone is timed) */
    hipLaunchKernelGGL(k_explain_reduce, dim3((unsigned)(col_end - col_begin)), dim3(256), 0, stream, (const double *)ctx->blk_part.p,
                       (int64_t)bases, nchunks, (const int *)ctx->len.p, (const int64_t *)ctx->off.p, col_begin, xscale, out);
    HIPCHK(hipGetLastError());
    gkm_launch_done(ctx, "k_explain", comparisons);
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: explain %d rows x columns [%d, %d) -> k_explain (%d chunks of %d rows, %zu bytes of LDS, "
                        "%.3g comparisons)\n", nrows, col_begin, col_end, nchunks, chunk, lds, comparisons);
    return 0;
}
