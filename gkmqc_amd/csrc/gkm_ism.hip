/*
 * gkm_ism.hip -- in-silico mutagenesis of a trained gkm-SVM: for every query x of a column range, every
 * position t and every base b, the change of the raw kernel values sum_s coef_s G(y, s) when y = x with base t set to b,
 * and the mismatch profiles P_m(y, y) of every such mutant against itself.  The change dG_s(t, b) of ONE support vector is
 * complete, as exact integer tallies in LDS, before it is folded; what a model does with it is the fold's business: a
 * linear model multiplies by a coefficient and adds, an RBF model normalises, exponentiates and adds.
 *
 *   A substitution at t changes only the query l-mers that cover it.  Take every pair (query l-mer u at p, forward or
 *   reverse-complement l-mer v of s) with m <= min(d + 1, L) mismatches and weight w = w_x[p] w_s[q]:
 *     U[m][p + i]       += w  for each MATCHED base i (m <= d): every other base there moves the pair to m + 1;
 *     B[m][p + i][v[i]] += w  for each MISMATCHED base i: only b = v[i] moves the pair to m - 1.
 *   Then dP_m(t, b) = U[m-1][t] - U[m][t] + B[m+1][t][b] - B[m][t][b], and with fold_u[m] = c_{m+1} - c_m and
 *   fold_b[m] = c_{m-1} - c_m (c_{d+1} = 0), dG_s(t, b) = sum_m fold_u[m] U[m][t] + sum_m fold_b[m] B[m][t][b].
 *
 * Hypothetical importance is a second fold of the same tallies: a pair MISMATCHED at t against the
 * support vector's base b is, in y = x with base t set to b, a pair with one mismatch fewer that is MATCHED at t, so
 * explain's tally of y is H_y[m][t] = B[m + 1][t][b], and the raw hypothetical score of (t, b) is
 * sum_s coef_s sum_{m=1..d+1} share[m-1] B[m][t][b] (b != x[t]) or sum_s coef_s sum_{m=0..d} share[m] U[m][t] (b = x[t]).
 *
 * Kernels
 *   k_ism            one workgroup per (query, chunk of support vectors, tile of query positions): exact uint32 tallies
 *                    U and B of each support vector in LDS (ds_add_u32: order-free) and an exact uint64 profile of the
 *                    tile's own l-mers, folded in ascending m into per-(t, b) doubles and a per-tile G, support vectors in
 *                    list order; one partial row per chunk
 *   k_ism_reduce     the partial rows summed in chunk order into the (T, 4) output (0.0 at the query's own base), and
 *                    base(x) = sum_s coef_s G(x, s) summed over tiles and chunks in order
 *   k_ism<ISM_HYP>   (k_ism is k_ism<ISM_LIN>; reported as k_ism<true>) the same enumeration, tallies, chunking and
 *                    tiling with the hypothetical fold: 4 doubles per base, no profile
 *   k_ism_hyp_reduce k_ism<ISM_HYP>'s partial rows summed in chunk order into the (T, 4) output, the query's own base
 *                    included
 *   k_ism<ISM_RBF>   (reported as k_ism_rbf) the same enumeration, tallies, chunking and tiling with the RBF fold of
 *                    no profile; the raw G(x, s) arrives from a Gram launch, and each support vector adds
 *                    dual_s exp(gamma (G(y, s) / (sq_s sqrt(G(y, y))) - 1)) per mutant instead of coef_s dG_s; its partial
 *                    rows and per-tile base go through k_ism_reduce
 *   k_ism_self_base  P_m(x, x), exact uint64 (alone: gkmhip_self_profiles, the exact norms of the interpretation paths)
 *   k_ism_self       P_m(y, y) of the three mutants at one position: P_m(x, x) plus the exact change of every pair in
 *                    which a changed l-mer takes part (about 4 L T comparisons per mutant)
 *
 * Nothing depends on arrival order, so a query's values are bit-identical whatever the block it shares and however often
 * it runs: the chunking is a function of the number of support vectors only, the tiling of (L, d) only.
 */
#include "gkm_lmer_dev.h"

namespace {

/* what k_ism does with a support vector's tallies: the linear fold of in-silico mutagenesis, the hypothetical fold, or the
 * RBF fold */
enum { ISM_LIN = 0, ISM_HYP = 1, ISM_RBF = 2 };

constexpr int ISM_THREADS = 256;
constexpr int ISM_R = 8;        /* query l-mers per thread: 256 x 8 = 2 048 >= the l-mers of any tile */
constexpr int ISM_OWN = 8;      /* tile positions per thread in the fold: 256 x 8 = 2 048 >= the longest tile */
constexpr int ISM_MAX_CHUNKS = 16;
constexpr size_t ISM_LDS = 160 * 1024; /* gfx950's LDS: the most one workgroup may take */
constexpr int ISM_QCAP = 128;   /* hits queued per wave: flushed at 64, and one push adds at most 64 */
constexpr int ISM_QWORDS = 3;   /* words per queued hit */
/* LDS besides the tallies: the profile counters, then each wave's hit queue */
constexpr size_t ISM_LDS_FIXED = GKM_MAXD1 * sizeof(unsigned long long) +
                                 (size_t)(ISM_THREADS / 64) * ISM_QCAP * ISM_QWORDS * sizeof(uint32_t);

/* support vectors per chunk: at least 64, at most ISM_MAX_CHUNKS chunks (the partial rows take chunks x 3 x bases doubles) */
int ism_chunk(int nrows) { return std::max(64, (nrows + ISM_MAX_CHUNKS - 1) / ISM_MAX_CHUNKS); }

/* B rows hold the pairs with m = 1 .. mb mismatches */
int ism_mb(int L, int d) { return std::min(d + 1, L); }

/* query positions per tile: the U and B rows of a tile and the profile counters within the LDS.  A function of (L, d)
 * only, so a query is cut the same way whatever the launch; one tile holds any query (2 047 bases) up to d = 3 */
int ism_tile(int L, int d)
{
    const size_t per = (size_t)(d + 1 + 3 * ism_mb(L, d)) * sizeof(uint32_t);
    return (int)std::min<size_t>(ISM_R * ISM_THREADS, (ISM_LDS - ISM_LDS_FIXED) / per);
}

struct IsmArgs {
    const int *rows;
    int nrows, chunk;
    const int *len;
    const int64_t *off, *lmoff;
    const uint32_t *lmf, *lmr; /* l-mer | weight << 24 (k_pack_lmers) */
    const double *coef;        /* [nrows] */
    double fu[GKM_MAXD1];      /* U row m, m = 0..d */
    double fb[GKM_MAXD1];      /* B row m at index m - 1, m = 1..mb */
    double gc[GKM_MAXD1];      /* profile m, m = 0..d */
    int L, d, mb, col_begin;
    int tile, stride, ntiles;  /* positions per tile, LDS row length (min(tile, longest query)), tiles of the launch */
    double *part;              /* [chunk][3 x bases of the range] (hypothetical mode: 4 x bases) */
    int64_t part_stride;
    double *gpart;             /* [chunk][query][tile] */
    /* the RBF fold only (there coef holds the dual coefficients, not divided by the norms) */
    const double *sq;          /* [n]: sqrt(G(i, i)) per uploaded sequence */
    const double *gx;          /* [nrows][ldg]: raw G(x_j, rows[i]) at column j - col_begin */
    int64_t ldg;
    const double *ysq;         /* 4 per base of the range: sqrt(G(y, y)) */
    const uint8_t *codes;
    double gamma;
};

/* A pair (query l-mer at tile position pt, i.e. query position t0 + pt; support-vector l-mer v) with m <= mb mismatches
 * (mm: one bit 2j per mismatched base, j = L - 1 - i for base i of the l-mer).  Base i sits at tile position pt + i.
 * Only the linear mode keeps a profile. */
template <int MODE>
__device__ __forceinline__ void ism_hit(uint32_t *U, uint32_t *B, unsigned long long *P, int stride, int tlen, int d,
                                        int L, int m, int pt, uint32_t mm, uint32_t u, uint32_t v, uint32_t w)
{
    if constexpr (MODE == ISM_LIN) {
        if (m <= d && pt >= 0) atomicAdd(P + m, (unsigned long long)w); /* (the l-mers of the tile's own positions only) */
    }
    const int top = pt + L - 1;
    for (int j = 0; j < L; j++) {
        const int tl = top - j;
        if ((unsigned)tl >= (unsigned)tlen) continue;
        if ((mm >> (2 * j)) & 1u) {
            /* v's base is one of the three that are not u's: slot (v[i] - u[i] - 1) mod 4 */
            const uint32_t slot = ((v >> (2 * j)) - (u >> (2 * j)) - 1u) & 3u;
            atomicAdd(B + ((m - 1) * 3 + (int)slot) * stride + tl, w);
        } else if (m <= d) {
            atomicAdd(U + m * stride + tl, w);
        }
    }
}

/* Hits are rare (about 2 % of the pairs at L = 10, d = 3 on iid bases) but most wave-wide comparison steps have one, so a
 * walk over the L bases inside the comparison loop would run with one or two lanes active.  Instead each wave appends
 * its hits (u | m << 24, v, pt + 16 | w << 16) to a queue of its own in LDS and walks 64 of them at a time, one per lane.
 * Called with the whole wave active; qn is wave-uniform. */
__device__ __forceinline__ int ism_push(uint32_t *Q, int qn, bool hit, uint32_t a, uint32_t b, uint32_t c)
{
    const unsigned long long bal = __ballot(hit);
    if (bal == 0ull) return qn;
    if (hit) {
        const int k = qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        Q[ISM_QWORDS * k] = a;
        Q[ISM_QWORDS * k + 1] = b;
        Q[ISM_QWORDS * k + 2] = c;
    }
    return qn + __popcll(bal);
}

template <int MODE>
__device__ __forceinline__ void ism_flush(const uint32_t *Q, int qn, int lane, uint32_t *U, uint32_t *B,
                                          unsigned long long *P, int stride, int tlen, int d, int L)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int k = lane; k < qn; k += 64) {
        const uint32_t a = Q[ISM_QWORDS * k], v = Q[ISM_QWORDS * k + 1], c = Q[ISM_QWORDS * k + 2];
        const uint32_t u = a & LMER_CODE;
        /* (the mask is symmetric; with v first the compiler keeps the operand order it has always given the fold) */
        ism_hit<MODE>(U, B, P, stride, tlen, d, L, (int)(a >> 24), (int)(c & 0xFFFFu) - 16, lmer_mask(v, u), u, v, c >> 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

/* ISM_LIN: in-silico mutagenesis; ISM_HYP: the hypothetical mode, part rows [slot 0, slot 1, slot 2, own] per base
 * (slot s: the mutant to base (x[t] + 1 + s) mod 4); ISM_RBF: every mutant's RBF decision sum, part rows as ISM_LIN's.
 * They differ in the fold and what they write only */
template <int MODE>
__global__ __launch_bounds__(ISM_THREADS) void k_ism(const IsmArgs A)
{
    extern __shared__ unsigned long long lds[];
    constexpr bool HYP = MODE == ISM_HYP;
    constexpr int W = HYP ? 4 : 3; /* doubles per base of a partial row */
    unsigned long long *P = lds;                     /* [d + 1] */
    uint32_t *U = (uint32_t *)(lds + GKM_MAXD1);     /* [d + 1][stride] */
    uint32_t *B = U + (A.d + 1) * A.stride;          /* [mb][3][stride] */
    uint32_t *Q = B + 3 * A.mb * A.stride + (threadIdx.x >> 6) * (ISM_QCAP * ISM_QWORDS); /* this wave's hit queue */
    const int lane = threadIdx.x & 63;
    const int tid = threadIdx.x;
    const int jl = blockIdx.x, j = A.col_begin + jl;
    const int c = blockIdx.y, z = blockIdx.z;
    const int i0 = c * A.chunk, i1 = min(A.nrows, i0 + A.chunk);
    const int L = A.L, d = A.d, mb = A.mb, stride = A.stride;
    const int T = A.len[j];
    const int t0 = z * A.tile;
    if (t0 >= T) return; /* (workgroup-uniform: no tile of this query) */
    const int tlen = min(A.tile, T - t0);
    const int nx = T - L + 1;
    /* the l-mers that cover a position of the tile: [pl0, pl1) */
    const int pl0 = max(0, t0 - L + 1), pl1 = min(nx, t0 + tlen);
    const int64_t ox = A.lmoff[j];
    uint32_t u[ISM_R], wu[ISM_R];
    int lim[ISM_R];
#pragma unroll
    for (int r = 0; r < ISM_R; r++) {
        const int p = pl0 + r * ISM_THREADS + tid;
        const uint32_t e = p < pl1 ? A.lmf[ox + p] : 0u;
        u[r] = e & LMER_CODE;
        wu[r] = e >> LMER_WSHIFT;
        lim[r] = p < pl1 ? mb : -1;
    }
    const int w0 = (tid >> 6) * 64;
    const int rn = __builtin_amdgcn_readfirstlane(min(ISM_R, max(0, (pl1 - pl0 - w0 + ISM_THREADS - 1) / ISM_THREADS)));

    double acc[ISM_OWN][W];
#pragma unroll
    for (int k = 0; k < ISM_OWN; k++) {
        acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        if constexpr (HYP) acc[k][3] = 0.0;
    }
    double gacc = 0.0;
    /* RBF: the norms of this thread's 3 x ISM_OWN mutants, slot s being base (x[t] + 1 + s) mod 4, stay in registers */
    double yn[MODE == ISM_RBF ? ISM_OWN : 1][3];
    if constexpr (MODE == ISM_RBF) {
        const uint8_t *x = A.codes + A.off[j] + t0;
        const double *yq = A.ysq + 4 * (A.off[j] - A.off[A.col_begin] + t0);
#pragma unroll
        for (int k = 0; k < ISM_OWN; k++) {
            const int tl = k * ISM_THREADS + tid;
            const int xb = tl < tlen ? x[tl] & 3 : 0;
#pragma unroll
            for (int s = 0; s < 3; s++) yn[k][s] = tl < tlen ? yq[4 * tl + ((xb + 1 + s) & 3)] : 1.0;
        }
    }
    for (int e = tid; e < (d + 1 + 3 * mb) * stride; e += ISM_THREADS) U[e] = 0u;
    if (tid <= d) P[tid] = 0ull;
    __syncthreads();

    for (int i = i0; i < i1; i++) {
        const int s = A.rows[i];
        const int ns = A.len[s] - L + 1;
        constexpr int QB = 8;
        const sgpr_words lf = (sgpr_words)(A.lmf + A.lmoff[s]), lr = (sgpr_words)(A.lmr + A.lmoff[s]);
        int qn = 0;
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
                for (int r = 0; r < ISM_R; r++) {
                    if (r >= rn) break;
                    const int mf = lmer_mm(u[r], xf[t]), mr = lmer_mm(u[r], xr[t]);
                    const uint32_t ptw = (uint32_t)(pl0 + r * ISM_THREADS + tid - t0 + 16);
                    qn = ism_push(Q, qn, mf <= lim[r], u[r] | ((uint32_t)mf << 24), xf[t] & LMER_CODE,
                                  ptw | (wu[r] * (xf[t] >> LMER_WSHIFT)) << 16);
                    if (qn >= 64) {
                        ism_flush<MODE>(Q, qn, lane, U, B, P, stride, tlen, d, L);
                        qn = 0;
                    }
                    qn = ism_push(Q, qn, mr <= lim[r], u[r] | ((uint32_t)mr << 24), xr[t] & LMER_CODE,
                                  ptw | (wu[r] * (xr[t] >> LMER_WSHIFT)) << 16);
                    if (qn >= 64) {
                        ism_flush<MODE>(Q, qn, lane, U, B, P, stride, tlen, d, L);
                        qn = 0;
                    }
                }
            }
        }
        if (qn) ism_flush<MODE>(Q, qn, lane, U, B, P, stride, tlen, d, L);
        __syncthreads();
        /* fold in ascending m: a(t, b) = sum_m fu[m] U[m][t] + fb[m] B[m][t][b], then acc += coef_s a; each thread clears
         * what it has read, so the next support vector starts from zero after one barrier.  Hypothetical mode (fu[m] =
         * share[m], fb[m - 1] = share[m - 1]): the own column takes the U rows only, each mutant column its B rows only,
         * in k_explain's expression shape.  RBF mode: a is dG_s(t, b) as the linear mode forms it, and acc += dual_s
         * exp(gamma ((G(x, s) + a) / (sq_s sqrt(G(y, y))) - 1)), k_normalize_full's expression shape */
        const double cs = A.coef[i];
        double sqs = 0.0, gxs = 0.0;
        if constexpr (MODE == ISM_RBF) {
            sqs = A.sq[s];
            gxs = A.gx[(int64_t)i * A.ldg + jl];
        }
#pragma unroll
        for (int k = 0; k < ISM_OWN; k++) {
            const int tl = k * ISM_THREADS + tid;
            if constexpr (HYP) {
                if (tl < tlen) {
                    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                    for (int m = 0; m <= d || m <= mb; m++) {
                        if (m <= d) {
                            a3 += A.fu[m] * (double)U[m * stride + tl];
                            U[m * stride + tl] = 0u;
                        }
                        if (m >= 1 && m <= mb) {
                            uint32_t *b = B + (m - 1) * 3 * stride + tl;
                            a0 += A.fb[m - 1] * (double)b[0];
                            a1 += A.fb[m - 1] * (double)b[stride];
                            a2 += A.fb[m - 1] * (double)b[2 * stride];
                            b[0] = b[stride] = b[2 * stride] = 0u;
                        }
                    }
                    acc[k][0] += cs * a0;
                    acc[k][1] += cs * a1;
                    acc[k][2] += cs * a2;
                    acc[k][3] += cs * a3;
                }
            } else if (tl < tlen) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                for (int m = 0; m <= d || m <= mb; m++) {
                    if (m <= d) {
                        const double x = A.fu[m] * (double)U[m * stride + tl];
                        U[m * stride + tl] = 0u;
                        a0 += x;
                        a1 += x;
                        a2 += x;
                    }
                    if (m >= 1 && m <= mb) {
                        uint32_t *b = B + (m - 1) * 3 * stride + tl;
                        a0 += A.fb[m - 1] * (double)b[0];
                        a1 += A.fb[m - 1] * (double)b[stride];
                        a2 += A.fb[m - 1] * (double)b[2 * stride];
                        b[0] = b[stride] = b[2 * stride] = 0u;
                    }
                }
                if constexpr (MODE == ISM_RBF) {
                    acc[k][0] += cs * exp(A.gamma * ((gxs + a0) / (sqs * yn[k][0]) - 1));
                    acc[k][1] += cs * exp(A.gamma * ((gxs + a1) / (sqs * yn[k][1]) - 1));
                    acc[k][2] += cs * exp(A.gamma * ((gxs + a2) / (sqs * yn[k][2]) - 1));
                } else {
                    acc[k][0] += cs * a0;
                    acc[k][1] += cs * a1;
                    acc[k][2] += cs * a2;
                }
            }
        }
        if constexpr (MODE == ISM_RBF) {
            /* score(x)'s sum, once per query: the first tile keeps it, the others add 0.0 in k_ism_reduce */
            if (tid == 0 && z == 0) gacc += cs * exp(A.gamma * (gxs / (sqs * A.sq[j]) - 1));
        }
        if constexpr (MODE == ISM_LIN) {
            if (tid == 0) {
                double g = 0.0;
                for (int m = 0; m <= d; m++) {
                    g += A.gc[m] * (double)P[m];
                    P[m] = 0ull;
                }
                gacc += cs * g;
            }
        }
        __syncthreads();
    }
    double *row = A.part + (int64_t)c * A.part_stride + W * (A.off[j] - A.off[A.col_begin] + t0);
#pragma unroll
    for (int k = 0; k < ISM_OWN; k++) {
        const int tl = k * ISM_THREADS + tid;
        if (tl < tlen) {
            row[W * tl] = acc[k][0];
            row[W * tl + 1] = acc[k][1];
            row[W * tl + 2] = acc[k][2];
            if constexpr (HYP) row[W * tl + 3] = acc[k][3];
        }
    }
    if constexpr (!HYP) {
        if (tid == 0) A.gpart[((int64_t)c * gridDim.x + jl) * A.ntiles + z] = gacc;
    }
}

/* out[4 (off[j] - off[col_begin] + t) + b] = the partial rows of (t, b) summed in chunk order, 0.0 at b = x[t];
 * base[j - col_begin] = the tiles' G summed in tile order, each over the chunks in order */
__global__ void k_ism_reduce(const double *__restrict__ part, int64_t part_stride, const double *__restrict__ gpart,
                             int nchunks, int ntiles, int tile, const int *__restrict__ len, const int64_t *__restrict__ off,
                             const uint8_t *__restrict__ codes, int col_begin, double *__restrict__ out,
                             double *__restrict__ base)
{
    const int jl = blockIdx.x, j = col_begin + jl;
    const int T = len[j];
    const int64_t b0 = off[j] - off[col_begin];
    const uint8_t *x = codes + off[j];
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const int xb = x[t] & 3;
        double *o = out + 4 * (b0 + t);
        o[xb] = 0.0;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const int64_t e = 3 * (b0 + t) + s;
            double v = part[e];
            for (int c = 1; c < nchunks; c++) v += part[(int64_t)c * part_stride + e];
            o[(xb + 1 + s) & 3] = v;
        }
    }
    if (base && threadIdx.x == 0) {
        const int nt = (T + tile - 1) / tile;
        double v = 0.0;
        for (int z = 0; z < nt; z++)
            for (int c = 0; c < nchunks; c++) v += gpart[((int64_t)c * gridDim.x + jl) * ntiles + z];
        base[jl] = v;
    }
}

/* out[4 (off[j] - off[col_begin] + t) + b] = k_ism<true>'s partial rows of (t, b) summed in chunk order, the query's own
 * base included */
__global__ void k_ism_hyp_reduce(const double *__restrict__ part, int64_t part_stride, int nchunks,
                                 const int *__restrict__ len, const int64_t *__restrict__ off,
                                 const uint8_t *__restrict__ codes, int col_begin, double *__restrict__ out)
{
    const int jl = blockIdx.x, j = col_begin + jl;
    const int T = len[j];
    const int64_t b0 = off[j] - off[col_begin];
    const uint8_t *x = codes + off[j];
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const int xb = x[t] & 3;
        double *o = out + 4 * (b0 + t);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int64_t e = 4 * (b0 + t) + s;
            double v = part[e];
            for (int c = 1; c < nchunks; c++) v += part[(int64_t)c * part_stride + e];
            o[(xb + 1 + s) & 3] = v; /* (s = 3: the own base) */
        }
    }
}

/* P_m(x, x) of each query of the range: pself[jl][m], m = 0..d */
__global__ __launch_bounds__(ISM_THREADS) void k_ism_self_base(const int *__restrict__ len, const int64_t *__restrict__ lmoff,
                                                              const uint32_t *__restrict__ lmf, const uint32_t *__restrict__ lmr,
                                                              int L, int d, int col_begin, int64_t *__restrict__ pself)
{
    __shared__ unsigned long long Pm[GKM_MAXD1];
    const int jl = blockIdx.x, j = col_begin + jl, tid = threadIdx.x;
    const int nx = len[j] - L + 1;
    const int64_t ox = lmoff[j];
    if (tid <= d) Pm[tid] = 0ull;
    __syncthreads();
    for (int p = tid; p < nx; p += ISM_THREADS) {
        const uint32_t ue = lmf[ox + p];
        const uint32_t uu = ue & LMER_CODE, wu = ue >> LMER_WSHIFT;
        for (int q = 0; q < 2 * nx; q++) {
            const uint32_t ve = q < nx ? lmf[ox + q] : lmr[ox + q - nx];
            const int m = lmer_mm(uu, ve & LMER_CODE);
            if (m <= d) atomicAdd(Pm + m, (unsigned long long)(wu * (ve >> LMER_WSHIFT)));
        }
    }
    __syncthreads();
    if (tid <= d) pself[(int64_t)jl * (d + 1) + tid] = (int64_t)Pm[tid];
}

/* One pair of the self profile: u / v are the l-mers of x; su / sv the shift of the substituted base in each (-1: the
 * l-mer does not cover t).  The pair leaves its count m_x and joins m_y for each of the three mutants. */
__device__ __forceinline__ void self_pair(unsigned long long *D, int d, const uint32_t dl[3], uint32_t u, int su,
                                          uint32_t v, int sv, uint32_t w)
{
    const int mx = lmer_mm(u, v);
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const uint32_t uy = su >= 0 ? u ^ (dl[s] << su) : u;
        const uint32_t vy = sv >= 0 ? v ^ (dl[s] << sv) : v;
        const int my = lmer_mm(uy, vy);
        if (my == mx) continue;
        if (mx <= d) atomicAdd(D + s * (d + 1) + mx, (unsigned long long)(-(long long)w));
        if (my <= d) atomicAdd(D + s * (d + 1) + my, (unsigned long long)w);
    }
}

/* prof[((off[j] - off[col_begin] + t) * 4 + b) * (d + 1) + m] = P_m(y, y), y = x with base t set to b (b = x[t]: x
 * itself); one workgroup per (query, position) */
__global__ __launch_bounds__(ISM_THREADS) void k_ism_self(const int *__restrict__ len, const int64_t *__restrict__ off,
                                                         const int64_t *__restrict__ lmoff, const uint32_t *__restrict__ lmf,
                                                         const uint32_t *__restrict__ lmr, const uint8_t *__restrict__ codes,
                                                         int L, int d, int col_begin, const int64_t *__restrict__ pself,
                                                         int64_t *__restrict__ prof)
{
    __shared__ unsigned long long D[3 * GKM_MAXD1]; /* [mutant][m]: the change, two's complement */
    const int jl = blockIdx.x, j = col_begin + jl, t = blockIdx.y, tid = threadIdx.x;
    const int T = len[j];
    if (t >= T) return; /* (workgroup-uniform) */
    const int nx = T - L + 1;
    const int64_t ox = lmoff[j];
    const int xb = codes[off[j] + t] & 3;
    /* the forward l-mers that cover t: [a0, a1]; the reverse-complement l-mer r is the forward l-mer nx - 1 - r */
    const int a0 = max(0, t - L + 1), a1 = min(t, nx - 1), na = a1 - a0 + 1;
    uint32_t dl[3]; /* x[t] ^ b: in a forward l-mer at base t - p, in a reverse one (complemented: the same xor) mirrored */
#pragma unroll
    for (int s = 0; s < 3; s++) dl[s] = (uint32_t)(xb ^ ((xb + 1 + s) & 3));
    for (int e = tid; e < 3 * (d + 1); e += ISM_THREADS) D[e] = 0ull;
    __syncthreads();
    /* every pair with a changed query-side l-mer */
    for (int p = a0; p <= a1; p++) {
        const uint32_t ue = lmf[ox + p];
        const int su = 2 * (L - 1 - (t - p));
        for (int q = tid; q < 2 * nx; q += ISM_THREADS) {
            const bool rc = q >= nx;
            const uint32_t ve = rc ? lmr[ox + q - nx] : lmf[ox + q];
            const int pv = rc ? 2 * nx - 1 - q : q;
            const int sv = pv < a0 || pv > a1 ? -1 : rc ? 2 * (t - pv) : 2 * (L - 1 - (t - pv));
            self_pair(D, d, dl, ue & LMER_CODE, su, ve & LMER_CODE, sv, (ue >> LMER_WSHIFT) * (ve >> LMER_WSHIFT));
        }
    }
    /* every pair of an unchanged query-side l-mer with a changed one on the other side */
    for (int ci = 0; ci < 2 * na; ci++) {
        const bool rc = ci >= na;
        const int pv = a0 + (rc ? ci - na : ci);
        const uint32_t ve = rc ? lmr[ox + nx - 1 - pv] : lmf[ox + pv];
        const int sv = rc ? 2 * (t - pv) : 2 * (L - 1 - (t - pv));
        for (int p = tid; p < nx; p += ISM_THREADS) {
            if (p >= a0 && p <= a1) continue;
            const uint32_t ue = lmf[ox + p];
            self_pair(D, d, dl, ue & LMER_CODE, -1, ve & LMER_CODE, sv, (ue >> LMER_WSHIFT) * (ve >> LMER_WSHIFT));
        }
    }
    __syncthreads();
    int64_t *o = prof + (off[j] - off[col_begin] + t) * 4 * (d + 1);
    for (int e = tid; e < 4 * (d + 1); e += ISM_THREADS) {
        const int b = e / (d + 1), m = e - b * (d + 1);
        int64_t v = pself[(int64_t)jl * (d + 1) + m];
        if (b != xb) v += (int64_t)D[((b - xb - 1) & 3) * (d + 1) + m];
        o[e] = v;
    }
}

/* gkmhip_ism_block (ISM_LIN), gkmhip_hyp_block (ISM_HYP) and gkmhip_ism_rbf_block (ISM_RBF) behind their argument checks,
 * fold coefficients (A.fu, A.fb, A.gc) and, for ISM_RBF, A.sq, A.gx, A.ldg and A.ysq: k_ism<MODE> over (rows) x [col_begin,
 * col_end), then its reduce kernel.  4 (hypothetical) or 3 partial doubles per base; the other two keep a per-tile value
 * per query and return base. */
template <int MODE>
int ism_launch(gkmhip_ctx *ctx, IsmArgs &A, const int *rows, int nrows, int col_begin, int col_end, const double *coef,
               double *out, double *base, hipStream_t stream)
{
    constexpr bool HYP = MODE == ISM_HYP;
    constexpr int per = HYP ? 4 : 3;
    constexpr const char *entry[] = {"gkmhip_ism_block", "gkmhip_hyp_block", "gkmhip_ism_rbf_block"};
    constexpr const char *kernel[] = {"k_ism", "k_ism<true>", "k_ism_rbf"};
    constexpr const char *what[] = {"ism", "hypothetical", "ism (RBF fold)"};
    if (int rc = check_range(ctx, col_begin, col_end, entry[MODE])) return rc;
    if (MODE == ISM_RBF && A.ldg < col_end - col_begin)
        return set_err_msg("gkmhip_ism_rbf_block: leading dimension too small", 2);
    const int L = ctx->L, d = ctx->d, mb = ism_mb(L, d);
    if (HYP && d >= L)
        return set_err_msg("gkmhip_hyp_block: needs d < L (a pair with m = L has no matched base to credit)", 2);
    const int tile = ism_tile(L, d);
    double row_lmers = 0;
    if (int rc = check_rows(ctx, rows, nrows, &row_lmers)) return rc;
    int tmax = 0;
    int64_t bases = 0;
    scan_range(ctx, col_begin, col_end, &tmax, &bases);
    double tile_lmers = 0; /* query l-mers loaded over all tiles (a tile also takes the L - 1 l-mers before it) */
    for (int j = col_begin; j < col_end; j++) {
        const int T = ctx->h_len[(size_t)j], nx = T - L + 1;
        for (int t0 = 0; t0 < T; t0 += tile) tile_lmers += std::min(nx, t0 + tile) - std::max(0, t0 - L + 1);
    }
    const double comparisons = 2.0 * row_lmers * tile_lmers;
    const int ntiles = (tmax + tile - 1) / tile, stride = std::min(tile, tmax);
    const int ncols = col_end - col_begin;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    const int chunk = ism_chunk(nrows), nchunks = (nrows + chunk - 1) / chunk;
    if (ctx->blk_part.ensure((size_t)nchunks * per * (size_t)bases, true) ||
        (!HYP && ctx->ism_gpart.ensure((size_t)nchunks * (size_t)ncols * (size_t)ntiles, true)))
        return 4;
    if (int rc = upload_rows(ctx, rows, nrows, stream)) return rc;
    A.rows = ctx->blk_rows.p; A.nrows = nrows; A.chunk = chunk;
    A.len = ctx->len.p; A.off = ctx->off.p; A.lmoff = ctx->lmoff.p;
    A.lmf = ctx->lmf.p; A.lmr = ctx->lmf.p + ctx->lm_stride;
    A.coef = coef;
    A.L = L; A.d = d; A.mb = mb; A.col_begin = col_begin;
    A.tile = tile; A.stride = stride; A.ntiles = ntiles;
    A.part = ctx->blk_part.p; A.part_stride = per * bases; A.gpart = HYP ? nullptr : ctx->ism_gpart.p;
    A.codes = ctx->codes.p; A.gamma = ctx->gamma;
    /* at most 6 248 + 4 x (13 + 3 x 12) x 804 = 163 832 bytes (L = 12, d = 12); 44 648 at gkmQC's shape */
    const size_t lds = ISM_LDS_FIXED + (size_t)(d + 1 + 3 * mb) * (size_t)stride * sizeof(uint32_t);
    HIPCHK(hipFuncSetAttribute((const void *)k_ism<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_ism<MODE>, dim3((unsigned)ncols, (unsigned)nchunks, (unsigned)ntiles), dim3(ISM_THREADS), lds,
                       stream, A);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc; /* (k_ism<MODE> alone is timed) */
    if constexpr (HYP)
        hipLaunchKernelGGL(k_ism_hyp_reduce, dim3((unsigned)ncols), dim3(256), 0, stream, (const double *)ctx->blk_part.p,
                           (int64_t)per * bases, nchunks, (const int *)ctx->len.p, (const int64_t *)ctx->off.p,
                           (const uint8_t *)ctx->codes.p, col_begin, out);
    else
        hipLaunchKernelGGL(k_ism_reduce, dim3((unsigned)ncols), dim3(256), 0, stream, (const double *)ctx->blk_part.p,
                           (int64_t)per * bases, (const double *)ctx->ism_gpart.p, nchunks, ntiles, tile,
                           (const int *)ctx->len.p, (const int64_t *)ctx->off.p, (const uint8_t *)ctx->codes.p, col_begin,
                           out, base);
    HIPCHK(hipGetLastError());
    gkm_launch_done(ctx, kernel[MODE], comparisons);
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: %s %d rows x columns [%d, %d) -> %s (%d chunks of %d rows, %d tiles of %d positions, "
                        "%zu bytes of LDS, %.3g comparisons)\n", what[MODE], nrows, col_begin, col_end,
                ctx->last_kernel, nchunks, chunk, ntiles, tile, lds, comparisons);
    return 0;
}

} /* namespace */

extern "C" int gkmhip_ism_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end,
                                const double *fold_u, const double *fold_b, const double *gcoef, const double *coef,
                                double *out, double *base, void *stream_)
{
    if (!ctx || !rows || nrows <= 0 || !fold_u || !fold_b || !gcoef || !coef || !out)
        return set_err_msg("gkmhip_ism_block: bad arguments", 2);
    IsmArgs A = {};
    for (int m = 0; m < GKM_MAXD1; m++) {
        A.fu[m] = m <= ctx->d ? fold_u[m] : 0.0;
        A.fb[m] = m < ism_mb(ctx->L, ctx->d) ? fold_b[m] : 0.0;
        A.gc[m] = m <= ctx->d ? gcoef[m] : 0.0;
    }
    return ism_launch<ISM_LIN>(ctx, A, rows, nrows, col_begin, col_end, coef, out, base, (hipStream_t)stream_);
}

extern "C" int gkmhip_hyp_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end,
                                const double *share, const double *coef, double *out, void *stream_)
{
    if (!ctx || !rows || nrows <= 0 || !share || !coef || !out) return set_err_msg("gkmhip_hyp_block: bad arguments", 2);
    IsmArgs A = {};
    for (int m = 0; m < GKM_MAXD1; m++) {
        A.fu[m] = m <= ctx->d ? share[m] : 0.0;                    /* U row m: share[m] */
        A.fb[m] = m < ism_mb(ctx->L, ctx->d) ? share[m] : 0.0;     /* B row m + 1: share[m] */
        A.gc[m] = 0.0;
    }
    return ism_launch<ISM_HYP>(ctx, A, rows, nrows, col_begin, col_end, coef, out, nullptr, (hipStream_t)stream_);
}

extern "C" int gkmhip_ism_rbf_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end,
                                    const double *fold_u, const double *fold_b, const double *dual, const double *sq,
                                    const double *gx, int64_t ld, const double *ysq, double *out, double *base,
                                    void *stream_)
{
    if (!ctx || !rows || nrows <= 0 || !fold_u || !fold_b || !dual || !sq || !gx || !ysq || !out)
        return set_err_msg("gkmhip_ism_rbf_block: bad arguments", 2);
    if (!ctx->rbf)
        return set_err_msg("gkmhip_ism_rbf_block: the context's kernel type is not 3 or 5 (linear types: gkmhip_ism_block)", 2);
    IsmArgs A = {};
    for (int m = 0; m < GKM_MAXD1; m++) {
        A.fu[m] = m <= ctx->d ? fold_u[m] : 0.0;
        A.fb[m] = m < ism_mb(ctx->L, ctx->d) ? fold_b[m] : 0.0;
        A.gc[m] = 0.0;
    }
    A.sq = sq; A.gx = gx; A.ldg = ld; A.ysq = ysq;
    return ism_launch<ISM_RBF>(ctx, A, rows, nrows, col_begin, col_end, dual, out, base, (hipStream_t)stream_);
}

extern "C" int gkmhip_ism_self_profiles(gkmhip_ctx *ctx, int col_begin, int col_end, int64_t *prof, void *stream_)
{
    if (!ctx || !prof) return set_err_msg("gkmhip_ism_self_profiles: bad arguments", 2);
    if (int rc = check_range(ctx, col_begin, col_end, "gkmhip_ism_self_profiles")) return rc;
    const int L = ctx->L, d = ctx->d, ncols = col_end - col_begin;
    int tmax = 0;
    double comparisons = 0;
    for (int j = col_begin; j < col_end; j++) {
        const int T = ctx->h_len[(size_t)j], nx = T - L + 1;
        tmax = std::max(tmax, T);
        comparisons += 2.0 * nx * nx; /* P_m(x, x) */
        for (int t = 0; t < T; t++) {
            const int na = std::min(t, nx - 1) - std::max(0, t - L + 1) + 1;
            comparisons += 4.0 * (2.0 * na * nx + 2.0 * na * (nx - na)); /* x and the three mutants */
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    if (ctx->ism_pself.ensure((size_t)ncols * (size_t)(d + 1), true)) return 4;
    const uint32_t *lmr = ctx->lmf.p + ctx->lm_stride;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_ism_self_base, dim3((unsigned)ncols), dim3(ISM_THREADS), 0, stream, (const int *)ctx->len.p,
                       (const int64_t *)ctx->lmoff.p, (const uint32_t *)ctx->lmf.p, lmr, L, d, col_begin, ctx->ism_pself.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ism_self, dim3((unsigned)ncols, (unsigned)tmax), dim3(ISM_THREADS), 0, stream,
                       (const int *)ctx->len.p, (const int64_t *)ctx->off.p, (const int64_t *)ctx->lmoff.p,
                       (const uint32_t *)ctx->lmf.p, lmr, (const uint8_t *)ctx->codes.p, L, d, col_begin,
                       (const int64_t *)ctx->ism_pself.p, prof);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_ism_self", comparisons);
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: ism self profiles of columns [%d, %d) -> k_ism_self_base + k_ism_self (%d x %d workgroups, "
                        "%.3g comparisons)\n", col_begin, col_end, ncols, tmax, comparisons);
    return 0;
}

extern "C" int gkmhip_self_profiles(gkmhip_ctx *ctx, int col_begin, int col_end, int64_t *pself, void *stream_)
{
    if (!ctx || !pself) return set_err_msg("gkmhip_self_profiles: bad arguments", 2);
    if (int rc = check_range(ctx, col_begin, col_end, "gkmhip_self_profiles")) return rc;
    double comparisons = 0;
    for (int j = col_begin; j < col_end; j++) {
        const double nx = ctx->h_len[(size_t)j] - ctx->L + 1;
        comparisons += 2.0 * nx * nx;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (ensure_lmers(ctx, stream, true)) return 4;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_ism_self_base, dim3((unsigned)(col_end - col_begin)), dim3(ISM_THREADS), 0, stream,
                       (const int *)ctx->len.p, (const int64_t *)ctx->lmoff.p, (const uint32_t *)ctx->lmf.p,
                       (const uint32_t *)(ctx->lmf.p + ctx->lm_stride), ctx->L, ctx->d, col_begin, pself);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_ism_self_base", comparisons);
    return 0;
}
