/*
 * gkm_hip.h -- device-layer C ABI of the gkm kernel-matrix path (MI355X / gfx950).
 *
 * Plain pointers and sizes only; no torch / C++ types.  `gkm_main_pywrapper`
 * (include/gkmkern_pylib.h) is a thin C host on top of these calls; bench.py and
 * the GPU tests bind them with ctypes and pass device pointers and a HIP stream
 * obtained from PyTorch-ROCm.
 *
 * What each call replaces in the reference (all in src/libgkm.c unless noted):
 *   gkmhip_create / gkmhip_destroy   gkmkernel_init :978-1033, gkmkernel_destroy :1058-1068
 *   gkmhip_set_sequences             gkmkernel_new_object :841-938 (encoding, rc strand,
 *                                    positional weights) + gkmkernel_build_tree :1035-1056
 *                                    (the k-mer tree is replaced by bit-plane tables)
 *   gkmhip_gram_rows                 the row loop pthread_gkmkernel_kernelfunc_batch_all
 *                                    (src/gkmkern_pylib.c:70-90) -> gkmkernel_kernelfunc_batch_all
 *                                    :1156-1185 -> kmertree_dfs :315-387, for a set of rows;
 *                                    it also yields the self terms of
 *                                    gkmkernel_kernelfunc_sqnorm_single :723-759
 *   gkmhip_normalize                 the division / RBF of :1168-1179 and the unit diagonal
 *                                    of src/gkmkern_pylib.c:218-221
 *
 * Output convention: `G` is a row-major fp64 matrix with leading dimension `ld`
 * (elements).  gkmhip_gram_rows writes RAW values G(a,j) = sum_m c_m P_m(a,j) for
 * j <= a (diagonal included, nothing above it).  gkmhip_normalize turns a matrix
 * of raw values (all rows present) into K in place.
 *
 * All functions return 0 on success and a non-zero code on failure;
 * gkmhip_last_error() describes the most recent failure of the calling thread.
 */
#ifndef GKM_HIP_H
#define GKM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gkmhip_ctx gkmhip_ctx;

/* (BITSLICE_GROUPS: the bit-sliced kernel with GROUP records -- one hit compaction per group of five words -- where a
 * same-length launch would take shift records by default: the older variants, kept as the bit-for-bit cross-check of the
 * newer ones, as DIRECT is of the bit-sliced kernel.  Everywhere else it is BITSLICE.) */
enum { GKMHIP_KERNEL_AUTO = 0, GKMHIP_KERNEL_DIRECT = 1, GKMHIP_KERNEL_BITSLICE = 2, GKMHIP_KERNEL_BITSLICE_GROUPS = 3 };

const char *gkmhip_last_error(void);
int gkmhip_device_count(void);
/* the calling thread's current HIP device (-1 if there is none) / make `device` current: the
 * boundary call restores the caller's device before it returns */
int gkmhip_current_device(void);
int gkmhip_set_current_device(int device);

/* c: the d+1 mismatch weights c_0..c_d (host-computed, include/gkmkern_pylib.h).
 * rbf != 0 selects K <- exp(gamma (K-1)) in gkmhip_normalize (kernel types 3, 5). */
gkmhip_ctx *gkmhip_create(int device, int L, int d, const double *c, int rbf, double gamma);
void gkmhip_destroy(gkmhip_ctx *ctx);

int gkmhip_n_sequences(const gkmhip_ctx *ctx); /* sequences uploaded */
int gkmhip_device_of(const gkmhip_ctx *ctx);
void gkmhip_set_error_message(const char *msg); /* what gkmhip_last_error() returns next (calling thread) */

/* choose the kernel family (default AUTO: the bit-sliced kernel where it is instantiated for (L, d) AND the faster one --
 * at most ~7.5 % of the window pairs within d mismatches for iid sequences --, the general kernel elsewhere;
 * BITSLICE and BITSLICE_GROUPS fail where the kernel is not instantiated) */
/* Per-launch scratch (row tables of one gkmhip_gram_rows* call) exists twice.  A caller that issues
 * consecutive launches on two different streams, so that one launch fills the CUs the previous one is
 * draining, selects slot 0 / 1 alternately; launches that share a slot must share a stream. */
int gkmhip_set_scratch_slot(gkmhip_ctx *ctx, int slot);

int gkmhip_set_kernel(gkmhip_ctx *ctx, int which);

/* Upload n sequences.  codes: base codes 0..3, concatenated; offsets[n+1] (elements).
 * wdist: positional weights as a function of the distance to the centre l-mer: the
 * weight of l-mer p of a sequence with n l-mers is wdist[|n/2 - p|] (this is all the
 * reference's exponential-decay weights depend on, src/libgkm.c:912-925); it must cover
 * distances 0..max(n)/2; entries past 1024 (no l-mer of a 2047-base sequence is that far from
 * its centre) are ignored.  wdist == NULL: all weights are 1.
 * The upload runs on `stream` and has completed when the call returns (the arrays may be freed);
 * device tables are built on first use. */
int gkmhip_set_sequences(gkmhip_ctx *ctx, int n, const uint8_t *codes, const int64_t *offsets,
                         const uint8_t *wdist, int wdist_len, void *stream);

/* Raw Gram values for the rows listed in `rows` (host array of nrows ascending sequence
 * indices): row rows[i] is written to G + i*ld (local_rows != 0) or to
 * G + rows[i]*ld (local_rows == 0).  `G` is a DEVICE pointer.  If P != NULL (device,
 * int32) the integer mismatch profiles are stored as P[(i_or_row*ldp + j)*(d+1) + m]
 * for j <= a.  Both ld and, where P is given, ldp must exceed the largest row index listed (error 2 otherwise, nothing
 * launched).  Work is enqueued on `stream` (a hipStream_t, may be NULL). */
int gkmhip_gram_rows(gkmhip_ctx *ctx, const int *rows, int nrows, int local_rows, double *G,
                     int64_t ld, int32_t *P, int64_t ldp, void *stream);

/* The same rows into a PACKED slab: row rows[i] is written to G + row_off[i] (host array of nrows element offsets),
 * columns 0..rows[i] only -- rows[i] + 1 doubles, so rows may sit back to back.  This is the send buffer of the
 * multi-GPU all-gather (gkmhip_gram_allgather; layout in gkmqc_amd/csrc/gkm_shard.h): only j <= a is ever read, and
 * shipping n doubles per row moved twice the bytes (round 3). */
int gkmhip_gram_rows_packed(gkmhip_ctx *ctx, const int *rows, int nrows, double *G, const int64_t *row_off,
                            void *stream);

/* Rectangular variant for prediction-style use (the batch-vs-support-vector call of the
 * reference, gkmkernel_kernelfunc_batch, src/libgkm.c:1115-1153): raw G(rows[i], j) for EVERY
 * uploaded sequence j (not only j <= a).  G needs ld >= n. */
int gkmhip_gram_rows_full(gkmhip_ctx *ctx, const int *rows, int nrows, int local_rows, double *G, int64_t ld,
                          void *stream);

/* A block of columns (scoring: the support vectors as rows, a block of queries as the columns): raw G(rows[i], j) for
 * col_begin <= j < col_end, stored at G[i*ld + (j - col_begin)]; every (row, column) pair of the range, no triangle; the
 * rows (host array, strictly ascending) may lie inside or outside the range.  ld >= col_end - col_begin.  G is a DEVICE
 * pointer; the work is enqueued on `stream`.  Served by the same kernels as gkmhip_gram_rows. */
int gkmhip_gram_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, double *G, int64_t ld,
                      void *stream);

/* Per-base importance: rows are support vectors, the columns [col_begin, col_end) queries.  For query j and
 * each of its bases t, out[off[j] - off[col_begin] + t] = xscale[j - col_begin] * sum_i coef[i] * A_i(j)[t], the sum over
 * the rows in list order, where A_i(j)[t] = sum_m share[m] H_m[t] (ascending m) and H_m[t] is the exact integer tally of
 * w_j[p] w_i[q] over the l-mer pairs (query l-mer p, forward or reverse-complement l-mer q of row i) with m <= d
 * mismatches whose base t - p is a MATCHED base (off: the offsets given to gkmhip_set_sequences).  With
 * share[m] = c_m / (L - m), sum_t A_i(j)[t] = G(j, rows[i]).
 *   share  HOST, d + 1 doubles (tests pass unit vectors to read single tallies);
 *   coef   DEVICE, nrows doubles (scoring: dual_coef_i / sqnorm_i);
 *   xscale DEVICE, col_end - col_begin doubles, or NULL for 1 (scoring: 1 / sqnorm_j);
 *   out    DEVICE, the bases of the range; nothing else is written.
 * rows: host array, strictly ascending.  Needs d < L.  Bit-identical for a query whatever the range it is in: the rows are
 * cut into chunks by their number only, each chunk's sum is exact integer tallies folded in a fixed order, and the chunks
 * are summed in order.  Work is enqueued on `stream`; last_kernel_ms / last_comparisons / last_kernel_name describe it. */
int gkmhip_explain_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, const double *share,
                         const double *coef, const double *xscale, double *out, void *stream);

/* In-silico mutagenesis, support-vector side: rows are support vectors, the columns [col_begin, col_end)
 * queries.  For query j, each of its bases t and each base b (0..3 = A, C, G, T) other than x_j[t],
 *   out[4 (off[j] - off[col_begin] + t) + b] = sum_i coef[i] sum_{m ascending} (fold_u[m] U_m[t] + fold_b[m-1] B_m[t][b]),
 * the sum over the rows in list order, and 0.0 at b = x_j[t].  U_m[t] is the exact integer tally of w_j[p] w_i[q] over the
 * l-mer pairs (query l-mer p, forward or reverse-complement l-mer q of row i) with m <= d mismatches whose base t - p is
 * MATCHED; B_m[t][b] the same over the pairs with 1 <= m <= min(d + 1, L) mismatches whose base t - p is MISMATCHED with
 * base b on the row's side.  With c_{d+1} = 0, fold_u[m] = c_{m+1} - c_m and fold_b[m-1] = c_{m-1} - c_m, out is
 * sum_i coef[i] (G(y, rows[i]) - G(x_j, rows[i])) for the mutant y.  If base is not NULL,
 * base[j - col_begin] = sum_i coef[i] sum_m gcoef[m] P_m(x_j, rows[i]) (= sum_i coef[i] G(x_j, rows[i]) with gcoef = c).
 *   fold_u, gcoef HOST, d + 1 doubles (m = 0..d); fold_b HOST, d + 1 doubles (m = 1..d + 1; beyond m = L unused)
 *                 (tests pass unit vectors to read single tallies);
 *   coef          DEVICE, nrows doubles (scoring: dual_coef_i / sqnorm_i);
 *   out           DEVICE, 4 doubles per base of the range; base DEVICE, col_end - col_begin doubles, or NULL.
 * rows: host array, strictly ascending.  Any (L, d), any query length: query positions are tiled when a query's tallies
 * do not fit in LDS.  Bit-identical for a query whatever the range it is in: the rows are cut into chunks by their number
 * only and the queries into tiles by (L, d) only, each chunk's sum is exact integer tallies folded in a fixed order, and
 * the chunks and tiles are summed in order.  Work is enqueued on `stream`; last_kernel_ms / last_comparisons /
 * last_kernel_name describe k_ism. */
int gkmhip_ism_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, const double *fold_u,
                     const double *fold_b, const double *gcoef, const double *coef, double *out, double *base,
                     void *stream);

/* Hypothetical importance, raw: rows are support vectors, the columns [col_begin, col_end) queries.  For
 * query j, each of its bases t and each base b (0..3 = A, C, G, T),
 *   out[4 (off[j] - off[col_begin] + t) + b] = sum_i coef[i] sum_{m=1..d+1} share[m-1] B_m[t][b]   (b != x_j[t])
 *                                            = sum_i coef[i] sum_{m=0..d}   share[m]   U_m[t]      (b == x_j[t])
 * the sums over the rows in list order and over m in ascending order from 0.0, with U and B the tallies of
 * gkmhip_ism_block.  B_{m+1}[t][b] is gkmhip_explain_block's tally H_m[t] of the mutant y = x_j with base t set to b, so
 * with share[m] = c_m / (L - m) the value at b times 1 / sqrt(G(y, y)) is explain's value of y at t, bit for bit.
 *   share HOST, d + 1 doubles (tests pass unit vectors to read single tallies);
 *   coef  DEVICE, nrows doubles (scoring: dual_coef_i / sqnorm_i);
 *   out   DEVICE, 4 doubles per base of the range; nothing else is written.
 * rows: host array, strictly ascending.  Needs d < L.  Chunking, tiling and bit-identity as gkmhip_ism_block.  Work is
 * enqueued on `stream`; last_kernel_ms / last_comparisons / last_kernel_name describe k_ism_hyp. */
int gkmhip_hyp_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, const double *share,
                     const double *coef, double *out, void *stream);

/* Every single-base mutant's decision sum for an RBF model (kernel types 3 and 5): rows are support vectors,
 * the columns [col_begin, col_end) queries.  With gamma the context's and
 *   term(i, G, n) = dual[i] * exp(gamma * (G / (sq[rows[i]] * n) - 1))   (product first, one division, then exp: the
 *                                                                         expression gkmhip_normalize_block evaluates),
 * for query j, each of its bases t and each base b other than x_j[t],
 *   out[4 (off[j] - off[col_begin] + t) + b] = sum_i term(i, gx[i][j - col_begin] + dG_i(t, b), ysq[4 (.. + t) + b]),
 * the sum over the rows in list order, where dG_i(t, b) = sum_{m ascending} (fold_u[m] U_m[t] + fold_b[m-1] B_m[t][b]) is
 * formed from the exact tallies exactly as gkmhip_ism_block forms it; and 0.0 at b = x_j[t], which the caller fills (it
 * is base's value).  If base is not NULL, base[j - col_begin] = sum_i term(i, gx[i][j - col_begin], sq[j]).
 *   fold_u, fold_b HOST, d + 1 doubles each, as gkmhip_ism_block's;
 *   dual           DEVICE, nrows doubles (scoring: dual_coef_i, NOT divided by the norm);
 *   sq             DEVICE, n doubles: sqrt(G(i, i)) of every uploaded sequence;
 *   gx             DEVICE, row i at gx + i ld: the raw G(x_j, rows[i]) of gkmhip_gram_block over the same rows and range
 *                  (not normalised); ld >= col_end - col_begin;
 *   ysq            DEVICE, 4 doubles per base of the range: sqrt(G(y, y)) of the mutant to base b (at b = x_j[t]: unused);
 *   out            DEVICE, 4 doubles per base of the range; base DEVICE, col_end - col_begin doubles, or NULL.
 * rows: host array, strictly ascending.  A context of another kernel type is refused.  Chunking, tiling and bit-identity
 * as gkmhip_ism_block: no floating-point atomics, the chunks' partial rows are summed in chunk order.  Work is enqueued on
 * `stream`; last_kernel_ms / last_comparisons / last_kernel_name describe k_ism_rbf. */
int gkmhip_ism_rbf_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, const double *fold_u,
                         const double *fold_b, const double *dual, const double *sq, const double *gx, int64_t ld,
                         const double *ysq, double *out, double *base, void *stream);

/* In-silico mutagenesis, self side: for query j of [col_begin, col_end), each base t and each base b (0..3),
 *   prof[(4 (off[j] - off[col_begin] + t) + b) (d + 1) + m] = P_m(y, y), m = 0..d,
 * the exact integer mismatch profile of y = x_j with base t set to b against itself (b = x_j[t]: P_m(x_j, x_j)), as
 * gkmhip_self_norms counts it: forward l-mers of y against forward and reverse-complement l-mers of y.
 *   prof DEVICE, 4 (d + 1) int64 per base of the range; nothing else is written.
 * Work is enqueued on `stream`; last_kernel_ms / last_comparisons / last_kernel_name describe k_ism_self_base + k_ism_self. */
int gkmhip_ism_self_profiles(gkmhip_ctx *ctx, int col_begin, int col_end, int64_t *prof, void *stream);

/* Exact self profiles: for every uploaded sequence j of [col_begin, col_end),
 *   pself[(j - col_begin) (d + 1) + m] = P_m(x_j, x_j), m = 0..d,
 * the integer mismatch profile of x_j against itself (forward l-mers against forward and reverse-complement l-mers) in
 * 64 bits.  gkmhip_self_norms keeps the reference's 32-bit profile, which wraps once a profile reaches 2^31 (a long
 * low-complexity sequence with large positional weights); below that, sum_m c_m (double)pself[m] in ascending m from 0.0
 * is bit for bit the square of gkmhip_self_norms' value.  explain, ism, hypothetical and the l-mer tables take their
 * norms from here.
 *   pself DEVICE, (col_end - col_begin) (d + 1) int64; nothing else is written.
 * Work is enqueued on `stream`; last_kernel_ms / last_comparisons / last_kernel_name describe k_ism_self_base. */
int gkmhip_self_profiles(gkmhip_ctx *ctx, int col_begin, int col_end, int64_t *pself, void *stream);

/* L-mer weight table: for every code u of [u_begin, u_end) (an l-mer packed as gkm_bitslice.h's
 * lmer_entry packs it, first base in the highest pair, no weight byte),
 *   W[u - u_begin] = sum_{i ascending} cv[i] * (cf + cr),   cf = c[m(u, v[i])] if that mismatch count is <= d, else 0.0,
 *                                                           cr the same for rc(v[i]),
 * the sum from 0.0 in that order whatever the range, the launch or the run (no atomics), so W[u] and W[rc(u)] are
 * bit-identical.  With v the canonical classes (min(code, rc(code))) of a model's support-vector l-mers and cv[i] the sum
 * of dual_coef_s / sq_s w_s[q] over the class, W is the model's weight per l-mer and score(x) = sum_p w_x[p] W(u_p) / sq_x
 * + rho.  L and d are the context's; no sequences need be uploaded.
 *   c  HOST, d + 1 doubles (tests pass unit vectors to count single mismatch classes);
 *   v  DEVICE, nv l-mer codes (distinct, ascending and canonical for a model's table; the sum is defined for any);
 *   cv DEVICE, nv doubles;
 *   W  DEVICE, u_end - u_begin doubles; nothing else is written.
 * 0 <= u_begin < u_end <= 4^L.  Work is enqueued on `stream`; last_kernel_ms / last_comparisons (2 nv (u_end - u_begin))
 * / last_kernel_name describe k_lmer_weights. */
int gkmhip_lmer_weights(gkmhip_ctx *ctx, const double *c, const uint32_t *v, const double *cv, int nv, uint32_t u_begin,
                        uint32_t u_end, double *W, void *stream);

/* Scores from an l-mer weight table: for every uploaded sequence j of [col_begin, col_end),
 *   out[j - col_begin] = sum_p w_j[p] W[code(u_p)]
 * over its forward l-mers u_p with their positional weights (the context's l-mer table).  One wave per sequence with a
 * fixed assignment of positions to lanes and a fixed reduction, so the value is bit-identical whatever range or
 * neighbours the sequence has.
 *   W   DEVICE, 4^L doubles, indexed by code;
 *   out DEVICE, col_end - col_begin doubles.
 * Work is enqueued on `stream`; last_kernel_ms / last_comparisons (the l-mers looked up) / last_kernel_name describe
 * k_lmer_score. */
int gkmhip_lmer_score(gkmhip_ctx *ctx, int col_begin, int col_end, const double *W, double *out, void *stream);

/* Per-base importance table: for every code u of [u_begin, u_end) and offset i = 0..L-1 (offset 0 is the
 * l-mer's first base, in the highest pair),
 *   V[(u - u_begin) L + i] = sum_{j ascending} cv[j] * (tf + tr),   tf = share[m(u, v[j])] if that mismatch count is <= d
 *                                                                   and base i of u equals base i of v[j], else 0.0,
 *                                                                   tr the same for rc(v[j]),
 * the sum from 0.0 in that order whatever the range, the launch or the run (no atomics), so V[rc(u)][L-1-i] and V[u][i]
 * are bit-identical.  With (v, cv) the classes of gkmhip_lmer_weights and share[m] = c[m] / (L - m), sum_i V[u][i] is
 * that table's W[u] and explain(x)[t] = sum_i w_x[t-i] V[u_{t-i}][i] / sq_x.  L and d are the context's; no sequences
 * need be uploaded.
 *   share HOST, d + 1 doubles (tests pass unit vectors to count single mismatch classes);
 *   v     DEVICE, nv l-mer codes; cv DEVICE, nv doubles;
 *   V     DEVICE, (u_end - u_begin) L doubles, row-major; nothing else is written.
 * 0 <= u_begin < u_end <= 4^L.  Work is enqueued on `stream`; last_kernel_ms / last_comparisons (2 nv (u_end - u_begin))
 * / last_kernel_name describe k_lmer_importance. */
int gkmhip_lmer_importance(gkmhip_ctx *ctx, const double *share, const uint32_t *v, const double *cv, int nv,
                           uint32_t u_begin, uint32_t u_end, double *V, void *stream);

/* Explanations from an importance table: for every uploaded sequence j of [col_begin, col_end) and each of its bases t,
 *   E[off[j] - off[col_begin] + t] = xscale[j - col_begin] * sum_{i ascending} w_j[t-i] V[code(u_{t-i}) L + i]
 * over the offsets i = 0..L-1 whose l-mer t - i exists (the context's forward l-mer table), from 0.0.  One thread per
 * base and a fixed order: bit-identical whatever range or neighbours the sequence has.
 *   V      DEVICE, 4^L x L doubles (gkmhip_lmer_importance over all codes);
 *   xscale DEVICE, col_end - col_begin doubles (explaining: 1 / sqnorm_j);
 *   E      DEVICE, one double per base of the range.
 * Work is enqueued on `stream`; last_kernel_ms / last_comparisons (the values gathered, L per l-mer) / last_kernel_name
 * describe k_lmer_explain. */
int gkmhip_lmer_explain(gkmhip_ctx *ctx, int col_begin, int col_end, const double *V, const double *xscale, double *E,
                        void *stream);

/* Raw hypothetical importance from an importance table: for sequence j of the range, each base t and each base b (0..3),
 *   R[4 (off[j] - off[col_begin] + t) + b] = sum_{i ascending} w_j[t-i] V[code(u_{t-i} with base i set to b) L + i],
 * gkmhip_lmer_explain's sum (unscaled) of the mutant y = x_j with base t set to b, at t; at b = x_j[t] that of x_j itself,
 * bit for bit.
 *   V DEVICE, 4^L x L doubles; R DEVICE, 4 doubles per base of the range.
 * Work is enqueued on `stream`; last_kernel_ms / last_comparisons (the values gathered, 4 L per l-mer) / last_kernel_name
 * describe k_lmer_hyp. */
int gkmhip_lmer_hyp(gkmhip_ctx *ctx, int col_begin, int col_end, const double *V, double *R, void *stream);

/* ---- scanning a long sequence with an l-mer weight table (gkm_scan.hip) ----
 * The score of every window of `width` bases (L <= width <= 2047) at a stride, each as if the window were a sequence of
 * its own.  The long sequence does not go through gkmhip_set_sequences: these calls take the context for L and d only,
 * and plain DEVICE pointers.  With n = width - L + 1, wt the n positional weights every window shares (DEVICE, n bytes:
 * gkm_position_weights of n) and window i = the l-mers [i stride, i stride + n) of lm:
 *
 * gkmhip_scan_lmers: lm[p] = the code of the forward l-mer at base p (first base in the highest pair), bit 31 set when
 * it covers a base whose valid[] byte is 0.  codes, valid: nbases bytes each (codes 0..3); lm: nbases - L + 1 words. */
int gkmhip_scan_lmers(gkmhip_ctx *ctx, const uint8_t *codes, const uint8_t *valid, int64_t nbases, uint32_t *lm,
                      void *stream);
/* prof[i (d + 1) + m] = P_m of window i against itself, m = 0..d, exact in 64 bits:
 *   sum_{p, q in window i} wt[p - a_i] wt[q - a_i] ([m(f_p, f_q) = m] + [m(f_p, rc f_q) = m])
 * -- gkmhip_self_profiles' value for the window cut out as a sequence.  lm may point into a longer array (the first
 * window's first l-mer); nlm: the words readable from there, at least (nwin - 1) stride + n.  A flagged l-mer takes part
 * in no pair (the caller drops the windows that hold one).  One workgroup serves a stretch of gkmhip_scan_group
 * consecutive windows and compares every l-mer pair of the stretch once per strand, not once per window.
 * last_kernel_ms / last_comparisons (the pair comparisons made, strands counted singly) / last_kernel_name describe
 * k_scan_profiles. */
int gkmhip_scan_profiles(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width, int stride,
                         int64_t nwin, int64_t *prof, void *stream);
/* out[i] = sum_p wt[p] W[code(lm[i stride + p])], summed as gkmhip_lmer_score sums a sequence (bit-identical to it for
 * the window cut out).  W: DEVICE, 4^L doubles.  last_* describe k_scan_score. */
int gkmhip_scan_score(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width, int stride,
                      int64_t nwin, const double *W, double *out, void *stream);
/* windows per stretch of k_scan_profiles: a function of (L, width, stride) only; 0 for arguments the scan refuses */
int gkmhip_scan_group(const gkmhip_ctx *ctx, int width, int stride);

/* ---- windowed kernel matrices between two long sequences (gkm_wsim.hip) ----
 * The gkm kernel between every window of `width` bases (L <= width <= 2047) of a record x at stride_x and every window
 * of a record y at stride_y, each pair as if the two windows were sequences of their own.  Unweighted kernel types only
 * (0..3): with positional weights a pair's value would depend on the window that holds it.  Like the scan calls these
 * take the context for L, d, the coefficients, the RBF flag and gamma only, and plain DEVICE pointers.  lmx, lmy: the
 * words of gkmhip_scan_lmers from the first window's first l-mer on (they may point into longer arrays); nlmx, nlmy: the
 * words readable from there, at least (nw - 1) stride + n with n = width - L + 1.  Window i of x = the l-mers
 * [i stride_x, i stride_x + n) of lmx, window j of y = [j stride_y, j stride_y + n) of lmy.
 *
 * gkmhip_wsim_profiles: G[i ld + j] = ((0.0 + c_0 P_0) + c_1 P_1) + ... + c_d P_d, the raw value of gkmhip_gram_rows for
 * the two windows cut out, with
 *   P_m(i, j) = sum_{p in window i} sum_{q in window j} ([m(f_p, g_q) = m] + [m(f_p, rc g_q) = m])
 * and, where prof is not NULL, prof[(i nwy + j) (d + 1) + m] = P_m(i, j) (int32; 2 n^2 < 2^31).  Cells of G beyond
 * column nwy of a row are not written; nothing else is.  A flagged l-mer takes part in no pair (the caller gives the
 * windows that hold one a NaN norm).  One workgroup serves a tile of gkmhip_wsim_group windows of x by windows of y and
 * compares every l-mer pair of the tile once per strand, not once per window pair.  last_kernel_ms / last_comparisons
 * (the sum over tiles of 2 Sx Sy, the l-mer words of the tile on either axis) / last_kernel_name describe
 * k_wsim_profiles.  Refused with error 2, nothing written: a NULL lmx, lmy or G, a width outside L..2047, a stride
 * below 1, nwx or nwy outside 1..2^30 or more than 2^38 pairs, ld < nwy, windows beyond nlmx or nlmy, more than
 * 2^31 - 1 tiles. */
int gkmhip_wsim_profiles(gkmhip_ctx *ctx, const uint32_t *lmx, int64_t nlmx, const uint32_t *lmy, int64_t nlmy, int width,
                         int stride_x, int stride_y, int64_t nwx, int64_t nwy, double *G, int64_t ld, int32_t *prof,
                         void *stream);
/* in place: G[i ld + j] / (sqx[i] sqy[j]) (the product first, one division, as gkmhip_normalize_block), RBF contexts
 * exp(gamma (K - 1)) of that.  No unit diagonal is forced.  A NaN norm makes its row (sqx) or column (sqy) NaN.
 * last_* describe k_wsim_normalize. */
int gkmhip_wsim_normalize(gkmhip_ctx *ctx, double *G, int64_t ld, int64_t nwx, int64_t nwy, const double *sqx,
                          const double *sqy, void *stream);
/* per row i of K (nwx x nwy, leading dimension ld): best_j[i] = the ELIGIBLE column with the largest K[i ld + j], the
 * lowest such j on a tie, best_k[i] = its value; -1 and NaN where no column is eligible.  Column j is eligible when
 * K[i ld + j] is not a NaN and |start_x + i stride_x - (start_y + j stride_y)| >= min_separation (bases; 0: every
 * column).  Starts and min_separation in 0..2^40.  One wave per row, no atomics.  last_* describe k_wsim_best. */
int gkmhip_wsim_best(gkmhip_ctx *ctx, const double *K, int64_t ld, int64_t nwx, int64_t nwy, int64_t start_x,
                     int64_t stride_x, int64_t start_y, int64_t stride_y, int64_t min_separation, int64_t *best_j,
                     double *best_k, void *stream);
/* windows of a tile of k_wsim_profiles along x and y: a function of (L, d, width, stride_x, stride_y) only; 1 along an
 * axis whose stride is at least n.  Needs no context and no device.  0, or 2 (and 0, 0) for arguments the launch
 * refuses. */
int gkmhip_wsim_group(int L, int d, int width, int stride_x, int stride_y, int *gx, int *gy);

/* ---- the best local path through a windowed kernel matrix (gkm_walign.hip) ----
 * Smith-Waterman with a linear gap penalty, in doubles, over a block K (nwx x nwy, leading dimension ld) as
 * gkmhip_wsim_normalize leaves it, in DP coordinates (i, c): i the row of K, c its DP column, which reads K[i ld + c], or
 * with flip != 0 K[i ld + nwy - 1 - c] (the columns walked backwards: the reverse orientation).  With offset finite and
 * gap >= 0 finite,
 *   v = K(i, j(c));  h = 0.0, dir = 0 (STOP)
 *   if v == v:  t = H(i-1, c-1) + (v - offset);  if t > h: h = t, dir = 1 (DIAG)
 *   t = H(i-1, c) - gap;                         if t > h: h = t, dir = 2 (UP)
 *   t = H(i, c-1) - gap;                         if t > h: h = t, dir = 3 (LEFT)
 *   H(i, c) = h;  D(i, c) = dir
 * every comparison a strict >, in that order; a NaN K takes no diagonal step but may be crossed by gap steps.  The bits
 * of every H follow from the definition alone: not from the tiling, the launch or the run.
 *
 * gkmhip_walign_block: the DP over one block, the cells beyond its upper and left edge given by the caller, so that a
 * matrix cut into blocks is served block row by block row, each from left to right in DP columns.  top: nwy doubles,
 * read as H(-1, 0..nwy-1) and overwritten in place with the block's last row; left: nwx doubles, read as H(0..nwx-1, -1)
 * and overwritten in place with the block's last column; corner: one DEVICE double, H(-1, -1), read only.  D: NULL (a
 * score-only run) or uint8 [nwx][ldd], D[i ldd + c] in DP coordinates; cells beyond column nwy of a row are not written.
 * best_h (one double) and best_ic (two int64: i, c, local to the block): the block's best cell -- the largest H, the
 * lower i and then the lower c on a tie -- or (0.0, -1, -1) where no H is positive.  scratch: DEVICE, 8-byte aligned, at
 * least gkmhip_walign_scratch_bytes(nwx, nwy) bytes (-1 for nwx or nwy outside 1..2^20).  One wave serves a tile of
 * gkmhip_walign_tile rows by columns (needs no context and no device); tile (I, J) needs (I-1, J) and (I, J-1), so the
 * call issues one launch per tile anti-diagonal on `stream`, tiles_x + tiles_y - 1 of them, and does not wait: no
 * workgroup waits for another.  No atomics.  last_kernel_ms (all the call's launches) / last_kernel_name describe
 * k_walign_tiles; last_comparisons: nwx nwy cells.  Refused with error 2, nothing written: a NULL pointer other than D,
 * ld < nwy, ldd < nwy (with or without D), nwx or nwy outside 1..2^20, a non-finite offset, a gap that is negative or not finite,
 * a scratch too small. */
int gkmhip_walign_tile(int *rows, int *cols);
int64_t gkmhip_walign_scratch_bytes(int64_t nwx, int64_t nwy);
int gkmhip_walign_block(gkmhip_ctx *ctx, const double *K, int64_t ld, int64_t nwx, int64_t nwy, int flip, double offset,
                        double gap, double *top, double *left, const double *corner, uint8_t *D, int64_t ldd,
                        double *best_h, int64_t *best_ic, void *scratch, int64_t scratch_bytes, void *stream);
/* Walks D (uint8 [nwx][ldd], the WHOLE problem's, in DP coordinates) back from (end_i, end_c): DIAG to (i-1, c-1), UP to
 * (i-1, c), LEFT to (i, c-1), until a STOP cell (any byte but 1, 2, 3 stops) or until the walk leaves the matrix.  path:
 * the DIAG cells as (i, c) int32 pairs from the end backwards; count: three int64, the number of pairs and the cell (i, c)
 * at which the walk stopped (the STOP cell, or the first cell outside: i or c is -1).  One wave; the 64 x 64 direction
 * bytes up-left of the current cell are staged in LDS and walked there.  Every step lowers i + c: at most nwx + nwy
 * steps whatever D holds.  last_* describe k_walign_trace.  Refused with error 2, nothing written: a NULL pointer,
 * ldd < nwy, nwx or nwy outside 1..2^20, an end cell outside the matrix, capacity < min(nwx, nwy) pairs. */
int gkmhip_walign_trace(gkmhip_ctx *ctx, const uint8_t *D, int64_t ldd, int64_t nwx, int64_t nwy, int64_t end_i,
                        int64_t end_c, int32_t *path, int64_t capacity, int64_t *count, void *stream);

/* ---- regions of a scan: thresholded runs of windows with their summits (gkm_regions.hip) ----
 * Over the nwin windows of a scan launch (the same lm, nlm, width, stride) and their finished scores score[i ld] (DEVICE;
 * ld >= 1, so a column of a panel's nwin x nm result is served where it lies).  Window i PASSES when none of its
 * width - L + 1 words of lm is flagged (bit 31) and score[i ld] >= threshold by IEEE comparison (a NaN never passes; a
 * threshold of -inf passes every window without a flagged word; a NaN threshold is refused).  Consecutive passing windows
 * p < q belong to one region when q - p <= gap + 1 (gap >= 0).  A region is five values in window indices of THIS launch:
 * first, last (its first and last passing window), windows (how many passed), peak (the largest score among them) and
 * summit (the first passing window that attains it); regions ascend.  The launch knows nothing of its neighbours.
 * Nothing is added and no atomic is used: the same arguments give the same bytes on every run.
 *
 * gkmhip_regions_count: *count (HOST) = the regions of the launch; complete on return (it waits for `stream`).  scratch:
 * DEVICE, 8-byte aligned, at least gkmhip_regions_scratch_bytes(nlm, nwin) bytes (-1 for nlm < 1, nlm >= 2^40 or nwin
 * outside 1..2^30); it keeps what gkmhip_regions_fill needs.
 * gkmhip_regions_fill: after gkmhip_regions_count with the same arguments and scratch (anything else is refused, error 2,
 * from a 64-byte header it reads back): regions 0 .. count - 1 into the five DEVICE arrays of `capacity` elements each.
 * No cell beyond count - 1 is written.  capacity < count: error 2 and nothing is written.  count == 0: nothing is
 * launched and the arrays may be NULL.
 * last_kernel_ms / last_kernel_name: k_regions_summaries for the count call (the events bracket all its launches: the
 * prefix count of flagged words, the wave summaries and their scan) and k_regions_fill for the fill call;
 * last_comparisons: nwin.  gkmhip_regions_span: the windows one workgroup of either kernel owns. */
int64_t gkmhip_regions_scratch_bytes(int64_t nlm, int64_t nwin);
int gkmhip_regions_count(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                         int stride, int64_t nwin, double threshold, int64_t gap, void *scratch, int64_t scratch_bytes,
                         int64_t *count, void *stream);
int gkmhip_regions_fill(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                        int stride, int64_t nwin, double threshold, int64_t gap, void *scratch, int64_t scratch_bytes,
                        int64_t capacity, int32_t *first, int32_t *last, int32_t *summit, int32_t *windows, double *peak,
                        void *stream);
int gkmhip_regions_span(void);

/* ---- the distribution of a scan's scores: digit histograms, edge histograms, bounded collection (DESIGN.md §5p;
 * gkm_dist.hip) ----
 * Over the nwin windows of a scan launch and their finished scores score[i ld], as the region calls take them.  Window i
 * is SCORED when none of its width - L + 1 words of lm is flagged (bit 31) and score[i ld] is no NaN; what stands at any
 * other window is never used as a value.  The KEY of a double with the bits b is b ^ (b >> 63 ? ~0 : 1 << 63), a
 * bijection of 64-bit words under which ascending keys are ascending non-NaN doubles, -0.0 just below +0.0.
 *
 * gkmhip_dist_digit_bits: B, the bits of a key one refinement level resolves.  The 64 bits are resolved in
 * ceil(64 / B) levels: the first takes the top 64 - B (levels - 1) bits, every later one the next B; the level
 * boundaries are the numbers of bits resolved after each level.
 * gkmhip_dist_scratch_bytes: what each call below needs as `scratch` (DEVICE, 8-byte aligned); -1 for nlm outside
 * 1..2^40 - 1 or nwin outside 1..2^30.
 *
 * gkmhip_dist_digits ADDS to hist (DEVICE uint64, never zeroed here: a pass runs over many launches).  nprefix == 0
 * (prefix_bits 0): every scored window adds 1 at hist[its key's first-level digit], 2^(first level's bits) counters.
 * Otherwise prefix is a HOST array of 1..64 strictly ascending values of prefix_bits bits, prefix_bits a level boundary
 * below 64 (anything else: error 2): a scored window whose key's top prefix_bits bits equal prefix[j] adds 1 at
 * hist[j 2^B + the key's next B bits]; other windows add nothing.  hist: max(nprefix, 1) rows.
 * gkmhip_dist_edges ADDS 1 at hist[#{j : edges[j] <= v}] for every scored window's score v (numpy's searchsorted(edges, v,
 * side="right"), compared as doubles): edges DEVICE, nedges in 1..4096 ascending doubles without a NaN, which is the
 * caller's duty (they are read on the device only); hist: nedges + 1 counters.
 * gkmhip_dist_collect: every scored window whose key's top prefix_bits bits equal one of the 1..64 prefixes appends its
 * score to out (DEVICE) at the running *counter (DEVICE int64, in and out): *counter advances by the matches whatever
 * the capacity, and values at positions >= capacity are dropped, not written.  The order of the appended values is
 * not defined; their multiset is.
 *
 * All counting is by integer atomics, so the counters are the same bytes on every run.  Nothing but the documented
 * cells is written.  A workgroup owns 1024 consecutive windows.  The calls launch on `stream` and do not wait.
 * last_kernel_name: k_dist_digits, k_dist_edges, k_dist_collect (the events bracket the prefix count of flagged words
 * too); last_comparisons: nwin. */
int gkmhip_dist_digit_bits(void);
int64_t gkmhip_dist_scratch_bytes(int64_t nlm, int64_t nwin);
int gkmhip_dist_digits(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                       int stride, int64_t nwin, const uint64_t *prefix, int nprefix, int prefix_bits, uint64_t *hist,
                       void *scratch, int64_t scratch_bytes, void *stream);
int gkmhip_dist_edges(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                      int stride, int64_t nwin, const double *edges, int nedges, uint64_t *hist, void *scratch,
                      int64_t scratch_bytes, void *stream);
int gkmhip_dist_collect(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                        int stride, int64_t nwin, const uint64_t *prefix, int nprefix, int prefix_bits, double *out,
                        int64_t capacity, int64_t *counter, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- variant effects from an l-mer weight table: deltaSVM (gkm_delta.hip) ----
 * The change in the summed weights of the l-mers a variant touches.  For a base string z with n = len(z) - L + 1 l-mers
 * u_0 .. u_{n-1}, S(z) = ((0.0 + W[u_0]) + W[u_1]) + ... + W[u_{n-1}] in plain double additions, 0.0 when n < 1.  No
 * positional weights enter (a variant has no window).  Like the scan calls these take the context for L only and plain
 * DEVICE pointers unless said otherwise; W: DEVICE, 4^L doubles; lm: the words of gkmhip_scan_lmers over the same bases.
 * Every value is one lane's own chain of additions: it depends on W and the bases around the variant only, not on the
 * launch, the other variants or the run.
 *
 * gkmhip_delta_sat: every SNV of the positions [t_begin, t_end) of the nlm + L - 1 bases that lm covers:
 *   out[(t - t_begin) * 4 + b] = S(context of t with base t replaced by b) - S(context of t),
 * the context being the bases [max(0, t - (L-1)), min(nlm + L - 1, t + L)), whose l-mers are lm[max(0, t-L+1) ..
 * min(t, nlm-1)]; the base at t is read from those words.  +0.0 at b = the base at t; all four NaN when a word of the
 * context is flagged (bit 31).  out: (t_end - t_begin) x 4 doubles, 16-byte aligned.  last_comparisons: the W gathers
 * made (four per l-mer over a position); last_kernel_ms / last_kernel_name describe k_delta_sat. */
#define GKMHIP_DELTA_MAX_ALLELE 255
int gkmhip_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end, const double *W,
                     double *out, void *stream);
/* out[i] = S(x[a:pos] + alt_i + x[pos+r:e]) - S(x[a:e]) for variant i = (pos, r, alt_off, alt_len), four int32 in a
 * row of var, replacing the r bases from pos by the alt_len bases alt[alt_off ..]; a = max(0, pos - (L-1)), e =
 * min(nbases, pos + r + (L-1)); both alleles at most GKMHIP_DELTA_MAX_ALLELE bases, either may be empty.  var (nvar x 4)
 * and alt (nalt base codes) are HOST arrays: every variant is checked against nbases and nalt before anything is
 * launched (error 2 names the first that fails), and both are on the device when the call returns.  codes: DEVICE, nbases
 * base codes 0..3; lm: DEVICE, their nbases - L + 1 words (not read, and may be NULL, when nbases < L).  Validity is the
 * caller's: flags in lm are ignored (a variant over an invalid base has no value; gkmpredict.delta makes it NaN).
 * last_comparisons: the W gathers made (the l-mers of both strings); last_* describe k_delta_variants. */
int gkmhip_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases, const int32_t *var,
                          int nvar, const uint8_t *alt, int64_t nalt, const double *W, double *out, void *stream);

/* ---- l-mer weight panels: many tables per lookup (gkm_panel.hip, gkm_delta.hip) ----
 * nm tables (1 <= nm <= GKMHIP_PANEL_MAX) that share the context's parameters, interleaved: P[u * ms + m] = W_m[u], DEVICE,
 * 4^L rows of ms doubles, ms >= nm and ms % 8 == 0 (rows of whole 64-byte lines), what lies beyond column nm never
 * surfaces.  Each call is its single-table counterpart for every model at once -- the same arguments, the same refusals
 * (error 2; also for a null P, nm outside 1..64, ms < nm, ms % 8 != 0) -- with the model index as the last axis of the
 * output, and for every m the value written is, bit for bit, what the counterpart writes for the table P[:, m]: the same
 * order of additions per model, no atomics, nothing that depends on the launch.  last_comparisons: the ROWS looked up
 * (the counterpart's count, not multiplied by nm); last_kernel_ms / last_kernel_name describe k_panel_score,
 * k_panel_scan_score, k_panel_delta_sat and k_panel_delta_variants.
 *   gkmhip_panel_score           out: (col_end - col_begin) x nm doubles   (gkmhip_lmer_score)
 *   gkmhip_panel_scan_score      out: nwin x nm doubles                    (gkmhip_scan_score)
 *   gkmhip_panel_delta_sat       out: (t_end - t_begin) x 4 x nm doubles   (gkmhip_delta_sat)
 *   gkmhip_panel_delta_variants  out: nvar x nm doubles                    (gkmhip_delta_variants) */
#define GKMHIP_PANEL_MAX 64
int gkmhip_panel_score(gkmhip_ctx *ctx, int col_begin, int col_end, const double *P, int nm, int ms, double *out,
                       void *stream);
int gkmhip_panel_scan_score(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width, int stride,
                            int64_t nwin, const double *P, int nm, int ms, double *out, void *stream);
int gkmhip_panel_delta_sat(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, int64_t t_begin, int64_t t_end, const double *P,
                           int nm, int ms, double *out, void *stream);
int gkmhip_panel_delta_variants(gkmhip_ctx *ctx, const uint32_t *lm, const uint8_t *codes, int64_t nbases, const int32_t *var,
                                int nvar, const uint8_t *alt, int64_t nalt, const double *P, int nm, int ms, double *out,
                                void *stream);

/* A panel folded in one pass (gkm_panel_fold.hip): gkmhip_lmer_weights for nm models at once, written
 * into the panel's own device image.  For every code u of [u_begin, u_end) and every model m < nm,
 *   P[(u - u_begin) * ms + m] = sum_{i ascending} CV[i * ms + m] * (cf + cr)      (cf, cr as gkmhip_lmer_weights defines them)
 * from 0.0 in that order: bit for bit what gkmhip_lmer_weights writes for (v, CV[:, m]), whatever nm, ms, the range, the
 * launch or the run (no atomics; no workgroup waits for another).  The comparisons are made once for all models.
 *   c  HOST, d + 1 doubles;
 *   v  DEVICE, nv l-mer codes (for a panel: the ascending union of the models' canonical classes);
 *   CV DEVICE, nv rows of ms doubles: CV[i * ms + m] is class i's coefficient for model m (0.0 where m lacks the class);
 *   P  DEVICE, (u_end - u_begin) rows of ms doubles; columns nm..ms-1 are written as +0.0; nothing else is written.
 * Refusals (error 2, nothing written): those of gkmhip_lmer_weights and of the panel calls above.  last_comparisons:
 * 2 nv (u_end - u_begin), not multiplied by nm; last_kernel_ms / last_kernel_name describe k_panel_weights. */
int gkmhip_panel_weights(gkmhip_ctx *ctx, const double *c, const uint32_t *v, const double *CV, int nv, int nm, int ms,
                         uint32_t u_begin, uint32_t u_end, double *P, void *stream);

/* ---- a weight table or panel contracted with position weight windows (gkm_contract.hip) ----
 * A window is L rows of four doubles, P[i][b]: l-mer position i (0 the first base, the highest bit pair of a code), base b
 * (A, C, G, T).  Its value a(P) = sum over all 4^L codes u of W(u) prod_i P[i][u_i] is evaluated in one fixed order, the
 * last base first, every product and sum rounded:
 *   T_L[u] = W[u];  T_i[v] = ((T_{i+1}[4v] P[i][0] + T_{i+1}[4v+1] P[i][1]) + T_{i+1}[4v+2] P[i][2]) + T_{i+1}[4v+3] P[i][3]
 *   a(P) = T_0[0]
 * so the bits written follow from W and P alone: not from the tiling, the launches or the run.  No atomics.
 *   gkmhip_lmer_contract   W: 4^L DEVICE doubles; P: nwin x L x 4 DEVICE doubles; out: nwin doubles
 *   gkmhip_panel_contract  rows: the panel image (4^L rows of ms doubles, as above); out: nwin x ld doubles, ld >= nm, row w
 *                          holds the nm models' values of window w, cells nm..ld-1 keep their bytes; column m is, bit for
 *                          bit, gkmhip_lmer_contract on the table rows[:, m]
 * The partial values of the tiles (L > 6) live in the context and grow on demand, gkmhip_contract_scratch_bytes(L, nm,
 * nwin) bytes of them (nm = 0: a single table; -1 for refused arguments): the caller provides no scratch, and calls on
 * one context must be ordered by their streams.  nwin == 0 succeeds without a launch.  Refused with error 2, nothing
 * written: a NULL pointer, nwin < 0 or above gkmhip_contract_max_windows(L, nm) (at most GKMHIP_CONTRACT_MAX_WINDOWS, fewer
 * where the partials would pass 4 GiB; -1 for L outside 2..12 or nm outside 0..64), ld < nm, nm outside 1..64, a bad ms.
 * last_kernel_ms covers the tile kernel and the fold; last_kernel_name: k_lmer_contract / k_panel_contract;
 * last_comparisons: 4^L nwin (times nm). */
#define GKMHIP_CONTRACT_MAX_WINDOWS 65536
int64_t gkmhip_contract_max_windows(int L, int nm);
int64_t gkmhip_contract_scratch_bytes(int L, int nm, int64_t nwin);
int gkmhip_lmer_contract(gkmhip_ctx *ctx, const double *W, const double *P, int64_t nwin, double *out, void *stream);
int gkmhip_panel_contract(gkmhip_ctx *ctx, const double *rows, int nm, int ms, const double *P, int64_t nwin, double *out,
                          int64_t ld, void *stream);

/* ---- the genome window index of null-sequence sampling (gkm_nullidx.hip) ----
 * One chromosome: seq = T raw FASTA bytes, line breaks removed, case kept; t = the window width, 1 <= t <= 2047.  Per byte:
 * na (one of nN), cg (one of cgCG), rp (one of acgt); any other byte sets none.  The windows are the starts i in
 * [0, T - t): nwin = max(0, T - t) of them (the start T - t is not one).  NA_i, CG_i, RP_i: the flags summed over
 * [i, i + t).  A window is indexed iff NA_i == 0, under the key CG_i (t + 1) + RP_i.  These calls take no context: a
 * device index, plain DEVICE pointers and a stream.  Each refuses t outside 1..2047 and T >= 2^31 - 1 (error 2) before
 * it looks at anything else, and launches nothing then.  Every output is the same bytes on every run.
 *
 * gkmhip_nullidx_keys: key[i] for the nwin windows (0xFFFFFFFF where NA_i > 0) and the three flags of all T bases packed
 * eight per byte, the first base in the highest bit, the last byte zero-padded: na, cg, rp of (T + 7) / 8 bytes each,
 * 8-byte aligned.  One workgroup serves gkmhip_nullidx_tile() consecutive windows. */
int gkmhip_nullidx_tile(void);
int gkmhip_nullidx_keys(int device, const uint8_t *seq, int64_t T, int t, uint32_t *key, uint8_t *na, uint8_t *cg, uint8_t *rp,
                        void *stream);
/* the bytes of DEVICE scratch the two calls below ask for (the sort's two pairs of buffers and its digit counts), -1
 * for arguments they refuse */
int64_t gkmhip_nullidx_scratch_bytes(int64_t T, int t);
/* ptr[c (t + 1) + r] = the number of indexed windows with a key below c (t + 1) + r (an empty cell carries the running
 * total) and ptr[(t + 1)^2] = their number, len: (t + 1)^2 + 1 int32.  key: what gkmhip_nullidx_keys wrote for (T, t). */
int gkmhip_nullidx_cells(int device, const uint32_t *key, int64_t T, int t, int32_t *ptr, void *scratch, int64_t scratch_bytes,
                         void *stream);
/* pos[0 .. len): the indexed window starts ordered by key, ascending inside a key; pos has room for nwin int32 and
 * what lies behind len is the starts of the windows that hold an N.  A stable least-significant-digit radix sort over
 * the key bits in which no atomic places an element. */
int gkmhip_nullidx_sort(int device, const uint32_t *key, int64_t T, int t, int32_t *pos, void *scratch, int64_t scratch_bytes,
                        void *stream);

/* ---- nearest columns and cells above a threshold of a block of kernel values (gkm_knn.hip) ----
 * K: any DEVICE matrix of doubles, nrows x ncols with leading dimension ld >= ncols -- a block written by
 * gkmhip_gram_block + gkmhip_normalize_block, or a resident matrix.  Column j of the block is the global column
 * c = col_base + j; row_id: DEVICE int32[nrows], the global column that is row i's own, -1 for none.  Cell (i, j) is
 * ELIGIBLE iff K[i ld + j] is not a NaN and c != row_id[i] (mode 0) or c > row_id[i] (mode 1: the upper triangle).
 * Like the nullidx calls these take no context (a device index, DEVICE pointers and a stream) and keep no events: a
 * caller times them with events of its own.  Each refuses with error 2, nothing launched and nothing written: a NULL
 * pointer, negative nrows or ncols, nrows >= 2^25, ld < ncols, col_base < 0 or col_base + ncols >= 2^31, a mode other
 * than 0 and 1 (and what is named below).  nrows = 0 is served and launches nothing.  Every output is the same bytes on
 * every run: no atomic places or orders anything.
 *
 * gkmhip_knn_merge: best_idx int32[nrows kcap], best_val double[nrows kcap], 1 <= kcap <= 64 (else error 2): row i's
 * running list, larger value first and on equal values (-0.0 == 0.0) the lower global column first; the cell's own bits
 * are kept.  Unfilled entries are idx -1, val NaN at the end, which is also the state the caller writes before the first
 * call.  The call merges the eligible cells of the block into the lists, so it is made once per column block.  This is a
 * selection under a strict total order (a row's eligible cells have distinct columns): the final lists are the same
 * bytes whatever the cut into column blocks and whatever the order of the calls.  Rows whose list does not change are
 * not written. */
int gkmhip_knn_merge(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                     int64_t col_base, int mode, int kcap, int32_t *best_idx, double *best_val, void *stream);
/* count[i] (DEVICE int64[nrows], overwritten) = the eligible cells of row i with a value >= threshold (a NaN threshold:
 * none) */
int gkmhip_pairs_count(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                       int64_t col_base, int mode, double threshold, int64_t *count, void *stream);
/* Row i writes those cells in ascending column at the slots offset[i], offset[i] + 1, ...: out_i = row_id[i], out_j = c,
 * out_v = the value.  offset: DEVICE int64[nrows], the exclusive prefix of the counts plus what earlier calls wrote.
 * A slot at or beyond capacity (or below 0) is not written; a negative capacity is refused. */
int gkmhip_pairs_fill(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                      int64_t col_base, int mode, double threshold, const int64_t *offset, int64_t capacity, int32_t *out_i,
                      int32_t *out_j, double *out_v, void *stream);

/* sqnorm[i] = sqrt(G(i,i)) for all uploaded sequences (device array of n doubles), computed
 * from the diagonal band only (~1 % of the work of the whole matrix).  Replaces
 * gkmkernel_kernelfunc_sqnorm_single, src/libgkm.c:723-759. */
int gkmhip_self_norms(gkmhip_ctx *ctx, double *sqnorm, void *stream);

/* K(rows[i], j) = G / (sqnorm[rows[i]] sqnorm[j]) (+ RBF), 1.0 where j == rows[i], for rows written by
 * gkmhip_gram_rows_full with the same rows / local_rows. */
int gkmhip_normalize_rows_full(gkmhip_ctx *ctx, const int *rows, int nrows, int local_rows, double *G, int64_t ld,
                               const double *sqnorm, void *stream);

/* K = G / (sqnorm[rows[i]] * sqnorm[j]) (+ RBF) in place on a block written by gkmhip_gram_block with the same rows and
 * range; 1.0 where j == rows[i].  The same kernel and operation order as gkmhip_normalize_rows_full. */
int gkmhip_normalize_block(gkmhip_ctx *ctx, const int *rows, int nrows, int col_begin, int col_end, double *G, int64_t ld,
                           const double *sqnorm, void *stream);

/* In place on a device matrix holding raw values for ALL n rows (lower triangle +
 * diagonal): K(a,j) = G(a,j) / (sqrt(G(a,a)) sqrt(G(j,j))), optional RBF, K(a,a)=1.
 * If sqnorm != NULL (device, n doubles) it receives sqrt(G(a,a)).
 * symmetric != 0 additionally mirrors the lower triangle into the upper one. */
int gkmhip_normalize(gkmhip_ctx *ctx, double *G, int64_t ld, double *sqnorm, int symmetric,
                     void *stream);

/* plain device memory helpers so that a C host needs nothing but this header */
void *gkmhip_malloc(int device, size_t bytes);
void gkmhip_free(void *p);
int gkmhip_memcpy_d2h(void *dst, const void *src, size_t bytes);
int gkmhip_memcpy_h2d(void *dst, const void *src, size_t bytes);
int gkmhip_sync(void *stream);

/* Copy the lower triangle (+ diagonal) of a device K (n rows, ld) into caller-owned
 * host row pointers: rows[a][0..a].  Uses pinned staging and `nthreads` host threads.  ld >= n (error 2 otherwise).
 * The copies run on a stream of the call's own: K must be complete when the call is made. */
int gkmhip_copy_lower_to_rows(gkmhip_ctx *ctx, const double *K, int64_t ld, int n,
                              double **rows, int nthreads);

/* Whole Gram matrix straight into caller-owned host rows (rows[a][0..a] = K(a, 0..a-1), 1.0):
 * gram + normalise + device-to-host as a pipeline over row blocks of about equal work, so that
 * the PCIe transfer and the host-side scatter of one block overlap the kernel of the next.
 * G: device scratch of n x ld doubles.  This is what gkm_main_pywrapper uses. */
int gkmhip_gram_to_host_rows(gkmhip_ctx *ctx, double *G, int64_t ld, double **rows, int nthreads);

/* The same for one of `nparts` contexts (one per GPU, one host thread each) filling disjoint row
 * blocks of ONE host matrix: context `part` takes every nparts-th block; self norms come from a
 * diagonal-band pass, so no device needs another device's rows and no collective is involved.
 * This is how gkm_main_pywrapper uses several GPUs of a node (GKM_DEVICES). */
int gkmhip_gram_part_to_host_rows(gkmhip_ctx *ctx, double *G, int64_t ld, double **rows, int nthreads, int part,
                                  int nparts);

/* ---- several GPUs, one host process (gkm_multi.hip) ----
 * Every context (one per device, same parameters, same sequences uploaded) computes the rows of its
 * folded row blocks; the row slabs -- packed, a + 1 doubles for row a: n^2 / (2 nctx) doubles per rank and
 * matrix -- are all-gathered over xGMI (RCCL ncclAllGather on communicators
 * made by ncclCommInitAll; peer copies when several contexts share one device or RCCL cannot be
 * loaded; GKM_ALLGATHER=rccl|p2p forces one), then every device un-permutes and normalises its copy.
 * K[g]: device pointer ON ctxs[g]'s DEVICE to an n x ld matrix that receives K (lower triangle +
 * unit diagonal, the upper triangle too if symmetric != 0) -- the same matrix, bit for bit, as
 * gkmhip_gram_rows + gkmhip_normalize produce on one device.  chunks: slabs per rank whose transfer
 * overlaps the next slab's kernel (0 = chosen from (n, nctx): 1 for one context, else 2, or 3 / 4 where that pads the slabs 3 % less -- gkm_shard.h auto_chunks).  One host thread per device for the duration of
 * the call; blocks until every device holds the matrix.  This is what feeds the GPU-resident
 * cross-validation (include/gkm_svm.h) from an N-GPU matrix; the reference's consumer is
 * scripts/gkmsvm.py:104-122. */
int gkmhip_gram_allgather(gkmhip_ctx **ctxs, int nctx, double **K, int64_t ld, int symmetric, int chunks);
/* ONE rank of a `ranks`-way gkmhip_gram_allgather ALONE on its device (measurement: what a rank's step costs without
 * the transfer, on a box with one GPU): rank `rank`'s chunks exactly as gkmhip_gram_allgather runs them (same layout,
 * streams, scratch slots, packed slabs), its slab copied into its gathered buffer on the device, then the whole matrix
 * assembled and normalised into K from that buffer -- whose other ranks' slabs must be there from an earlier
 * gkmhip_gram_allgather over `ranks` contexts with the same `chunks` (all on this device: the one-GPU rehearsal).
 * out6 = {wall ms on the host clock, kernels ms (sum over the chunks' launches incl. tables / row planes / untile),
 * copy-in ms, un-permute + normalise ms, l-mer comparisons, chunks}. */
int gkmhip_gram_rank_alone(gkmhip_ctx *ctx, int rank, int ranks, int chunks, double *K, int64_t ld, int symmetric,
                           double *out6);
/* "rccl", "p2p" or "none": how the most recent gkmhip_gram_allgather moved the slabs */
const char *gkmhip_last_transport(void);
/* RCCL communicators AND each rank's buffers (its slab, the gathered slabs, gather index, self norms, streams,
 * events: ~1.7 GB per device at n = 10 000 on two devices) are kept for the life of the process, keyed by
 * (device, n, ranks, chunks): bin/gkmqc.py asks for ~20 matrices of one size per run, and hipMalloc / hipFree
 * synchronise the device.  This destroys the communicators and frees the buffers (optional). */
void gkmhip_release_comms(void);
/* hipMalloc calls gkmhip_gram_allgather has made so far in this process (a second call of the same shape makes
 * none) */
long gkmhip_allgather_alloc_count(void);
/* bytes every rank RECEIVED from its peers in the most recent gkmhip_gram_allgather (per matrix) */
long long gkmhip_allgather_bytes_per_rank(void);
/* What the most recent successful gkmhip_gram_allgather measured with HIP events on its own streams:
 * out[0] = ranks, out[1] = chunks, out[2] = transport (0 none, 1 peer copies, 2 RCCL), then for every rank
 * {kernel ms summed over its chunks, transfer ms summed over its chunks, un-permute + normalise ms, l-mer
 * comparisons of its rows}.  Returns the number of doubles written, 0 if `cap` is too small or nothing ran. */
int gkmhip_allgather_stats(double *out, int cap);
/* WHEN the chunks of rank `rank` ran in the most recent gkmhip_gram_allgather / gkmhip_gram_rank_alone: for every chunk
 * c, out[4c .. 4c+3] = start and end of its launch group (tables, row planes, Gram kernel, untile) and start and end of
 * its transfer, in ms from the start of the rank's first launch group (HIP event timestamps).  The transfer of chunk c
 * can only hide behind the kernel of chunk c + 1 if chunk c ENDS well before chunk c + 1 does.  Returns the number of
 * doubles written, 0 if `cap` is too small or nothing ran. */
int gkmhip_allgather_chunk_times(int rank, double *out, int cap);

/* Un-permutation + normalisation in one pass: matrix row a is row slot_of_row[a] (device array, n
 * int64) of `slabs` (device, leading dimension lds >= n, raw values); with lds == 1 slot_of_row[a] is the
 * element offset at which row a starts (packed slabs: gkmhip_gram_rows_packed).  K receives what
 * gkmhip_normalize would produce, sqnorm (device, n doubles) the self norms. */
int gkmhip_assemble_normalize(gkmhip_ctx *ctx, const double *slabs, int64_t lds, const int64_t *slot_of_row,
                              double *K, int64_t ld, double *sqnorm, int symmetric, void *stream);

/* A new non-blocking HIP stream on the current device that is PROVEN to run beside the `nbusy` streams of `busy`
 * (hipStream_t each): HIP maps streams onto a few hardware queues in creation order and two streams that share one
 * execute in order -- a copy or collective stream that lands on the compute stream's queue overlaps nothing.  Each
 * candidate is tried with a 2-ms spin kernel on the busy stream and a 4-byte copy on the candidate; after six
 * candidates the last one is returned anyway (*beside = 0).  NULL on error.  Destroy it with hipStreamDestroy. */
void *gkmhip_create_stream_beside(void *const *busy, int nbusy, int *beside);

/* The pinned staging buffers of the copy-out calls (2 x 64 MB) are kept for the life of the
 * process; this releases them (optional). */
void gkmhip_release_host_cache(void);

/* elapsed milliseconds of the device work of the most recent gkmhip_gram_rows call
 * (HIP events recorded on its stream around the dominant kernel); <0 if unavailable */
double gkmhip_last_kernel_ms(gkmhip_ctx *ctx);
/* Timing a LOOP of launches from outside: between gkmhip_kernel_timeline(ctx, 1) and gkmhip_kernel_timeline(ctx, 0) every
 * launch keeps its own pair of events (no host wait in between); gkmhip_kernel_timeline_ms waits for them and returns
 * the sum of the Gram kernels' durations since the last switch-on (*launches = how many), <0 on failure. */
int gkmhip_kernel_timeline(gkmhip_ctx *ctx, int on);
double gkmhip_kernel_timeline_ms(gkmhip_ctx *ctx, int *launches);
/* ... and WHEN they ran: out[2i], out[2i+1] = start and end of the i-th Gram kernel since the switch-on, in ms from the
 * start of the first (launches on different streams may overlap).  Returns the number of doubles written. */
int gkmhip_kernel_timeline_spans(gkmhip_ctx *ctx, double *out, int cap);
/* number of l-mer comparisons that call evaluated (algorithmic: 2 n_a n_j per pair) */
double gkmhip_last_comparisons(gkmhip_ctx *ctx);
const char *gkmhip_last_kernel_name(gkmhip_ctx *ctx);
/* rows that the most recent Gram launch carried as RIDERS -- in bit rows 30, 31 of lanes whose own row ends below them
 * (same-length problems) -- 0 if it packed without them or another kernel served it */
int gkmhip_last_riders(gkmhip_ctx *ctx);
/* which k_gram_bitslice variant the most recent Gram launch ran -- the kernel's PK: 1, 2 several pieces per lane (64, 128
 * row slots), 4 same length with group records, 5 the same with riders, 6 and 7 those two with shift records (DESIGN.md
 * section 5) -- or 0 where k_gram_direct served it.  The kernel's name is the same for 4 to 7. */
int gkmhip_last_variant(gkmhip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
