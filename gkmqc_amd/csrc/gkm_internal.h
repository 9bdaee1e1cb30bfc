/*
 * gkm_internal.h -- what the translation units of the MI355X (gfx950) device layer share.  Not installed; the public
 * C ABI is include/gkm_hip.h.
 *
 *   gkm_context.hip        errors, context, upload, per-sequence device tables (k_build_sb, k_pack_strands, k_pack_lmers),
 *                          pinned host pools, memory helpers, the argument checks and row upload that the launches over
 *                          (row list) x (column range) share (check_range, check_rows, scan_range, upload_rows)
 *   gkm_gram_bitslice.hip  HOT: k_gram_bitslice (bit-sliced diagonal mismatch profiles) and its instantiation table
 *   gkm_gram.hip           launch geometry (row packing, work-item order, per-launch tables), k_build_rowplanes, k_untile,
 *                          the general kernel k_gram_direct, gkmhip_gram_rows*
 *   gkm_normalize.hip      k_sqnorm, k_normalize, k_assemble_normalize: square roots of the diagonal, division, RBF
 *   gkm_copyout.hip        device matrix -> the caller's host rows: row blocks, staging pieces, the stream prober
 *   gkm_lmer_dev.h         packed l-mers on the device: scalar-load pointer types, the fields of a packed entry, reverse
 *                          complement, mismatch mask and count, the coefficient block a table kernel takes by value
 *   gkm_explain.hip        per-base importance of a trained model (k_explain, k_explain_reduce), gkmhip_explain_block
 *   gkm_ism.hip            in-silico mutagenesis of a trained model (k_ism, k_ism_reduce, k_ism_self_base, k_ism_self),
 *                          gkmhip_ism_self_profiles; hypothetical importance (k_ism<ISM_HYP>, k_ism_hyp_reduce); every
 *                          mutant's score for RBF models (k_ism<ISM_RBF>); gkmhip_ism_block, gkmhip_hyp_block and
 *                          gkmhip_ism_rbf_block, all through ism_launch<MODE>
 *   gkm_lmer.hip           l-mer weight tables of a trained model and scores from them (k_lmer_weights, k_lmer_score),
 *                          gkmhip_lmer_weights, gkmhip_lmer_score
 *   gkm_limp.hip           per-base importance tables of a trained model and explanations from them (k_lmer_importance,
 *                          k_lmer_explain, k_lmer_hyp), gkmhip_lmer_importance, gkmhip_lmer_explain, gkmhip_lmer_hyp
 *   gkm_scan.hip           every window of a long sequence scored from an l-mer weight table (k_scan_lmers, k_scan_profiles,
 *                          k_scan_score), gkmhip_scan_lmers, gkmhip_scan_profiles, gkmhip_scan_score, gkmhip_scan_group
 *   gkm_delta.hip          variant effects from an l-mer weight table or panel: every SNV of every position and a list of
 *                          variants, one body each over a weight accessor (k_delta_sat, k_delta_variants,
 *                          k_panel_delta_sat, k_panel_delta_variants), gkmhip_delta_sat, gkmhip_delta_variants,
 *                          gkmhip_panel_delta_sat, gkmhip_panel_delta_variants
 *   gkm_nullidx.hip        the genome window index of null-sequence sampling: window keys and flag planes, cell counts,
 *                          a stable radix sort of the window starts (k_nullidx_keys, k_nullidx_hist, k_nix_*,
 *                          k_nullidx_digits, k_nullidx_scatter), gkmhip_nullidx_keys, gkmhip_nullidx_cells,
 *                          gkmhip_nullidx_sort, gkmhip_nullidx_tile, gkmhip_nullidx_scratch_bytes; needs no context
 *   gkm_panel.hip          l-mer weight panels: up to 64 interleaved tables served by one lookup per l-mer, the lanes across
 *                          models: the two tree kernels (k_panel_score, k_panel_scan_score), gkmhip_panel_score,
 *                          gkmhip_panel_scan_score, and what every panel entry checks (panel_check, panel_shift)
 *   gkm_panel_fold.hip     a panel folded in one pass: the comparisons of k_lmer_weights made once for all models, the
 *                          hits compacted into an LDS list and resolved with the lanes across models into an accumulator
 *                          tile in LDS (k_panel_weights), gkmhip_panel_weights
 *   gkm_regions.hip        regions of a scan: thresholded runs of windows with peak and summit, a prefix count of flagged
 *                          words, a segmented reduction and a compaction across launches (k_regions_word_sums,
 *                          k_regions_scan_words, k_regions_word_prefix, k_regions_summaries, k_regions_scan,
 *                          k_regions_fill), gkmhip_regions_count, gkmhip_regions_fill, gkmhip_regions_scratch_bytes,
 *                          gkmhip_regions_span
 *   gkm_wordcnt.h          the prefix count of flagged l-mer words (k_regions_word_sums, k_regions_scan_words,
 *                          k_regions_word_prefix) that gkm_regions.hip and gkm_dist.hip both launch
 *   gkm_dist.hip           the distribution of a scan's scores: histograms of the scored windows by a digit of an
 *                          order-preserving key or by edges, and a bounded collection of the scores under key prefixes
 *                          (k_dist_digits, k_dist_edges, k_dist_collect), gkmhip_dist_digits, gkmhip_dist_edges,
 *                          gkmhip_dist_collect, gkmhip_dist_scratch_bytes, gkmhip_dist_digit_bits
 *   gkm_wsim.hip           the kernel between every window of one long sequence and every window of another: tiles of
 *                          window pairs whose l-mer pairs are compared once, a difference array per mismatch class, the
 *                          normalisation by the windows' norms, the best column of every row (k_wsim_profiles,
 *                          k_wsim_normalize, k_wsim_best), gkmhip_wsim_profiles, gkmhip_wsim_normalize, gkmhip_wsim_best,
 *                          gkmhip_wsim_group
 *   gkm_walign.hip         the best local path through a block of that matrix: Smith-Waterman in doubles, one wave per
 *                          tile and one launch per tile anti-diagonal, the edges carried in place, the best cell by
 *                          shuffles, the traceback through squares of direction bytes staged in LDS (k_walign_init,
 *                          k_walign_tiles, k_walign_best, k_walign_trace), gkmhip_walign_block, gkmhip_walign_trace,
 *                          gkmhip_walign_tile, gkmhip_walign_scratch_bytes
 *   gkm_contract.hip       a weight table or panel contracted with position weight windows, one fixed order of rounded
 *                          operations: tiles of 4^6 codes, 16 weights per lane and the levels across lanes through LDS,
 *                          or the lanes across models and a serial walk, then a fold launch over the tiles' partials
 *                          (k_lmer_contract, k_panel_contract, k_contract_fold), gkmhip_lmer_contract,
 *                          gkmhip_panel_contract, gkmhip_contract_max_windows, gkmhip_contract_scratch_bytes
 *   gkm_knn.hip            what is kept of a block of kernel values: the best columns of every row merged into a running
 *                          list under a total order, one wave per row and one entry per lane, and the cells at or above a
 *                          threshold counted and listed by ballots (k_knn_merge, k_pairs_count, k_pairs_fill),
 *                          gkmhip_knn_merge, gkmhip_pairs_count, gkmhip_pairs_fill; needs no context
 */
#ifndef GKM_INTERNAL_H
#define GKM_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/gkm_hip.h"
#include "gkm_bitslice.h"
#include "gkm_pack.h"

#define GKM_MAXD1 13 /* d <= 12 */
#define GKM_MAXLEN 2047 /* longest sequence (the reference truncates there: libgkm.h:29-34, libgkm.c:1286-1291) */
#define GKM_SCRATCH_SLOTS 2 /* per-launch scratch sets of a context (gkmhip_set_scratch_slot) */

/* ------------------------------------------------------------------ errors (gkm_context.hip) */
int gkm_set_err(const char *what, hipError_t e, const char *file, int line);
int gkm_set_err_msg(const std::string &m, int code);
#define set_err gkm_set_err
#define set_err_msg gkm_set_err_msg
#define HIPCHK(expr)                                                        \
    do {                                                                    \
        hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) return set_err(#expr, e_, __FILE__, __LINE__); \
    } while (0)

/* --------------------------------------------------------- pinned host pools (gkm_context.hip) */
constexpr int STAGE_SLOTS = 16; /* one pair of staging buffers per concurrently copying device thread */
int acquire_staging(size_t want, double **out, int slot);
struct PinBuf {
    char *p = nullptr;
    size_t cap = 0;
    std::atomic<int> in_use{0};
};
PinBuf *pin_acquire(size_t bytes);
void pin_release(void *ud);
void gkm_release_pipe_streams(); /* (the copy-out pipeline's cached streams, gkm_copyout.hip) */

/* ----------------------------------------------------------------- context */
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    /* headroom: per-launch scratch whose size drifts from launch to launch (the row blocks of the boundary
     * call) is allocated half as big again, because growing means hipFree, and hipFree waits for the device */
    int ensure(size_t count, bool headroom = false)
    {
        if (count <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(headroom ? count + count / 2 : count, 1);
        HIPCHK(hipMalloc((void **)&p, want * sizeof(T)));
        cap = want;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct gkmhip_ctx {
    int device = 0;
    int L = 0, d = 0, rbf = 0, kernel_pref = GKMHIP_KERNEL_AUTO;
    double c[GKM_MAXD1] = {0};
    double gamma = 1.0;
    int n = 0, weighted = 0, maxlen = 0, minlen = 0;
    std::vector<int> h_len;
    std::vector<int64_t> h_lmoff;
    std::vector<double> h_cum_n; /* prefix sums of n_j = len_j - L + 1 */
    DevBuf<uint8_t> codes, wd; /* wd: distance-indexed positional weights */
    int wd_len = 0;
    DevBuf<uint32_t> wdc; /* the same weights CENTRED (byte wdc_centre + s = wd[|s|]): the row side of the several-pieces group variants */
    int wdc_words = 0, wdc_centre = 0;
    DevBuf<int64_t> off, lmoff;
    DevBuf<int> len;
    DevBuf<uint32_t> lmf, sb; /* lmf: forward l-mer table, then the reverse-strand table (general kernel only) */
    DevBuf<uint32_t> colpk;   /* 2-bit packed strands [seq][pkw][strand], the two strands interleaved word by word
                               * (k_pack_strands; gkm_bitslice.h pk_word): the hit path's column side */
    int pkw = 0;
    bool have_colpk = false;
    DevBuf<uint32_t> postab;  /* [seq][ptw] positional weights with zero guard bands (k_build_postab): the hit path's column
                               * weights in the one-piece variants */
    int ptw = 0;
    bool have_postab = false;
    uint32_t lm_stride = 0;
    int sb_xw = 0, sb_W = 0;
    bool have_lmers = false, have_sb = false;
    /* per-call scratch, two sets (gkmhip_set_scratch_slot): a caller that alternates launches between
     * two streams alternates the slot, so a launch never rewrites what the previous one still reads */
    struct Scratch {
        DevBuf<int> rows;
        DevBuf<int64_t> rowoff;    /* packed row offsets (general kernel only; the bit-sliced one has them in `tables`) */
        DevBuf<char> tables;       /* all per-launch tables of the bit-sliced kernel, one upload */
        DevBuf<uint32_t> rowplanes, rowpk;
        DevBuf<double> S;          /* tile-transposed raw values (k_gram_bitslice -> k_untile) */
        void release()
        {
            rows.release(); rowoff.release(); tables.release(); rowplanes.release(); rowpk.release(); S.release();
        }
    } scratch[GKM_SCRATCH_SLOTS];
    int sel = 0;
    DevBuf<double> sq;
    hipEvent_t ev0 = nullptr, ev1 = nullptr; /* around the Gram kernel of the most recent launch */
    bool ev_valid = false;
    /* gkmhip_kernel_timeline: while on, every launch records its own pair of events (no host wait in between), so
     * that a caller can time a loop of launches from outside and read the kernels' share of it afterwards */
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tl_pairs;
    size_t tl_used = 0;
    bool tl_on = false;
    hipEvent_t last_e0 = nullptr, last_e1 = nullptr;
    double sampled_hit_share = -1.0; /* share of sampled l-mer pairs of THESE sequences within d mismatches (set_sequences) */
    double last_comparisons = 0;
    const char *last_kernel = "none";
    int last_riders = 0; /* rows the most recent Gram launch carried as riders (gkm_pack.h RIDER_B0) */
    int last_variant = 0; /* k_gram_bitslice's PK of the most recent Gram launch (1, 2, 4, 5, 6, 7), 0: k_gram_direct */
    /* gkmhip_explain_block, gkmhip_ism_block, gkmhip_hyp_block: the row list of the call (upload_rows) and the partial
     * rows of its support-vector chunks.  One buffer each for all three: a call's kernels consume them in stream order
     * before the next call on that stream can overwrite them (growing one is a hipFree, which waits for the device). */
    DevBuf<int> blk_rows;
    DevBuf<double> blk_part;
    /* gkmhip_ism_block, gkmhip_ism_rbf_block: the per-tile G (RBF: the query's own decision sum) of its chunks;
     * gkmhip_ism_self_profiles: the queries' own profiles P_m(x, x) */
    DevBuf<double> ism_gpart;
    DevBuf<int64_t> ism_pself;
    /* gkmhip_delta_variants: the alternate bases of the call (its variant table goes through upload_rows) */
    DevBuf<uint8_t> delta_alt;
    /* gkmhip_lmer_contract, gkmhip_panel_contract: the tiles' partials, consumed by the call's own fold launch */
    DevBuf<double> contract_part;
};

/* the pair of events the next timed kernel is bracketed by (gkm_context.hip; the Gram launches call it themselves) */
int gkm_launch_events(gkmhip_ctx *ctx, hipEvent_t *e0, hipEvent_t *e1);

/* The bracket of a timed launch (gkm_context.hip), in this order; each but the last returns an error code or 0.
 *   enter  the context's device; the sticky error discarded
 *   begin  the launch's pair of events taken (the context's own, or the kernel timeline's next), the first recorded
 *   stop   the launch error checked, the second event recorded: what lies between begin and stop is what
 *          gkmhip_last_kernel_ms and the timeline report
 *   done   once everything has succeeded: the name and the comparisons of the launch, its events valid */
int gkm_launch_enter(gkmhip_ctx *ctx);
int gkm_launch_begin(gkmhip_ctx *ctx, hipStream_t stream);
int gkm_launch_stop(gkmhip_ctx *ctx, hipStream_t stream);
void gkm_launch_done(gkmhip_ctx *ctx, const char *kernel, double comparisons);

constexpr int WD_LDS = 1024; /* distance weight table entries: >= max |n/2 - p| + 1 for n <= 2047 */

/* per-sequence device tables (gkm_context.hip): built by gkmhip_set_sequences, complete before any launch */
/* (wait: the table is complete on return, so that a launch on ANOTHER stream may read it -- what a launch that finds the
 * table missing needs; gkmhip_set_sequences builds all of them and waits once) */
int ensure_lmers(gkmhip_ctx *ctx, hipStream_t stream, bool wait = true);
int ensure_colpk(gkmhip_ctx *ctx, hipStream_t stream, bool wait = true);
int ensure_postab(gkmhip_ctx *ctx, hipStream_t stream, bool wait = true);
int ensure_sb(gkmhip_ctx *ctx, int W, hipStream_t stream, bool wait = true);
bool bitslice_serves(const gkmhip_ctx *ctx); /* which kernel this context's launches take (gkm_gram.hip) */

/* the prologue of a launch over (row list) x (column range) (gkm_context.hip) */
/* 0 <= col_begin < col_end <= n of the uploaded set, or error 2 with `what` (the entry point) in front */
int check_range(const gkmhip_ctx *ctx, int col_begin, int col_end, const char *what);
/* rows: strictly ascending sequence indices, or error 2; *row_lmers: the l-mers of those sequences */
int check_rows(const gkmhip_ctx *ctx, const int *rows, int nrows, double *row_lmers);
/* the longest sequence of a column range and the bases of all of them */
void scan_range(const gkmhip_ctx *ctx, int col_begin, int col_end, int *tmax, int64_t *bases);
/* rows -> ctx->blk_rows, complete on return */
int upload_rows(gkmhip_ctx *ctx, const int *rows, int nrows, hipStream_t stream);

/* what the launches over l-mer words share across files; `what`: the entry point, in front of every message */
/* the windows of a scan launch (gkm_scan.hip): width - L + 1, or a negative value after set_err_msg */
int scan_check(const gkmhip_ctx *ctx, const void *lm, int64_t nlm, const void *wt, int width, int stride, int64_t nwin,
               const void *out, const char *what);
/* a panel's pointer, models and row stride (gkm_panel.hip): 0 or error 2; log2 of nm rounded up to 8, 16, 32 or 64 */
int panel_check(const void *P, int nm, int ms, const char *what);
int panel_shift(int nm);

/* ------------------------------------------------------------ what a Gram launch writes */
struct GramOut {
    double *G;      /* raw values G(a,j); may be NULL when only `diag` is wanted */
    int64_t ld;
    int32_t *P;
    int64_t ldp;
    int local_rows;
    int write_all;  /* 0: only j <= a (lower triangle + diagonal); 1: every column visited */
    double *diag;   /* if set: diag[a] = G(a,a) */
    /* if set (packed row slabs, gkm_shard.h): local row r starts at G + row_off[r] instead of G + r * ld.
     * gram_launch() receives the HOST array and replaces it by its device copy. */
    const int64_t *row_off;
    /* the column that lands at offset 0 of a row: col_begin of a COLS_RANGE launch, 0 for every other mode */
    int col0;
};

__device__ __forceinline__ double *gram_cell(const GramOut &out, int64_t r, int j)
{
    return out.G + (out.row_off ? out.row_off[r] : r * out.ld) + (j - out.col0);
}

/* which columns a tile of rows visits */
enum { COLS_TRIANGLE = 0, COLS_FULL = 1, COLS_DIAGONAL = 2, COLS_RANGE = 3 /* [col_begin, col_end) of the launch */ };

/* rows r0..r1-1 of a matrix whose rows < r1 hold raw values (gkm_normalize.hip) */
int normalize_rows(gkmhip_ctx *ctx, double *G, int64_t ld, int r0, int r1, double *sq, int symmetric, hipStream_t stream,
                   bool have_norms = false);

#endif
