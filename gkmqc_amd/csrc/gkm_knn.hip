/*
 * gkm_knn.hip -- what is kept of a block of kernel values when the block itself is not wanted: the
 * kcap best columns of every row, and every cell at or above a threshold.  The block is any DEVICE matrix of doubles,
 * nrows x ncols with leading dimension ld: the output of gkmhip_gram_block + gkmhip_normalize_block in a block loop, or
 * a resident K.  No gkmhip_ctx, because no parameter of the gkm kernel family enters.
 *
 * Eligibility (all three kernels).  Column j of the block is the global column c = col_base + j.  Cell (i, j) is
 * eligible iff its value is not a NaN and c != row_id[i] (mode 0) or c > row_id[i] (mode 1, the upper triangle);
 * row_id[i] = -1: the row has no column of its own.
 *
 * The order.  Entry (v, c) stands before (w, e) iff v > w, or v == w and c < e (-0.0 == 0.0; the cell's own bits are
 * kept).  No two eligible cells of a row share a column, so this is a strict total order, and the kcap first of a set
 * under it do not depend on how the set is cut or in which order its parts arrive: after every column block has been
 * merged once, a row's list holds the same bytes whatever the cut into column blocks and whatever their order.
 *
 * Kernels (one wave per row each; no LDS, no atomics, no barrier, no workgroup waits for another)
 *   k_knn_merge    lane l holds entry l of the row's list.  Per 64 columns one coalesced read, then the ballot of the
 *                  eligible cells that stand before the list's last entry (read with a readlane).  Per set bit, lowest
 *                  first: the candidate is read from its lane, compared against the last entry once more (earlier
 *                  insertions of the same 64 may have moved it), its rank is the population count of the ballot "my
 *                  entry stands before the candidate", the entries from the rank on move one lane up by a wave-shift
 *                  DPP move and the lane of the rank takes the candidate.  An unfilled entry is (idx -1, NaN) and
 *                  stands behind every cell.
 *   k_pairs_count  count[i] = the eligible cells of row i with a value >= threshold: population counts of ballots
 *   k_pairs_fill   row i writes those cells in ascending column from offset[i] on: the slot of a cell is the row's
 *                  offset, the passing cells of the 64s before it and the population count of its 64's ballot below
 *                  its lane.  Slots at or beyond capacity are not written.
 *
 * Timing: like the gkm_nullidx.hip calls these keep no events (there is no context to keep them in); a caller that
 * wants the kernels' time brackets the call with events of its own on the stream it passes.
 */
#include "gkm_internal.h"

namespace {

constexpr int KN_THREADS = 256;
constexpr int KN_ROWS = KN_THREADS / 64; /* rows (waves) per workgroup */
constexpr int KN_MAXK = 64;

__device__ __forceinline__ int kn_below(unsigned long long m) /* set bits of m below this lane */
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ double kn_readlane(double v, int lane) /* lane: the same in every lane */
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

/* lane r <- lane r - 1's value (the wave shifted right by one lane, a DPP move per half); lane 0 keeps its own */
__device__ __forceinline__ double kn_from_below(double own)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(own), __double2loint(own), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(own), __double2hiint(own), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int kn_from_below(int own)
{
    return __builtin_amdgcn_update_dpp(own, own, 0x138, 0xf, 0xf, false);
}

/* (v, c), a cell (v not a NaN, c >= 0), stands before the entry (w, e); e < 0: the entry is unfilled */
__device__ __forceinline__ bool kn_cell_before(double v, int c, double w, int e)
{
    return e < 0 || v > w || (v == w && c < e);
}

__device__ __forceinline__ bool kn_eligible(double v, int c, int rid, int mode)
{
    return v == v && (mode ? c > rid : c != rid);
}

__global__ __launch_bounds__(KN_THREADS) void k_knn_merge(const double *__restrict__ K, int64_t ld, int nrows, int ncols,
                                                          const int32_t *__restrict__ row_id, int col_base, int mode,
                                                          int kcap, int32_t *__restrict__ best_idx,
                                                          double *__restrict__ best_val)
{
    const int lane = threadIdx.x & 63;
    const int i = (int)(((int64_t)blockIdx.x * KN_THREADS + threadIdx.x) >> 6); /* the same in every lane of a wave */
    if (i >= nrows) return;
    const int rid = row_id[i];
    const double *row = K + (int64_t)i * ld;
    const bool mine = lane < kcap;
    const int64_t slot = (int64_t)i * kcap + lane;
    int ei = mine ? best_idx[slot] : -1;
    double ev = mine ? best_val[slot] : 0.0;
    const int last = kcap - 1;
    int ti = __builtin_amdgcn_readlane(ei, last);
    double tv = kn_readlane(ev, last);
    bool changed = false;
    for (int j0 = 0; j0 < ncols; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < ncols;
        const double v = in ? row[j] : 0.0;
        const int c = col_base + j;
        unsigned long long m = __ballot(in && kn_eligible(v, c, rid, mode) && kn_cell_before(v, c, tv, ti));
        while (m) { /* (m is the same in every lane: the whole wave walks the loop together) */
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const double cv = kn_readlane(v, b);
            const int cc = col_base + j0 + b;
            if (!kn_cell_before(cv, cc, tv, ti)) continue;
            /* the entries that stand before the candidate are a prefix of the list: their number is its rank */
            const bool before = mine && ei >= 0 && !kn_cell_before(cv, cc, ev, ei);
            const int rank = __popcll(__ballot(before));
            const double sv = kn_from_below(ev);
            const int si = kn_from_below(ei);
            if (mine && lane > rank) {
                ev = sv;
                ei = si;
            } else if (lane == rank) { /* (rank < kcap: the candidate stands before the last entry) */
                ev = cv;
                ei = cc;
            }
            ti = __builtin_amdgcn_readlane(ei, last);
            tv = kn_readlane(ev, last);
            changed = true;
        }
    }
    if (changed && mine) {
        best_idx[slot] = ei;
        best_val[slot] = ev;
    }
}

__global__ __launch_bounds__(KN_THREADS) void k_pairs_count(const double *__restrict__ K, int64_t ld, int nrows, int ncols,
                                                            const int32_t *__restrict__ row_id, int col_base, int mode,
                                                            double threshold, int64_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int i = (int)(((int64_t)blockIdx.x * KN_THREADS + threadIdx.x) >> 6);
    if (i >= nrows) return;
    const int rid = row_id[i];
    const double *row = K + (int64_t)i * ld;
    int64_t n = 0;
    for (int j0 = 0; j0 < ncols; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < ncols;
        const double v = in ? row[j] : 0.0;
        n += __popcll(__ballot(in && kn_eligible(v, col_base + j, rid, mode) && v >= threshold));
    }
    if (lane == 0) count[i] = n;
}

__global__ __launch_bounds__(KN_THREADS) void k_pairs_fill(const double *__restrict__ K, int64_t ld, int nrows, int ncols,
                                                           const int32_t *__restrict__ row_id, int col_base, int mode,
                                                           double threshold, const int64_t *__restrict__ offset,
                                                           int64_t capacity, int32_t *__restrict__ out_i,
                                                           int32_t *__restrict__ out_j, double *__restrict__ out_v)
{
    const int lane = threadIdx.x & 63;
    const int i = (int)(((int64_t)blockIdx.x * KN_THREADS + threadIdx.x) >> 6);
    if (i >= nrows) return;
    const int rid = row_id[i];
    const double *row = K + (int64_t)i * ld;
    int64_t at = offset[i];
    if (at < 0) return; /* (no slot lies below 0) */
    for (int j0 = 0; j0 < ncols && at < capacity; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < ncols;
        const double v = in ? row[j] : 0.0;
        const int c = col_base + j;
        const bool pass = in && kn_eligible(v, c, rid, mode) && v >= threshold;
        const unsigned long long m = __ballot(pass);
        const int64_t dst = at + kn_below(m);
        if (pass && dst < capacity) {
            out_i[dst] = rid;
            out_j[dst] = c;
            out_v[dst] = v;
        }
        at += __popcll(m);
    }
}

/* 0, or error 2 after set_err_msg: what the three entry points share */
int knn_check(const void *K, int64_t ld, int64_t nrows, int64_t ncols, const void *row_id, int64_t col_base, int mode,
              const char *what)
{
    const std::string w(what);
    if (!K || !row_id) return set_err_msg(w + ": a NULL pointer", 2);
    if (nrows < 0 || ncols < 0) return set_err_msg(w + ": nrows and ncols must not be negative", 2);
    if (nrows > 0x7FFFFFFFLL / 64) return set_err_msg(w + ": at most 2^25 - 1 rows per call", 2);
    if (ld < ncols) return set_err_msg(w + ": ld must be at least ncols", 2);
    if (col_base < 0 || col_base + ncols > 0x7FFFFFFFLL) return set_err_msg(w + ": the global columns must lie in 0..2^31 - 2", 2);
    if (mode != 0 && mode != 1) return set_err_msg(w + ": mode must be 0 (all but the own column) or 1 (upper triangle)", 2);
    return 0;
}

inline unsigned knn_grid(int64_t nrows) { return (unsigned)((nrows + KN_ROWS - 1) / KN_ROWS); }

} /* namespace */

extern "C" int gkmhip_knn_merge(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                                int64_t col_base, int mode, int kcap, int32_t *best_idx, double *best_val, void *stream_)
{
    if (int rc = knn_check(K, ld, nrows, ncols, row_id, col_base, mode, "gkmhip_knn_merge")) return rc;
    if (!best_idx || !best_val) return set_err_msg("gkmhip_knn_merge: a NULL pointer", 2);
    if (kcap < 1 || kcap > KN_MAXK) return set_err_msg("gkmhip_knn_merge: kcap must lie in 1.." + std::to_string(KN_MAXK), 2);
    if (nrows == 0 || ncols == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_knn_merge, dim3(knn_grid(nrows)), dim3(KN_THREADS), 0, stream, K, ld, (int)nrows, (int)ncols, row_id,
                       (int)col_base, mode, kcap, best_idx, best_val);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gkmhip_pairs_count(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                                  int64_t col_base, int mode, double threshold, int64_t *count, void *stream_)
{
    if (int rc = knn_check(K, ld, nrows, ncols, row_id, col_base, mode, "gkmhip_pairs_count")) return rc;
    if (!count) return set_err_msg("gkmhip_pairs_count: a NULL pointer", 2);
    if (nrows == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pairs_count, dim3(knn_grid(nrows)), dim3(KN_THREADS), 0, stream, K, ld, (int)nrows, (int)ncols,
                       row_id, (int)col_base, mode, threshold, count);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gkmhip_pairs_fill(int device, const double *K, int64_t ld, int64_t nrows, int64_t ncols, const int32_t *row_id,
                                 int64_t col_base, int mode, double threshold, const int64_t *offset, int64_t capacity,
                                 int32_t *out_i, int32_t *out_j, double *out_v, void *stream_)
{
    if (int rc = knn_check(K, ld, nrows, ncols, row_id, col_base, mode, "gkmhip_pairs_fill")) return rc;
    if (!offset || !out_i || !out_j || !out_v) return set_err_msg("gkmhip_pairs_fill: a NULL pointer", 2);
    if (capacity < 0) return set_err_msg("gkmhip_pairs_fill: the capacity must not be negative", 2);
    if (nrows == 0 || ncols == 0 || capacity == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pairs_fill, dim3(knn_grid(nrows)), dim3(KN_THREADS), 0, stream, K, ld, (int)nrows, (int)ncols, row_id,
                       (int)col_base, mode, threshold, offset, capacity, out_i, out_j, out_v);
    HIPCHK(hipGetLastError());
    return 0;
}
