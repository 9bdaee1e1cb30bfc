/*
 * gkm_walign.hip -- the best local path through a windowed kernel matrix: Smith-Waterman with a linear
 * gap penalty, in doubles, over a block of gkmhip_wsim_profiles + gkmhip_wsim_normalize's K, and the traceback, both on
 * the device.  In DP coordinates (i, c) -- i the window of x, c = j forward, c = nwy - 1 - j with `flip` --
 *
 *   v = K(i, j(c));  h = 0.0, dir = STOP(0)
 *   if v == v:  t = H(i-1, c-1) + (v - offset);  if t > h: h = t, dir = DIAG(1)
 *   t = H(i-1, c) - gap;                         if t > h: h = t, dir = UP(2)
 *   t = H(i, c-1) - gap;                         if t > h: h = t, dir = LEFT(3)
 *   H(i, c) = h;  D(i, c) = dir
 *
 * Every H is a max of fixed expressions of one subtraction and one addition (no contraction: -ffp-contract=off), so its
 * bits do not depend on the order in which cells are evaluated or on how the matrix is cut into blocks and tiles.  The
 * best cell is the largest H, the lower i and then the lower c on a tie: a total order, exact and associative.
 *
 * Kernels
 *   k_walign_init   saves what the tiles of the first tile row and column need as H(i0-1, c0-1) -- cells of `top` and
 *                   `left` that other tiles overwrite before they run -- into the per-tile corner array.
 *   k_walign_tiles  HOT.  One wave per tile of WA_R rows by WA_C columns, one launch per tile anti-diagonal: tile (I, J)
 *                   needs (I-1, J) and (I, J-1), which the launch before finished.  Lane r owns row r and computes column
 *                   t - r at step t: "left" is its own previous value, "up" lane r-1's previous value by a DPP shift of the
 *                   wave, "diag" the "up" of one step earlier; lane 0 reads `top`, column 0 reads `left` and the corner.  K
 *                   and `top` are read WA_G columns ahead into registers, the direction bytes of WA_G columns leave as one
 *                   qword; the step itself holds no branch and no memory operation.
 *                   The tile overwrites its columns of `top` (its last row) and its rows of `left` (its last column) in
 *                   place -- each cell read before it is written -- and writes its bottom-right H to the corner array and
 *                   its best cell, reduced by shuffles, to a record.  No LDS, no barrier, no atomics; no workgroup waits
 *                   for another.
 *   k_walign_best   one wave: the tile records -> the block's best cell.
 *   k_walign_trace  one wave: walks D back from the end cell.  The 64 x 64 direction bytes up-left of the current cell
 *                   are staged in LDS by coalesced loads and walked there; every step lowers i + c, so at most
 *                   nwx + nwy steps are made whatever D holds.
 */
#include "gkm_internal.h"

namespace {

constexpr int WA_R = 64;  /* rows of a tile: one per lane */
constexpr int WA_C = 128; /* columns of a tile: a launch costs about 52 steps, so WA_C + 63 steps per launch over
                           * tiles_x + tiles_y - 1 launches is least near 128 at 5 000 x 5 000 cells */
constexpr int WA_G = 8;   /* columns a lane reads ahead and whose direction bytes it stores at once */
constexpr int WT_S = 64;  /* side of the square of direction bytes the trace stages */
constexpr int64_t WA_MAXW = (int64_t)1 << 20;

struct WaRec {
    double h;
    int64_t i, c;
};

/* (h, i, c) replaces (bh, bi, bc): a larger H, or the same positive H at a lower i, then a lower c.  No cell is (0.0, -1,
 * -1); a zero H never replaces it. */
__device__ __forceinline__ bool wa_better(double h, int64_t i, int64_t c, double bh, int64_t bi, int64_t bc)
{
    return h > bh || (h == bh && h > 0.0 && (i < bi || (i == bi && c < bc)));
}

__device__ __forceinline__ void wa_reduce(double &bh, int64_t &bi, int64_t &bc)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oh = __shfl_xor(bh, o, 64);
        const int64_t oi = (int64_t)__shfl_xor((long long)bi, o, 64), oc = (int64_t)__shfl_xor((long long)bc, o, 64);
        if (wa_better(oh, oi, oc, bh, bi, bc)) {
            bh = oh;
            bi = oi;
            bc = oc;
        }
    }
}

/* corners: [tiles_x + 1][tiles_y + 1], entry (I, J) = H(I WA_R - 1, J WA_C - 1) of the block */
__global__ __launch_bounds__(256) void k_walign_init(const double *top, const double *left, const double *corner,
                                                     double *corners, int tiles_x, int tiles_y)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0) corners[0] = *corner;
    else if (e < tiles_y) corners[e] = top[(int64_t)e * WA_C - 1];
    else if (e > tiles_y && e - tiles_y < tiles_x) corners[(int64_t)(e - tiles_y) * (tiles_y + 1)] = left[(int64_t)(e - tiles_y) * WA_R - 1];
}

/* lane r <- lane r - 1's `own` (the wave shifted right by one lane, a DPP move per half: no LDS round trip); lane 0,
 * which has no lane below it, keeps `edge` */
__device__ __forceinline__ double wa_from_above(double own, double edge)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(own), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(own), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

/* the tiles (I, J) with I + J = diag, I = i_first + blockIdx.x.  top, left: read and written in place (not restrict).
 * The step is free of branches and of memory operations: what a group of WA_G steps produced -- the direction bytes, and
 * in the tile's last row the H of `top` -- leaves at the start of the next group, before that group's read-ahead is
 * issued, so that waiting for the read-ahead never waits for a store just made. */
__global__ __launch_bounds__(64) void k_walign_tiles(const double *__restrict__ K, int64_t ld, int nwx, int nwy, int flip,
                                                     double offset, double gap, double *top, double *left,
                                                     uint8_t *__restrict__ D, int64_t ldd, double *corners, WaRec *__restrict__ rec,
                                                     int tiles_y, int diag, int i_first)
{
    const int lane = threadIdx.x;
    const int I = i_first + (int)blockIdx.x, J = diag - I;
    const int i0 = I * WA_R, c0 = J * WA_C;
    const int nr = min(WA_R, nwx - i0), nc = min(WA_C, nwy - c0);
    const bool row = lane < nr;
    const int ncl = row ? nc : 0; /* the lane's columns: local column cl is the lane's iff (unsigned)cl < ncl */
    const int64_t i = i0 + lane;
    const double *Krow = K + i * ld;
    uint8_t *Drow = D ? D + i * ldd : nullptr;
    double hl = row ? left[i] : 0.0;                                            /* H(i, c - 1): the lane's own latest value */
    double dg = wa_from_above(hl, corners[(int64_t)I * (tiles_y + 1) + J]);     /* H(i - 1, c - 1) */
    double bh = 0.0;
    int bc = -1;
    double kn[WA_G], tn[WA_G], kc[WA_G], tc[WA_G], hs[WA_G];
    uint32_t qlo = 0, qhi = 0;

#define WA_LOAD(T0)                                                                        \
    _Pragma("unroll") for (int s = 0; s < WA_G; s++) {                                     \
        const int cl = (T0) + s - lane;                                                    \
        const bool ok = (unsigned)cl < (unsigned)ncl;                                      \
        const int c = c0 + cl;                                                             \
        kn[s] = ok ? Krow[flip ? nwy - 1 - c : c] : 0.0;                                   \
        tn[s] = ok && lane == 0 ? top[c] : 0.0;                                            \
    }
#define WA_STORE(T0)                                                                       \
    {                                                                                      \
        const int cl0 = (T0) - lane;                                                       \
        if (Drow) {                                                                        \
            if (cl0 >= 0 && cl0 + WA_G <= ncl) {                                           \
                const uint64_t q = (uint64_t)qhi << 32 | qlo;                              \
                __builtin_memcpy(Drow + c0 + cl0, &q, 8); /* (any alignment) */            \
            } else {                                                                       \
                _Pragma("unroll") for (int s = 0; s < WA_G; s++)                           \
                    if ((unsigned)(cl0 + s) < (unsigned)ncl)                               \
                        Drow[c0 + cl0 + s] = (uint8_t)((s < 4 ? qlo : qhi) >> (8 * (s & 3))); \
            }                                                                              \
        }                                                                                  \
        if (lane == nr - 1) {                                                              \
            _Pragma("unroll") for (int s = 0; s < WA_G; s++)                               \
                if ((unsigned)(cl0 + s) < (unsigned)ncl) top[c0 + cl0 + s] = hs[s];        \
        }                                                                                  \
    }

    const int steps = nc + nr - 1;
    int t0 = 0;
    WA_LOAD(0)
    for (; t0 < steps; t0 += WA_G) {
#pragma unroll
        for (int s = 0; s < WA_G; s++) {
            kc[s] = kn[s];
            tc[s] = tn[s];
        }
        if (t0 > 0) WA_STORE(t0 - WA_G)
        if (t0 + WA_G < steps) {
            WA_LOAD(t0 + WA_G)
        }
        qlo = qhi = 0;
        const int base = t0 - lane;
#pragma unroll
        for (int s = 0; s < WA_G; s++) {
            const int cl = base + s;
            const bool act = (unsigned)cl < (unsigned)ncl;
            const double up = wa_from_above(hl, tc[s]); /* lane r-1's value of the step before, or top: H(i - 1, c) */
            double h = 0.0;
            uint32_t dir = 0;
            const double t1 = dg + (kc[s] - offset); /* a NaN K makes t1 a NaN, which is not > h: no test of its own */
            if (t1 > h) {
                h = t1;
                dir = 1;
            }
            const double t2 = up - gap;
            if (t2 > h) {
                h = t2;
                dir = 2;
            }
            const double t3 = hl - gap;
            if (t3 > h) {
                h = t3;
                dir = 3;
            }
            hs[s] = h;
            if (s < 4) qlo |= dir << (8 * (s & 3));
            else qhi |= dir << (8 * (s & 3));
            const bool gt = act && h > bh; /* ascending c within the lane's row: the lowest c of the largest H */
            bh = gt ? h : bh;
            bc = gt ? cl : bc;
            hl = act ? h : hl;
            dg = act ? up : dg;
        }
    }
    WA_STORE(t0 - WA_G)
#undef WA_LOAD
#undef WA_STORE
    if (row) left[i] = hl; /* the lane's last column: H(i, c0 + nc - 1) */
    if (lane == nr - 1) corners[(int64_t)(I + 1) * (tiles_y + 1) + (J + 1)] = hl;
    int64_t bi = bc >= 0 ? i : -1, bcc = bc >= 0 ? c0 + bc : -1;
    wa_reduce(bh, bi, bcc);
    if (lane == 0) {
        WaRec r;
        r.h = bh;
        r.i = bi;
        r.c = bcc;
        rec[(int64_t)I * tiles_y + J] = r;
    }
}

__global__ __launch_bounds__(64) void k_walign_best(const WaRec *__restrict__ rec, int64_t nrec, double *__restrict__ best_h,
                                                    int64_t *__restrict__ best_ic)
{
    double bh = 0.0;
    int64_t bi = -1, bc = -1;
    for (int64_t e = threadIdx.x; e < nrec; e += 64) {
        const WaRec r = rec[e];
        if (wa_better(r.h, r.i, r.c, bh, bi, bc)) {
            bh = r.h;
            bi = r.i;
            bc = r.c;
        }
    }
    wa_reduce(bh, bi, bc);
    if (threadIdx.x == 0) {
        best_h[0] = bh;
        best_ic[0] = bi;
        best_ic[1] = bc;
    }
}

__global__ __launch_bounds__(64) void k_walign_trace(const uint8_t *__restrict__ D, int64_t ldd, int64_t end_i, int64_t end_c,
                                                     int32_t *__restrict__ path, int64_t capacity, int64_t *__restrict__ count)
{
    __shared__ uint8_t sq[WT_S * WT_S];
    const int lane = threadIdx.x;
    int64_t i = end_i, c = end_c, n = 0;
    bool stop = false;
    while (!stop && i >= 0 && c >= 0) { /* one turn per staged square; the cell (i, c) lies in it, so every turn steps */
        const int64_t bi = max(i - (WT_S - 1), (int64_t)0), bc = max(c - (WT_S - 1), (int64_t)0);
        const int rows = (int)(i - bi) + 1, cols = (int)(c - bc) + 1;
        for (int r = 0; r < rows; r++)
            if (lane < cols) sq[r * WT_S + lane] = D[(bi + r) * ldd + bc + lane];
        __syncthreads();
        while (i >= bi && c >= bc) {
            const int dir = __builtin_amdgcn_readfirstlane((int)sq[(int)(i - bi) * WT_S + (int)(c - bc)]);
            if (dir == 1) {
                if (lane == 0 && n < capacity) {
                    path[2 * n] = (int32_t)i;
                    path[2 * n + 1] = (int32_t)c;
                }
                n++;
                i--;
                c--;
            } else if (dir == 2) {
                i--;
            } else if (dir == 3) {
                c--;
            } else { /* STOP, and any other byte: a corrupt D ends the walk */
                stop = true;
                break;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        count[0] = n;
        count[1] = i;
        count[2] = c;
    }
}

inline void walign_tiles(int64_t nwx, int64_t nwy, int64_t *tx, int64_t *ty)
{
    *tx = (nwx + WA_R - 1) / WA_R;
    *ty = (nwy + WA_C - 1) / WA_C;
}

inline bool walign_shape(int64_t nwx, int64_t nwy) { return nwx >= 1 && nwy >= 1 && nwx <= WA_MAXW && nwy <= WA_MAXW; }

} /* namespace */

extern "C" int gkmhip_walign_tile(int *rows, int *cols)
{
    if (!rows || !cols) return 2;
    *rows = WA_R;
    *cols = WA_C;
    return 0;
}

extern "C" int64_t gkmhip_walign_scratch_bytes(int64_t nwx, int64_t nwy)
{
    if (!walign_shape(nwx, nwy)) return -1;
    int64_t tx, ty;
    walign_tiles(nwx, nwy, &tx, &ty);
    return (tx + 1) * (ty + 1) * (int64_t)sizeof(double) + tx * ty * (int64_t)sizeof(WaRec);
}

extern "C" int gkmhip_walign_block(gkmhip_ctx *ctx, const double *K, int64_t ld, int64_t nwx, int64_t nwy, int flip, double offset,
                                   double gap, double *top, double *left, const double *corner, uint8_t *D, int64_t ldd,
                                   double *best_h, int64_t *best_ic, void *scratch, int64_t scratch_bytes, void *stream_)
{
    const char *what = "gkmhip_walign_block";
    if (!ctx || !K || !top || !left || !corner || !best_h || !best_ic || !scratch)
        return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (!walign_shape(nwx, nwy)) return set_err_msg(std::string(what) + ": needs 1..2^20 windows on each axis", 2);
    if (ld < nwy || ldd < nwy) return set_err_msg(std::string(what) + ": leading dimension too small", 2);
    if (!std::isfinite(offset) || !std::isfinite(gap) || gap < 0)
        return set_err_msg(std::string(what) + ": the offset must be finite and the gap penalty finite and not negative", 2);
    if (((uintptr_t)scratch & 7) || scratch_bytes < gkmhip_walign_scratch_bytes(nwx, nwy))
        return set_err_msg(std::string(what) + ": the scratch is too small or not 8-byte aligned", 2);
    int64_t tx, ty;
    walign_tiles(nwx, nwy, &tx, &ty);
    double *corners = (double *)scratch;
    WaRec *rec = (WaRec *)(corners + (tx + 1) * (ty + 1));
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_walign_init, dim3((unsigned)((tx + ty + 1 + 255) / 256)), dim3(256), 0, stream, top, left, corner, corners,
                       (int)tx, (int)ty);
    /* one launch per tile anti-diagonal, in stream order: no host wait, and no workgroup waits for another */
    for (int64_t s = 0; s < tx + ty - 1; s++) {
        const int64_t first = std::max<int64_t>(0, s - (ty - 1)), last = std::min<int64_t>(tx - 1, s);
        hipLaunchKernelGGL(k_walign_tiles, dim3((unsigned)(last - first + 1)), dim3(64), 0, stream, K, ld, (int)nwx, (int)nwy,
                           flip != 0, offset, gap, top, left, D, ldd, corners, rec, (int)ty, (int)s, (int)first);
    }
    hipLaunchKernelGGL(k_walign_best, dim3(1), dim3(64), 0, stream, rec, tx * ty, best_h, best_ic);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_walign_tiles", (double)nwx * (double)nwy); /* (cells) */
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: window alignment, %lld x %lld cells -> k_walign_tiles (%lld x %lld tiles of %d x %d, %lld launches)\n",
                (long long)nwx, (long long)nwy, (long long)tx, (long long)ty, WA_R, WA_C, (long long)(tx + ty - 1));
    return 0;
}

extern "C" int gkmhip_walign_trace(gkmhip_ctx *ctx, const uint8_t *D, int64_t ldd, int64_t nwx, int64_t nwy, int64_t end_i,
                                   int64_t end_c, int32_t *path, int64_t capacity, int64_t *count, void *stream_)
{
    const char *what = "gkmhip_walign_trace";
    if (!ctx || !D || !path || !count) return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (!walign_shape(nwx, nwy)) return set_err_msg(std::string(what) + ": needs 1..2^20 windows on each axis", 2);
    if (ldd < nwy) return set_err_msg(std::string(what) + ": leading dimension too small", 2);
    if (end_i < 0 || end_i >= nwx || end_c < 0 || end_c >= nwy)
        return set_err_msg(std::string(what) + ": the end cell lies outside the matrix", 2);
    if (capacity < std::min(nwx, nwy))
        return set_err_msg(std::string(what) + ": the path needs room for min(nwx, nwy) pairs", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_walign_trace, dim3(1), dim3(64), 0, stream, D, ldd, end_i, end_c, path, capacity, count);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_walign_trace", (double)(end_i + end_c + 2)); /* (the most steps the walk can make) */
    return 0;
}
