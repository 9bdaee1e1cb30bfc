/*
 * gkm_panel_fold.hip -- an l-mer weight panel folded in one pass: the weight tables of nm <= 64 models
 * that share the kernel parameters, written straight into the panel's device image,
 *
 *   P[(u - u_begin) * ms + m] = sum_i CV[i * ms + m] (c[m(u, v_i)] + c[m(u, rc(v_i))])      (c[.] = 0 beyond d)
 *
 * over the union v of the models' canonical classes; CV[i][m] is class i's coefficient for model m (0.0 where model m does
 * not hold the class).  The two-strand comparisons of a code against the classes, k_lmer_weights' whole cost, do not depend
 * on the model: they are made once, and only the multiply-add per hit is made per model.
 *
 * Kernel
 *   k_panel_weights  one wave per workgroup, 64 codes per wave.
 *                    COMPARE, lanes across codes: the classes stream through the wave as scalars, eight per request,
 *                    exactly as in k_lmer_weights.  A lane that hits (either strand within d) appends (its slot, the
 *                    class index, c[mf] + c[mr]) to a hit list in LDS: classes in ascending order, the lanes of one
 *                    class in lane order (a ballot and a prefix count give the position).
 *                    RESOLVE, lanes across models: the list front to back; per hit one coalesced read of the row
 *                    CV[i, :] and a read-modify-write of the row of the accumulator tile acc[slot][:] in LDS.  Lane m
 *                    touches column m only, and a wave's LDS operations complete in program order, so every (u, m) sees
 *                    its classes in ascending i: the order of k_lmer_weights' lane, hence its bits (each term a rounded
 *                    product, then a rounded add: -ffp-contract=off).
 *                    The list holds FOLD_CAP hits and is resolved whenever the next group of classes could overflow it
 *                    if every lane hit every class (L = 5, d = 3 does that), at the latest after the last class.
 *                    The tile, then, one contiguous block of the image, is stored with columns nm.. as +0.0.
 *
 * No atomics, no workgroup waits for another, and nothing depends on the launch geometry, nm, ms or the range: when the
 * list is resolved changes no order.  The accumulators live in LDS (MP columns per code, MP = nm rounded up to 8, 16, 32
 * or 64), never in a runtime-indexed per-lane array.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int FOLD_CODES = 64; /* codes per workgroup: one wave */
constexpr int FOLD_QB = 8;     /* classes per scalar request */
constexpr int FOLD_HALF = 4;   /* classes between two looks at the list's fill */
constexpr int FOLD_CAP = 512;  /* hits the list holds: two groups of FOLD_HALF classes hit by every lane */
constexpr int FOLD_RB = 8;     /* hits whose rows of CV are in flight together */

static_assert(FOLD_CAP >= 2 * FOLD_HALF * FOLD_CODES, "a group of classes must fit behind a list that was not resolved");

template <int MP>
struct FoldLds {
    double acc[FOLD_CODES * MP]; /* [slot][model] */
    double val[FOLD_CAP];        /* c[mf] + c[mr] of a hit */
    uint32_t cls[FOLD_CAP];      /* its class index */
    uint8_t slot[FOLD_CAP];      /* its code: u - the wave's first code */
    double cs[LMER_NC];
};

/* the hits [0, count) into the tile, front to back; lanes across models */
template <int MP>
__device__ __forceinline__ void fold_resolve(FoldLds<MP> &s, int count, const double *__restrict__ CV, int nm, int ms,
                                             int lane)
{
    __syncthreads(); /* (one wave: the list as the other lanes wrote it) */
    if (lane < nm) {
        int h = 0;
        for (; h + FOLD_RB <= count; h += FOLD_RB) {
            int sl[FOLD_RB];
            double x[FOLD_RB], w[FOLD_RB];
#pragma unroll
            for (int r = 0; r < FOLD_RB; r++) {
                sl[r] = s.slot[h + r];
                x[r] = s.val[h + r];
                w[r] = CV[(size_t)s.cls[h + r] * (size_t)ms + (size_t)lane];
            }
#pragma unroll
            for (int r = 0; r < FOLD_RB; r++) s.acc[sl[r] * MP + lane] += w[r] * x[r];
        }
        for (; h < count; h++)
            s.acc[(int)s.slot[h] * MP + lane] += CV[(size_t)s.cls[h] * (size_t)ms + (size_t)lane] * s.val[h];
    }
    __syncthreads(); /* (the list is free again) */
}

/* class i (code x) against this lane's code: the hitting lanes append to the list; -> the list's new fill */
template <int MP>
__device__ __forceinline__ int fold_compare(FoldLds<MP> &s, int count, uint32_t u, bool valid, uint32_t x, int i, int L,
                                            int d, int lane)
{
    const int mf = lmer_mm(u, x), mr = lmer_mm(u, lmer_rc(x, L));
    const bool hit = valid && min(mf, mr) <= d;
    const unsigned long long b = __ballot(hit);
    if (hit) {
        const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
        s.val[pos] = s.cs[mf] + s.cs[mr];
        s.cls[pos] = (uint32_t)i;
        s.slot[pos] = (uint8_t)lane;
    }
    return count + __popcll(b);
}

template <int MP>
__global__ __launch_bounds__(FOLD_CODES) void k_panel_weights(const uint32_t *v, const double *__restrict__ CV, int nv,
                                                              int nm, int ms, uint32_t u_begin, uint32_t u_end,
                                                              const LmerCoef C, int L, int d, double *__restrict__ P)
{
    __shared__ FoldLds<MP> s;
    const int lane = threadIdx.x;
    if (lane < LMER_NC) s.cs[lane] = C.c[lane];
#pragma unroll
    for (int t = 0; t < MP; t++) s.acc[t * FOLD_CODES + lane] = 0.0;
    __syncthreads();
    const uint32_t first = u_begin + blockIdx.x * (uint32_t)FOLD_CODES;
    const int codes = (int)min((uint32_t)FOLD_CODES, u_end - first);
    /* lanes past the range compare the range's last code and never hit */
    const bool valid = lane < codes;
    const uint32_t u = min(first + (uint32_t)lane, u_end - 1u);
    const sgpr_words sv = (sgpr_words)v;
    int count = 0; /* wave-uniform: sums of ballots' counts only */
    int i = 0;
    for (; i + FOLD_QB <= nv; i += FOLD_QB) {
        uint32_t x[FOLD_QB];
#pragma unroll
        for (int t = 0; t < FOLD_QB; t++) x[t] = sv[i + t];
#pragma unroll
        for (int t0 = 0; t0 < FOLD_QB; t0 += FOLD_HALF) {
            if (count > FOLD_CAP - FOLD_HALF * FOLD_CODES) {
                fold_resolve<MP>(s, count, CV, nm, ms, lane);
                count = 0;
            }
#pragma unroll
            for (int t = t0; t < t0 + FOLD_HALF; t++) count = fold_compare<MP>(s, count, u, valid, x[t], i + t, L, d, lane);
        }
    }
    /* the last nv % 8 classes one by one: the arrays are the caller's, with nothing behind their end */
    for (; i < nv; i++) {
        if (count > FOLD_CAP - FOLD_CODES) {
            fold_resolve<MP>(s, count, CV, nm, ms, lane);
            count = 0;
        }
        count = fold_compare<MP>(s, count, u, valid, sv[i], i, L, d, lane);
    }
    fold_resolve<MP>(s, count, CV, nm, ms, lane);
    /* the tile's rows are one contiguous block of the image: codes * ms doubles, the columns from nm on +0.0 */
    double *out = P + (size_t)(first - u_begin) * (size_t)ms;
    const int cells = codes * ms;
    for (int e = lane; e < cells; e += FOLD_CODES) {
        const int row = e / ms, col = e - row * ms;
        out[e] = col < nm ? s.acc[row * MP + col] : 0.0;
    }
}

} /* namespace */

extern "C" int gkmhip_panel_weights(gkmhip_ctx *ctx, const double *c, const uint32_t *v, const double *CV, int nv, int nm,
                                    int ms, uint32_t u_begin, uint32_t u_end, double *P, void *stream_)
{
    if (!ctx || !c || nv < 0 || (nv > 0 && (!v || !CV))) return set_err_msg("gkmhip_panel_weights: bad arguments", 2);
    if (int rc = panel_check(P, nm, ms, "gkmhip_panel_weights")) return rc;
    const int L = ctx->L, d = ctx->d;
    const uint32_t codes = 1u << (2 * L);
    if (u_begin >= u_end || u_end > codes)
        return set_err_msg("gkmhip_panel_weights: the code range must satisfy 0 <= u_begin < u_end <= 4^L", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const LmerCoef C = lmer_coef(c, d);
    const dim3 grid((unsigned)((u_end - u_begin + FOLD_CODES - 1) / FOLD_CODES));
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    switch (panel_shift(nm)) {
    case 3: hipLaunchKernelGGL(k_panel_weights<8>, grid, dim3(FOLD_CODES), 0, stream, v, CV, nv, nm, ms, u_begin, u_end, C, L, d, P); break;
    case 4: hipLaunchKernelGGL(k_panel_weights<16>, grid, dim3(FOLD_CODES), 0, stream, v, CV, nv, nm, ms, u_begin, u_end, C, L, d, P); break;
    case 5: hipLaunchKernelGGL(k_panel_weights<32>, grid, dim3(FOLD_CODES), 0, stream, v, CV, nv, nm, ms, u_begin, u_end, C, L, d, P); break;
    default: hipLaunchKernelGGL(k_panel_weights<64>, grid, dim3(FOLD_CODES), 0, stream, v, CV, nv, nm, ms, u_begin, u_end, C, L, d, P); break;
    }
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_panel_weights", 2.0 * (double)nv * (double)(u_end - u_begin));
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: panel weights, %d classes x %d models x codes [%u, %u) -> k_panel_weights (%.3g comparisons)\n",
                nv, nm, u_begin, u_end, ctx->last_comparisons);
    return 0;
}
