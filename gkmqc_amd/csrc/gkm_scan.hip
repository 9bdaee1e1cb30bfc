/*
 * gkm_scan.hip -- scanning a long sequence with an l-mer weight table: the score of every window of W
 * bases at a stride s, each as if the window were a query of its own.  With n = W - L + 1 l-mers per window, wt the n
 * positional weights every window shares and window a starting at forward l-mer a,
 *
 *   P_m(a) = sum_{p, q in [a, a + n)} wt[p - a] wt[q - a] ([m(f_p, f_q) = m] + [m(f_p, rc f_q) = m])     exact, 64 bits
 *   T(a)   = sum_{p in [a, a + n)} wt[p - a] W(f_p)
 *
 * The long sequence never enters the per-sequence tables of gkmhip_set_sequences (built for at most 2 047 bases): the
 * kernels take the context for L and d only, and plain device pointers.
 *
 * Kernels
 *   k_scan_lmers     base codes + validity mask -> one word per forward l-mer: the 2L-bit code, LMER_BAD set when the l-mer
 *                    covers an invalid base
 *   k_scan_profiles  HOT.  One workgroup owns a stretch of g <= 64 consecutive windows and stages their n + (g - 1) s
 *                    l-mer words in LDS.  Both strand terms are symmetric in (p, q), so lane p compares its l-mer (and
 *                    its reverse complement) with the l-mers q = p + delta, 0 <= delta < n, once: a pair is compared once
 *                    per strand for the whole stretch, not once per window that holds it.  A hit (m <= d on either
 *                    strand) is resolved by the whole wave with LANE i = WINDOW i of the stretch: every window that
 *                    holds both l-mers adds (2 - [delta = 0]) wt[p - a_i] wt[q - a_i] to its own counter.  A wave's
 *                    counters are its own and a lane only ever touches its window's, so the sums need no atomics; they
 *                    are integers, so no order matters.  The waves' counters are added at the end.
 *   k_scan_score     T(a), one wave per window, in k_lmer_score's order: lane l takes p = l, l + 64, ... ascending, then
 *                    the same butterfly; wt from a table of n bytes
 *
 * A flagged l-mer takes part in no pair: a window that holds one has no profile worth reading, and the caller drops it.
 */
#include "gkm_lmer_dev.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_GMAX = 64;       /* windows per stretch: one lane each when a hit is resolved */
constexpr int SP_STRETCH = 4096;  /* l-mer words of a stretch in LDS, at most */
constexpr int SS_THREADS = 256;   /* four windows per workgroup in k_scan_score */

/* windows per stretch: a function of (n, s) -- that is of (L, W, s) -- only */
inline int scan_group(int n, int s)
{
    if (s >= n) return 1; /* windows share no pair */
    return (int)std::min<int64_t>(SP_GMAX, 1 + (SP_STRETCH - n) / s);
}

/* pairs of a stretch of gw windows: q = p + delta, 0 <= delta < n, q inside the stretch; once per strand */
inline double stretch_comparisons(int n, int s, int gw)
{
    const double S = (double)n + (double)(gw - 1) * s;
    return 2.0 * (S * n - 0.5 * (double)n * (n - 1));
}

__global__ __launch_bounds__(256) void k_scan_lmers(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ valid,
                                                    int64_t nlm, int L, uint32_t *__restrict__ lm)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nlm) return;
    uint32_t v = 0u, ok = 1u;
    for (int i = 0; i < L; i++) {
        v = (v << 2) | (uint32_t)(codes[p + i] & 3);
        ok &= (uint32_t)(valid[p + i] != 0);
    }
    lm[p] = ok ? v : (v | LMER_BAD);
}

/* lm: the l-mer words from the first window's first l-mer on; window i of the launch starts at l-mer i * s.
 * Dynamic LDS: [SP_WAVES][d + 1][64] counters, the stretch's words, wt. */
__global__ __launch_bounds__(SP_THREADS) void k_scan_profiles(const uint32_t *__restrict__ lm, const uint8_t *__restrict__ wt,
                                                              int n, int s, int g, int64_t nwin, int L, int d,
                                                              int64_t *__restrict__ prof)
{
    extern __shared__ unsigned long long scan_lds[];
    unsigned long long *cnt = scan_lds;
    uint32_t *sl = (uint32_t *)(cnt + SP_WAVES * (d + 1) * 64);
    const int64_t w0 = (int64_t)blockIdx.x * g;
    const int gw = (int)min((int64_t)g, nwin - w0);
    const int S = n + (gw - 1) * s;
    uint8_t *swt = (uint8_t *)(sl + S);
    const uint32_t *src = lm + w0 * s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < SP_WAVES * (d + 1) * 64; e += SP_THREADS) cnt[e] = 0ull;
    for (int e = tid; e < S; e += SP_THREADS) sl[e] = src[e];
    for (int e = tid; e < n; e += SP_THREADS) swt[e] = wt[e];
    __syncthreads();
    unsigned long long *mine = cnt + wave * (d + 1) * 64 + lane;
    const int la = lane < gw ? lane * s : 0; /* the first l-mer of this lane's window, in the stretch */
    for (int base = wave * 64; base < S; base += SP_THREADS) {
        const int p = base + lane;
        const uint32_t xe = sl[min(p, S - 1)];
        const bool pok = p < S && !(xe & LMER_BAD);
        const uint32_t xf = xe & LMER_CODE, xr = lmer_rc(xf, L);
        const int dmax = min(n, S - base); /* (wave-uniform) */
        for (int delta = 0; delta < dmax; delta++) {
            const int q = p + delta;
            const uint32_t ye = sl[min(q, S - 1)];
            const int mf = lmer_mm(xf, ye & LMER_CODE), mr = lmer_mm(xr, ye & LMER_CODE);
            const bool hit = pok && q < S && !(ye & LMER_BAD) && min(mf, mr) <= d;
            unsigned long long todo = __ballot(hit);
            const int mm = mf | (mr << 8);
            while (todo) {
                const int hl = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int hm = __builtin_amdgcn_readlane(mm, hl);
                const int hf = hm & 0xFF, hr = hm >> 8;
                /* this lane's window holds both l-mers: a_i <= p and p + delta < a_i + n */
                const int pa = base + hl - la;
                if (lane < gw && pa >= 0 && pa + delta < n) {
                    const unsigned long long v =
                        (unsigned long long)((uint32_t)swt[pa] * (uint32_t)swt[pa + delta]) << (delta ? 1 : 0);
                    if (hf <= d) mine[hf * 64] += v;
                    if (hr <= d) mine[hr * 64] += v;
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < gw * (d + 1); e += SP_THREADS) {
        const int i = e / (d + 1), m = e - i * (d + 1);
        unsigned long long t = 0ull;
#pragma unroll
        for (int w = 0; w < SP_WAVES; w++) t += cnt[(w * (d + 1) + m) * 64 + i];
        prof[(w0 + i) * (d + 1) + m] = (int64_t)t;
    }
}

__global__ __launch_bounds__(SS_THREADS) void k_scan_score(const uint32_t *__restrict__ lm, const uint8_t *__restrict__ wt,
                                                           int n, int s, int64_t nwin, const double *__restrict__ W,
                                                           double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (SS_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nwin) return; /* a whole wave: nothing below waits for the workgroup */
    const uint32_t *e = lm + i * s;
    double acc = 0.0;
    for (int p = lane; p < n; p += 64) acc += (double)wt[p] * W[e[p] & LMER_CODE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[i] = acc;
}

} /* namespace */

/* the checks the window launches share, gkm_panel.hip's included: n, or a negative value after set_err_msg */
int scan_check(const gkmhip_ctx *ctx, const void *lm, int64_t nlm, const void *wt, int width, int stride, int64_t nwin,
               const void *out, const char *what)
{
    if (!ctx || !lm || !wt || !out) return -set_err_msg(std::string(what) + ": bad arguments", 2);
    if (width < ctx->L || width > GKM_MAXLEN)
        return -set_err_msg(std::string(what) + ": the width must lie in L.." + std::to_string(GKM_MAXLEN), 2);
    if (stride < 1) return -set_err_msg(std::string(what) + ": the stride must be at least 1", 2);
    const int n = width - ctx->L + 1;
    if (nwin < 1 || nwin > (int64_t)1 << 30 || (nwin - 1) * (int64_t)stride + n > nlm)
        return -set_err_msg(std::string(what) + ": the windows must lie inside the l-mer words given", 2);
    return n;
}

extern "C" int gkmhip_scan_group(const gkmhip_ctx *ctx, int width, int stride)
{
    if (!ctx || width < ctx->L || width > GKM_MAXLEN || stride < 1) return 0;
    return scan_group(width - ctx->L + 1, stride);
}

extern "C" int gkmhip_scan_lmers(gkmhip_ctx *ctx, const uint8_t *codes, const uint8_t *valid, int64_t nbases, uint32_t *lm,
                                 void *stream_)
{
    if (!ctx || !codes || !valid || !lm) return set_err_msg("gkmhip_scan_lmers: bad arguments", 2);
    const int64_t nlm = nbases - ctx->L + 1;
    if (nlm < 1 || nlm > ((int64_t)1 << 31) * 256 - 256)
        return set_err_msg("gkmhip_scan_lmers: needs at least L bases (and fewer than 2^39)", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    hipLaunchKernelGGL(k_scan_lmers, dim3((unsigned)((nlm + 255) / 256)), dim3(256), 0, stream, codes, valid, nlm, ctx->L, lm);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gkmhip_scan_profiles(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width,
                                    int stride, int64_t nwin, int64_t *prof, void *stream_)
{
    const int n = scan_check(ctx, lm, nlm, wt, width, stride, nwin, prof, "gkmhip_scan_profiles");
    if (n < 0) return -n;
    const int d = ctx->d;
    const int g = scan_group(n, stride);
    const int64_t blocks = (nwin + g - 1) / g;
    const int last = (int)(nwin - (blocks - 1) * g);
    /* counters, the longest stretch, wt */
    const size_t lds = (size_t)SP_WAVES * (d + 1) * 64 * 8 + ((size_t)n + (size_t)(g - 1) * stride) * 4 + (size_t)n;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_scan_profiles, dim3((unsigned)blocks), dim3(SP_THREADS), lds, stream, lm, wt, n, stride, g, nwin,
                       ctx->L, d, prof);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_scan_profiles",
                    (double)(blocks - 1) * stretch_comparisons(n, stride, g) + stretch_comparisons(n, stride, last));
    if (getenv("GKM_TRACE"))
        fprintf(stderr, "gkmhip: scan profiles, %lld windows of %d l-mers at stride %d -> k_scan_profiles (%lld stretches of "
                        "%d windows, %zu bytes of LDS, %.3g comparisons)\n", (long long)nwin, n, stride, (long long)blocks, g,
                lds, ctx->last_comparisons);
    return 0;
}

extern "C" int gkmhip_scan_score(gkmhip_ctx *ctx, const uint32_t *lm, int64_t nlm, const uint8_t *wt, int width, int stride,
                                 int64_t nwin, const double *W, double *out, void *stream_)
{
    const int n = scan_check(ctx, lm, nlm, wt, width, stride, nwin, out, "gkmhip_scan_score");
    if (n < 0) return -n;
    if (!W) return set_err_msg("gkmhip_scan_score: bad arguments", 2);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    const int per = SS_THREADS / 64;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_scan_score, dim3((unsigned)((nwin + per - 1) / per)), dim3(SS_THREADS), 0, stream, lm, wt, n, stride,
                       nwin, W, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_scan_score", (double)nwin * n); /* (l-mers looked up) */
    return 0;
}
