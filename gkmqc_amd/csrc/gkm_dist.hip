/*
 * gkm_dist.hip -- the distribution of a scan's scores: histograms of the scored windows of a launch by a
 * digit of an order-preserving 64-bit key or by a list of ascending edges, and the scores under given key prefixes
 * gathered into a bounded buffer.  Window i of the launch covers the l-mer words [i s, i s + n), n = width - L + 1, and
 * is SCORED when none of them is flagged (LMER_BAD) and score[i ld] is no NaN.  What stands at any other window is read
 * but never used as a value.
 *
 * The key of a double with the bits b is b ^ (b >> 63 ? ~0 : 1 << 63): ascending keys are ascending non-NaN doubles,
 * -0.0 just below +0.0.  Its 64 bits are resolved in DS_LEVELS levels, the first of DS_BITS0 bits, the others of DS_BITS.
 *
 * Kernels
 *   k_regions_word_sums, k_regions_scan_words, k_regions_word_prefix (gkm_wordcnt.h)
 *                    cnt[p], the flagged words before word p: validity is two loads per window.
 *   k_dist_digits    LANE = WINDOW, DS_STEPS windows per thread.  Level 0: every scored window counts at its key's top
 *                    DS_BITS0 bits in the workgroup's LDS histogram, whose non-zero counters are added to `hist` once.
 *                    Deeper: the wave holds the (at most 64) prefixes one per lane; a window finds its prefix by a
 *                    binary search of six shuffles and adds 1 at hist[prefix j][next digit] in global memory -- few
 *                    windows match, and nprefix * 2^DS_BITS counters would not fit in LDS.
 *   k_dist_edges     the same body (dist_count) with another binning functor: edges and counters in LDS, a window's bin
 *                    the number of edges <= its score by a binary search of fixed length.
 *   k_dist_collect   a window under one of the prefixes appends its score: one integer atomic per wave and step takes
 *                    the wave's slots, ballot and population count rank the lanes inside them.
 *
 * Every atomic adds an integer: the counts are sums of ones, the same bytes on every run whatever order the hardware
 * serves them in.  Only the ORDER of k_dist_collect's values depends on the run; their multiset does not.  No workgroup
 * waits for another.
 */
#include "gkm_wordcnt.h"

namespace {

constexpr int DS_BITS = 13;                                   /* what a level after the first resolves */
constexpr int DS_LEVELS = (64 + DS_BITS - 1) / DS_BITS;       /* 5 */
constexpr int DS_BITS0 = 64 - DS_BITS * (DS_LEVELS - 1);      /* 12: the sign and the exponent */
constexpr int DS_THREADS = 256;
constexpr int DS_STEPS = 4;                                   /* windows per thread */
constexpr int DS_SPAN = DS_THREADS * DS_STEPS;                /* windows per workgroup */
constexpr int DS_MAXPREFIX = 64;
constexpr int DS_MAXEDGES = 4096;
/* 2^DS_BITS counters are 32 KiB, a fifth of a CU's LDS; k_dist_edges keeps 48 KiB (edges and counters) */
static_assert((sizeof(uint32_t) << DS_BITS) <= 32768 && DS_BITS0 <= DS_BITS, "a level's histogram fits in LDS");

struct DistArgs {
    const double *score;
    int64_t ld;
    const uint32_t *cnt;
    int n, s;
    int64_t nwin;
};

struct DistPrefixes {
    unsigned long long v[DS_MAXPREFIX]; /* ascending, padded with ~0 (no prefix has 64 bits) */
    int shift;                          /* 64 - prefix_bits */
};

__device__ __forceinline__ unsigned long long dist_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}

/* the score of window i, and whether it is one */
__device__ __forceinline__ bool dist_scored(const DistArgs &a, int64_t i, double *v)
{
    if (i >= a.nwin) return false;
    const int64_t p = i * a.s;
    *v = a.score[i * a.ld];
    return a.cnt[p + a.n] == a.cnt[p] && *v == *v;
}

/* mine: this lane's prefix.  -> the index of the prefix that equals p, or -1; every lane of the wave must call it */
__device__ __forceinline__ int dist_find(unsigned long long mine, unsigned long long p)
{
    int j = 0;
#pragma unroll
    for (int h = DS_MAXPREFIX / 2; h; h >>= 1) {
        const unsigned long long q = __shfl(mine, j + h - 1, 64);
        if (q < p) j += h;
    }
    return __shfl(mine, j, 64) == p ? j : -1;
}

/* The binning functors: LOCAL -- the bins are the workgroup's LDS counters, flushed once -- or straight into `hist`.
 * prepare(): before the first window, by the whole workgroup; operator(): by every lane of a wave, scored or not. */
struct BinTopDigit {
    static constexpr bool LOCAL = true;
    __device__ __forceinline__ void prepare() const {}
    __device__ __forceinline__ int operator()(double v, bool scored) const
    {
        return scored ? (int)(dist_key(v) >> (64 - DS_BITS0)) : -1;
    }
};

struct BinPrefixDigit {
    static constexpr bool LOCAL = false;
    unsigned long long mine;
    int shift;
    __device__ __forceinline__ void prepare() const {}
    __device__ __forceinline__ int operator()(double v, bool scored) const
    {
        const unsigned long long k = dist_key(v);
        const int j = dist_find(mine, k >> shift);
        return scored && j >= 0 ? (j << DS_BITS) | (int)((k >> (shift - DS_BITS)) & ((1u << DS_BITS) - 1u)) : -1;
    }
};

struct BinEdges {
    static constexpr bool LOCAL = true;
    const double *edges; /* DEVICE */
    double *local;       /* LDS */
    int nedges, top;     /* top: the largest power of two <= nedges */
    __device__ __forceinline__ void prepare() const
    {
        for (int e = threadIdx.x; e < nedges; e += DS_THREADS) local[e] = edges[e];
    }
    __device__ __forceinline__ int operator()(double v, bool scored) const
    {
        int lo = 0; /* local[0 .. lo) <= v */
        for (int h = top; h; h >>= 1) {
            const int m = lo + h;
            if (m <= nedges && local[m - 1] <= v) lo = m;
        }
        return scored ? lo : -1;
    }
};

/* the body of k_dist_digits and k_dist_edges; counters: LDS, nlocal of them (LOCAL only) */
template <class Bin>
__device__ __forceinline__ void dist_count(const DistArgs &a, const Bin &bin, uint32_t *counters, int nlocal,
                                           unsigned long long *__restrict__ hist)
{
    if (Bin::LOCAL) {
        for (int c = threadIdx.x; c < nlocal; c += DS_THREADS) counters[c] = 0u;
        bin.prepare();
        __syncthreads();
    }
    const int64_t i0 = (int64_t)blockIdx.x * DS_SPAN + threadIdx.x;
#pragma unroll
    for (int r = 0; r < DS_STEPS; r++) {
        double v = 0.0;
        const bool scored = dist_scored(a, i0 + r * DS_THREADS, &v);
        const int b = bin(v, scored);
        if (b >= 0) {
            if (Bin::LOCAL) atomicAdd(&counters[b], 1u);
            else atomicAdd(&hist[b], 1ull);
        }
    }
    if (Bin::LOCAL) {
        __syncthreads();
        for (int c = threadIdx.x; c < nlocal; c += DS_THREADS) {
            const uint32_t k = counters[c];
            if (k) atomicAdd(&hist[c], (unsigned long long)k);
        }
    }
}

/* nprefix == 0: level 0 */
__global__ __launch_bounds__(DS_THREADS) void k_dist_digits(DistArgs a, DistPrefixes pre, int nprefix,
                                                            unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t counters[1 << DS_BITS0];
    if (nprefix == 0) dist_count(a, BinTopDigit{}, counters, 1 << DS_BITS0, hist);
    else dist_count(a, BinPrefixDigit{pre.v[threadIdx.x & 63], pre.shift}, counters, 0, hist);
}

__global__ __launch_bounds__(DS_THREADS) void k_dist_edges(DistArgs a, const double *__restrict__ edges, int nedges, int top,
                                                           unsigned long long *__restrict__ hist)
{
    __shared__ double local[DS_MAXEDGES];
    __shared__ uint32_t counters[DS_MAXEDGES + 1];
    dist_count(a, BinEdges{edges, local, nedges, top}, counters, nedges + 1, hist);
}

__global__ __launch_bounds__(DS_THREADS) void k_dist_collect(DistArgs a, DistPrefixes pre, double *__restrict__ out,
                                                             int64_t capacity, unsigned long long *__restrict__ counter)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long mine = pre.v[lane];
    const int64_t i0 = (int64_t)blockIdx.x * DS_SPAN + threadIdx.x;
#pragma unroll
    for (int r = 0; r < DS_STEPS; r++) {
        double v = 0.0;
        const bool scored = dist_scored(a, i0 + r * DS_THREADS, &v);
        const bool take = dist_find(mine, dist_key(v) >> pre.shift) >= 0 && scored;
        const unsigned long long m = __ballot(take);
        if (!m) continue; /* (the whole wave) */
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(counter, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const int64_t at = (int64_t)base + __popcll(m & lanes_below(lane));
        if (take && at < capacity) out[at] = v;
    }
}

struct DistPlan {
    size_t cnt, sums, total; /* offsets of cnt and of the word block sums in the scratch; its size */
};

DistPlan dist_plan(int64_t nlm)
{
    DistPlan p;
    p.cnt = 0;
    p.sums = pad256((size_t)(nlm + 1) * 4);
    p.total = p.sums + pad256((size_t)wordcnt_blocks(nlm) * 4);
    return p;
}

/* what the three entry points check alike: n, or a negative value after set_err_msg */
int dist_check(const gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
               int stride, int64_t nwin, const void *scratch, int64_t scratch_bytes, const char *what)
{
    const int n = scan_check(ctx, lm, nlm, score, width, stride, nwin, scratch, what);
    if (n < 0) return n;
    if (ld < 1) return -set_err_msg(std::string(what) + ": the leading dimension must be at least 1", 2);
    if (nlm >= (int64_t)1 << 40 || (((uintptr_t)scratch) & 7u) || scratch_bytes < (int64_t)dist_plan(nlm).total)
        return -set_err_msg(std::string(what) + ": the scratch must be 8-byte aligned and hold gkmhip_dist_scratch_bytes", 2);
    return n;
}

/* the HOST prefixes of a call -> the kernel's block: 0, or an error code after set_err_msg */
int dist_prefixes(const uint64_t *prefix, int nprefix, int prefix_bits, DistPrefixes *out, const char *what)
{
    if (nprefix < 1 || nprefix > DS_MAXPREFIX || !prefix)
        return set_err_msg(std::string(what) + ": 1.." + std::to_string(DS_MAXPREFIX) + " prefixes", 2);
    if (prefix_bits < DS_BITS0 || prefix_bits >= 64 || (prefix_bits - DS_BITS0) % DS_BITS)
        return set_err_msg(std::string(what) + ": prefix_bits " + std::to_string(prefix_bits) + " is no level boundary (" +
                           std::to_string(DS_BITS0) + " + j * " + std::to_string(DS_BITS) + " below 64)", 2);
    for (int j = 0; j < nprefix; j++)
        if ((prefix[j] >> prefix_bits) || (j && prefix[j] <= prefix[j - 1]))
            return set_err_msg(std::string(what) + ": the prefixes must ascend strictly and have prefix_bits bits", 2);
    for (int j = 0; j < DS_MAXPREFIX; j++) out->v[j] = j < nprefix ? prefix[j] : ~0ull;
    out->shift = 64 - prefix_bits;
    return 0;
}

DistArgs dist_begin(const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int n, int stride, int64_t nwin,
                    void *scratch, hipStream_t stream)
{
    const DistPlan p = dist_plan(nlm);
    uint32_t *cnt = (uint32_t *)((char *)scratch + p.cnt), *sums = (uint32_t *)((char *)scratch + p.sums);
    wordcnt_launch(lm, nlm, sums, cnt, stream);
    return DistArgs{score, ld, cnt, n, stride, nwin};
}

inline dim3 dist_grid(int64_t nwin) { return dim3((unsigned)((nwin + DS_SPAN - 1) / DS_SPAN)); }

} /* namespace */

extern "C" int gkmhip_dist_digit_bits(void) { return DS_BITS; }

extern "C" int64_t gkmhip_dist_scratch_bytes(int64_t nlm, int64_t nwin)
{
    if (nlm < 1 || nlm >= (int64_t)1 << 40 || nwin < 1 || nwin > (int64_t)1 << 30) return -1;
    return (int64_t)dist_plan(nlm).total;
}

extern "C" int gkmhip_dist_digits(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm,
                                  int width, int stride, int64_t nwin, const uint64_t *prefix, int nprefix,
                                  int prefix_bits, uint64_t *hist, void *scratch, int64_t scratch_bytes, void *stream_)
{
    const char *what = "gkmhip_dist_digits";
    const int n = dist_check(ctx, score, ld, lm, nlm, width, stride, nwin, scratch, scratch_bytes, what);
    if (n < 0) return -n;
    if (!hist || (((uintptr_t)hist) & 7u)) return set_err_msg(std::string(what) + ": bad arguments", 2);
    DistPrefixes pre{};
    if (nprefix == 0) {
        if (prefix_bits != 0) return set_err_msg(std::string(what) + ": level 0 (no prefix) has prefix_bits 0", 2);
    } else if (int rc = dist_prefixes(prefix, nprefix, prefix_bits, &pre, what)) {
        return rc;
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    const DistArgs a = dist_begin(score, ld, lm, nlm, n, stride, nwin, scratch, stream);
    hipLaunchKernelGGL(k_dist_digits, dist_grid(nwin), dim3(DS_THREADS), 0, stream, a, pre, nprefix,
                       (unsigned long long *)hist);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_dist_digits", (double)nwin); /* (windows looked at) */
    return 0;
}

extern "C" int gkmhip_dist_edges(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm,
                                 int width, int stride, int64_t nwin, const double *edges, int nedges, uint64_t *hist,
                                 void *scratch, int64_t scratch_bytes, void *stream_)
{
    const char *what = "gkmhip_dist_edges";
    const int n = dist_check(ctx, score, ld, lm, nlm, width, stride, nwin, scratch, scratch_bytes, what);
    if (n < 0) return -n;
    if (!hist || (((uintptr_t)hist) & 7u) || !edges || (((uintptr_t)edges) & 7u))
        return set_err_msg(std::string(what) + ": bad arguments", 2);
    if (nedges < 1 || nedges > DS_MAXEDGES)
        return set_err_msg(std::string(what) + ": 1.." + std::to_string(DS_MAXEDGES) + " edges", 2);
    int top = 1;
    while (top * 2 <= nedges) top *= 2;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    const DistArgs a = dist_begin(score, ld, lm, nlm, n, stride, nwin, scratch, stream);
    hipLaunchKernelGGL(k_dist_edges, dist_grid(nwin), dim3(DS_THREADS), 0, stream, a, edges, nedges, top,
                       (unsigned long long *)hist);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_dist_edges", (double)nwin);
    return 0;
}

extern "C" int gkmhip_dist_collect(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm,
                                   int width, int stride, int64_t nwin, const uint64_t *prefix, int nprefix,
                                   int prefix_bits, double *out, int64_t capacity, int64_t *counter, void *scratch,
                                   int64_t scratch_bytes, void *stream_)
{
    const char *what = "gkmhip_dist_collect";
    const int n = dist_check(ctx, score, ld, lm, nlm, width, stride, nwin, scratch, scratch_bytes, what);
    if (n < 0) return -n;
    if (!counter || (((uintptr_t)counter) & 7u) || capacity < 0 || (capacity > 0 && (!out || (((uintptr_t)out) & 7u))))
        return set_err_msg(std::string(what) + ": bad arguments", 2);
    DistPrefixes pre{};
    if (int rc = dist_prefixes(prefix, nprefix, prefix_bits, &pre, what)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    const DistArgs a = dist_begin(score, ld, lm, nlm, n, stride, nwin, scratch, stream);
    hipLaunchKernelGGL(k_dist_collect, dist_grid(nwin), dim3(DS_THREADS), 0, stream, a, pre, out, capacity,
                       (unsigned long long *)counter);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_dist_collect", (double)nwin);
    return 0;
}
