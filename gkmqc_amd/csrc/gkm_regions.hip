/*
 * gkm_regions.hip -- regions of a scan: the runs of windows whose score stays at or above a threshold,
 * each with its first and last window, how many windows passed, its peak and its summit.  Window i of the launch covers
 * the l-mer words [i s, i s + n), n = width - L + 1, and PASSES when none of them is flagged (LMER_BAD) and
 * score[i ld] >= threshold (a NaN never does).  Consecutive passing windows p < q share a region when q - p <= gap + 1.
 * Peak and summit are the reduction "larger score, on a tie the lower index" over a region's passing windows: exact and
 * associative, so every tree gives the same bits, and nothing here adds two doubles.
 *
 * Kernels
 *   k_regions_word_sums, k_regions_scan_words, k_regions_word_prefix (gkm_wordcnt.h, shared with gkm_dist.hip)
 *                         cnt[p] = flagged words among lm[0 .. p), p = 0 .. nlm: ballots and population counts per 64
 *                         words, the block totals scanned by one wave in a launch of its own.  Window i holds no flagged
 *                         word when cnt[i s + n] == cnt[i s]: two loads, whatever the width.
 *   k_regions_summaries   LANE = WINDOW.  A wave walks RG_WAVE consecutive windows 64 at a time and leaves their summary
 *                         (below); a workgroup's four waves own RG_SPAN consecutive windows.
 *   k_regions_scan        one wave: the exclusive prefix of the wave summaries under `fold`, in place, so that every wave
 *                         of the fill finds what precedes it -- the last passing window, the aggregate of the region
 *                         still open there, the regions begun so far; the total goes into the header.
 *   k_regions_fill        the same walk with that carry: a passing window that begins a region writes its own index as
 *                         `first` of region r and, for r > 0, closes region r - 1 (last, count, peak, summit); the wave
 *                         that holds the last window closes the last region.
 *
 * One step of the walk (regions_step): the pass flags of 64 windows are one ballot; the passing window before a lane is
 * the highest set bit below it, or the running value carried across steps, waves and workgroups; "begins a region" is a
 * second ballot, and a region's rank is the carried count plus a population count below the lane.  Peak and summit are a
 * segmented inclusive scan over the lanes, the segment of a lane starting at the highest begin bit at or below it.
 *
 * The summary of a range of windows: its first and last passing window, the region begins among its passing windows other
 * than the first (those the range decides alone), the aggregate of the passing windows before the first such begin
 * (head) and from the last one on (tail).  `fold` joins two adjacent ranges -- the only place where the later range's
 * first passing window learns whether it begins a region -- and is associative, which is all the scan needs.
 *
 * No workgroup waits for another: what crosses workgroups crosses a launch boundary.  No atomics: a slot is a rank
 * computed from the input order, so order and values are the same bytes on every run.
 */
#include "gkm_wordcnt.h"

namespace {

constexpr int RG_STEPS = 4;                   /* steps of 64 windows per wave */
constexpr int RG_WAVE = 64 * RG_STEPS;        /* windows per wave: one summary */
constexpr int RG_SPAN = RG_WAVE * RG_WAVES;   /* windows per workgroup */
constexpr int64_t RG_MAGIC = 0x31534E4F49474552LL;        /* "REGIONS1" */

/* what k_regions_scan leaves at the head of the scratch: the count, and the launch it belongs to */
struct RegHeader {
    int64_t magic, count, nwin, nlm, shape /* width << 32 | stride */, gap, threshold /* its bits */, ld;
};
static_assert(sizeof(RegHeader) == 64, "the header is 64 bytes");

struct Agg { /* of a set of passing windows; count == 0: the empty set */
    double peak;
    int32_t summit, count;
};

struct Summary {
    int32_t first, last, nstart; /* first < 0: no passing window */
    Agg head, tail;
};

/* a: the earlier windows */
__device__ __forceinline__ Agg agg_join(const Agg &a, const Agg &b)
{
    if (a.count == 0) return b;
    if (b.count == 0) return a;
    Agg r = b.peak > a.peak ? b : a;
    r.count = a.count + b.count;
    return r;
}

__device__ __forceinline__ Summary fold(const Summary &a, const Summary &b, int64_t gap)
{
    if (a.first < 0) return b;
    if (b.first < 0) return a;
    Summary r;
    r.first = a.first;
    r.last = b.last;
    if ((int64_t)b.first - a.last <= gap + 1) {
        r.nstart = a.nstart + b.nstart;
        r.head = a.nstart == 0 ? agg_join(a.head, b.head) : a.head;
        r.tail = b.nstart == 0 ? agg_join(a.tail, b.head) : b.tail;
    } else {
        r.nstart = a.nstart + b.nstart + 1;
        r.head = a.head;
        r.tail = b.tail;
    }
    return r;
}

__device__ __forceinline__ Agg agg_up(const Agg &a, int o)
{
    Agg r;
    r.peak = __shfl_up(a.peak, o, 64);
    r.summit = __shfl_up(a.summit, o, 64);
    r.count = __shfl_up(a.count, o, 64);
    return r;
}

__device__ __forceinline__ Agg agg_from(const Agg &a, int src)
{
    Agg r;
    r.peak = __shfl(a.peak, src, 64);
    r.summit = __shfl(a.summit, src, 64);
    r.count = __shfl(a.count, src, 64);
    return r;
}

__device__ __forceinline__ Summary summary_up(const Summary &s, int o)
{
    Summary r;
    r.first = __shfl_up(s.first, o, 64);
    r.last = __shfl_up(s.last, o, 64);
    r.nstart = __shfl_up(s.nstart, o, 64);
    r.head = agg_up(s.head, o);
    r.tail = agg_up(s.tail, o);
    return r;
}

__device__ __forceinline__ Summary summary_from(const Summary &s, int src)
{
    Summary r;
    r.first = __shfl(s.first, src, 64);
    r.last = __shfl(s.last, src, 64);
    r.nstart = __shfl(s.nstart, src, 64);
    r.head = agg_from(s.head, src);
    r.tail = agg_from(s.tail, src);
    return r;
}

__device__ __forceinline__ Summary summary_none()
{
    Summary s;
    s.first = s.last = -1;
    s.nstart = 0;
    s.head = s.tail = Agg{0.0, 0, 0};
    return s;
}

/* the wave summaries and, after k_regions_scan, the carries, in the scratch: one array per field */
struct RegEntries {
    int32_t *first, *last, *nstart, *head_summit, *head_count, *tail_summit, *tail_count;
    double *head_peak, *tail_peak;
};

/* where the regions go (DEVICE) */
struct RegOut {
    int32_t *first, *last, *summit, *count;
    double *peak;
    int64_t capacity;
};

/* what a launch is about */
struct RegArgs {
    const double *score;
    int64_t ld;
    const uint32_t *cnt;
    int n, s;
    int64_t nwin, gap;
    double threshold;
};

/* the running state of a walk, the same in every lane */
struct Walk {
    int32_t first, last, nreg; /* the first and the last passing window so far (-1: none), the regions begun so far */
    Agg open;                  /* of the passing windows of the region still open */
};

/* The 64 windows from i0 on.  FILL: begins and closed regions go to `out`; otherwise the first region that closes is kept in
 * *head (the walk started without a carry: it is the range's head). */
template <bool FILL>
__device__ __forceinline__ void regions_step(const RegArgs &a, int64_t i0, int lane, Walk &w, const RegOut &out, Agg *head)
{
    const int64_t i = i0 + lane;
    bool pass = false;
    double v = 0.0;
    if (i < a.nwin) {
        const int64_t p = i * a.s;
        v = a.score[i * a.ld];
        pass = a.cnt[p + a.n] == a.cnt[p] && v >= a.threshold;
    }
    const unsigned long long pm = __ballot(pass);
    if (!pm) return; /* (the whole wave) */
    const unsigned long long below = pm & lanes_below(lane);
    const int32_t prev = below ? (int32_t)i0 + 63 - __builtin_clzll(below) : w.last;
    const bool start = pass && (prev < 0 || i - prev > a.gap + 1);
    const unsigned long long sm = __ballot(start);
    /* this lane's segment starts at the highest begin at or below it; without one it reaches back into the open region */
    const unsigned long long mine = sm & ((2ull << lane) - 1ull);
    const int seglo = mine ? 63 - __builtin_clzll(mine) : 0;
    Agg g = pass ? Agg{v, (int32_t)i, 1} : Agg{0.0, 0, 0};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Agg u = agg_up(g, o);
        if (lane - o >= seglo) g = agg_join(u, g);
    }
    /* what a begin at this lane closes: the lane before it, and the open region where that lane's segment reaches back */
    Agg closed = agg_up(g, 1);
    const bool reaches = lane == 0 || !(sm & lanes_below(lane));
    if (lane == 0) closed = Agg{0.0, 0, 0};
    if (reaches) closed = agg_join(w.open, closed);
    const int32_t rank = w.nreg + __popcll(sm & lanes_below(lane));
    if (FILL) {
        if (start && rank < out.capacity) {
            out.first[rank] = (int32_t)i;
            if (rank > 0) {
                out.last[rank - 1] = prev;
                out.summit[rank - 1] = closed.summit;
                out.count[rank - 1] = closed.count;
                out.peak[rank - 1] = closed.peak;
            }
        }
    } else {
        const unsigned long long second = __ballot(start && rank == 1);
        if (second) *head = agg_from(closed, __builtin_ctzll(second));
    }
    const Agg end = agg_from(g, 63);
    w.open = sm ? end : agg_join(w.open, end);
    if (w.first < 0) w.first = (int32_t)i0 + __builtin_ctzll(pm);
    w.last = (int32_t)i0 + 63 - __builtin_clzll(pm);
    w.nreg += __popcll(sm);
}

__global__ __launch_bounds__(RG_THREADS) void k_regions_summaries(RegArgs a, int64_t nent, RegEntries e)
{
    const int lane = threadIdx.x & 63;
    const int64_t ent = (int64_t)blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (ent >= nent) return; /* a whole wave; nothing below waits for the workgroup */
    const int64_t w0 = ent * RG_WAVE;
    Walk w{-1, -1, 0, Agg{0.0, 0, 0}};
    Agg head{0.0, 0, 0};
    for (int r = 0; r < RG_STEPS && w0 + r * 64 < a.nwin; r++) regions_step<false>(a, w0 + r * 64, lane, w, RegOut{}, &head);
    if (lane == 0) {
        if (w.nreg < 2) head = w.open; /* one region, still open: the whole range */
        e.first[ent] = w.first;
        e.last[ent] = w.last;
        e.nstart[ent] = w.nreg > 0 ? w.nreg - 1 : 0;
        e.head_peak[ent] = head.peak;
        e.head_summit[ent] = head.summit;
        e.head_count[ent] = head.count;
        e.tail_peak[ent] = w.open.peak;
        e.tail_summit[ent] = w.open.summit;
        e.tail_count[ent] = w.open.count;
    }
}

/* One wave.  Entry j's summary -> what precedes it: last[j] the last passing window before the range (-1: none), nstart[j]
 * the regions begun before it, tail_*[j] the aggregate of the region open there.  The header is written last. */
__global__ __launch_bounds__(64) void k_regions_scan(RegEntries e, int64_t nent, int64_t gap, RegHeader h,
                                                     RegHeader *__restrict__ header)
{
    const int lane = threadIdx.x;
    Summary carry = summary_none();
    for (int64_t base = 0; base < nent; base += 64) {
        const int64_t j = base + lane;
        Summary s = summary_none();
        if (j < nent) {
            s.first = e.first[j];
            s.last = e.last[j];
            s.nstart = e.nstart[j];
            s.head = Agg{e.head_peak[j], e.head_summit[j], e.head_count[j]};
            s.tail = Agg{e.tail_peak[j], e.tail_summit[j], e.tail_count[j]};
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const Summary u = summary_up(s, o);
            if (lane >= o) s = fold(u, s, gap);
        }
        Summary before = summary_up(s, 1);
        if (lane == 0) before = summary_none();
        before = fold(carry, before, gap);
        if (j < nent) {
            e.last[j] = before.last;
            e.nstart[j] = before.first < 0 ? 0 : before.nstart + 1;
            e.tail_peak[j] = before.tail.peak;
            e.tail_summit[j] = before.tail.summit;
            e.tail_count[j] = before.tail.count;
        }
        carry = fold(carry, summary_from(s, 63), gap);
    }
    if (lane == 0) {
        h.count = carry.first < 0 ? 0 : (int64_t)carry.nstart + 1;
        *header = h;
    }
}

__global__ __launch_bounds__(RG_THREADS) void k_regions_fill(RegArgs a, int64_t nent, RegEntries e, RegOut out)
{
    const int lane = threadIdx.x & 63;
    const int64_t ent = (int64_t)blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (ent >= nent) return;
    const int64_t w0 = ent * RG_WAVE;
    Walk w{0, e.last[ent], e.nstart[ent], Agg{e.tail_peak[ent], e.tail_summit[ent], e.tail_count[ent]}};
    for (int r = 0; r < RG_STEPS && w0 + r * 64 < a.nwin; r++) regions_step<true>(a, w0 + r * 64, lane, w, out, nullptr);
    if (ent == nent - 1 && lane == 0 && w.nreg > 0 && w.nreg <= out.capacity) { /* the last window is behind us */
        out.last[w.nreg - 1] = w.last;
        out.summit[w.nreg - 1] = w.open.summit;
        out.count[w.nreg - 1] = w.open.count;
        out.peak[w.nreg - 1] = w.open.peak;
    }
}

/* the pieces of the scratch, in bytes from its start */
struct RegPlan {
    int64_t nent, wblocks;
    size_t cnt, sums, ent, total; /* offsets of cnt, the word block sums and the entries; the size */
    size_t stride;                /* bytes between the entries' arrays: nent doubles, padded */
};

RegPlan regions_plan(int64_t nlm, int64_t nwin)
{
    RegPlan p;
    p.nent = (nwin + RG_WAVE - 1) / RG_WAVE;
    p.wblocks = wordcnt_blocks(nlm);
    p.cnt = 256;
    p.sums = p.cnt + pad256((size_t)(nlm + 1) * 4);
    p.ent = p.sums + pad256((size_t)p.wblocks * 4);
    p.stride = pad256((size_t)p.nent * 8);
    p.total = p.ent + 9 * p.stride;
    return p;
}

RegEntries regions_entries(char *scratch, const RegPlan &p)
{
    char *b = scratch + p.ent;
    RegEntries e;
    e.head_peak = (double *)b;
    e.tail_peak = (double *)(b + p.stride);
    int32_t **ints[7] = {&e.first, &e.last, &e.nstart, &e.head_summit, &e.head_count, &e.tail_summit, &e.tail_count};
    for (int k = 0; k < 7; k++) *ints[k] = (int32_t *)(b + (2 + k) * p.stride);
    return e;
}

/* what the two entry points check alike: n, or a negative value after set_err_msg */
int regions_check(const gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm, int width,
                  int stride, int64_t nwin, double threshold, int64_t gap, const void *scratch, int64_t scratch_bytes,
                  const char *what)
{
    const int n = scan_check(ctx, lm, nlm, score, width, stride, nwin, scratch, what);
    if (n < 0) return n;
    if (ld < 1) return -set_err_msg(std::string(what) + ": the leading dimension must be at least 1", 2);
    if (gap < 0 || gap > (int64_t)1 << 40) return -set_err_msg(std::string(what) + ": the gap must lie in 0..2^40", 2);
    if (threshold != threshold) return -set_err_msg(std::string(what) + ": the threshold is NaN", 2);
    if (nlm >= (int64_t)1 << 40 || (((uintptr_t)scratch) & 7u) || scratch_bytes < (int64_t)regions_plan(nlm, nwin).total)
        return -set_err_msg(std::string(what) + ": the scratch must be 8-byte aligned and hold gkmhip_regions_scratch_bytes", 2);
    return n;
}

RegHeader regions_header(int64_t ld, int64_t nlm, int width, int stride, int64_t nwin, double threshold, int64_t gap)
{
    RegHeader h;
    h.magic = RG_MAGIC;
    h.count = 0;
    h.nwin = nwin;
    h.nlm = nlm;
    h.shape = ((int64_t)width << 32) | (int64_t)stride;
    h.gap = gap;
    memcpy(&h.threshold, &threshold, 8);
    h.ld = ld;
    return h;
}

} /* namespace */

extern "C" int gkmhip_regions_span(void) { return RG_SPAN; }

extern "C" int64_t gkmhip_regions_scratch_bytes(int64_t nlm, int64_t nwin)
{
    if (nlm < 1 || nlm >= (int64_t)1 << 40 || nwin < 1 || nwin > (int64_t)1 << 30) return -1;
    return (int64_t)regions_plan(nlm, nwin).total;
}

extern "C" int gkmhip_regions_count(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm,
                                    int width, int stride, int64_t nwin, double threshold, int64_t gap, void *scratch,
                                    int64_t scratch_bytes, int64_t *count, void *stream_)
{
    const int n = regions_check(ctx, score, ld, lm, nlm, width, stride, nwin, threshold, gap, scratch, scratch_bytes,
                                "gkmhip_regions_count");
    if (n < 0) return -n;
    if (!count) return set_err_msg("gkmhip_regions_count: bad arguments", 2);
    const RegPlan p = regions_plan(nlm, nwin);
    char *s = (char *)scratch;
    uint32_t *cnt = (uint32_t *)(s + p.cnt), *sums = (uint32_t *)(s + p.sums);
    const RegEntries e = regions_entries(s, p);
    const RegArgs a{score, ld, cnt, n, stride, nwin, gap, threshold};
    const unsigned blocks = (unsigned)((p.nent + RG_WAVES - 1) / RG_WAVES);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    wordcnt_launch(lm, nlm, sums, cnt, stream);
    hipLaunchKernelGGL(k_regions_summaries, dim3(blocks), dim3(RG_THREADS), 0, stream, a, p.nent, e);
    hipLaunchKernelGGL(k_regions_scan, dim3(1), dim3(64), 0, stream, e, p.nent, gap,
                       regions_header(ld, nlm, width, stride, nwin, threshold, gap), (RegHeader *)s);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    int64_t got = 0;
    HIPCHK(hipMemcpyAsync(&got, s + offsetof(RegHeader, count), 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    *count = got;
    gkm_launch_done(ctx, "k_regions_summaries", (double)nwin); /* (windows looked at) */
    return 0;
}

extern "C" int gkmhip_regions_fill(gkmhip_ctx *ctx, const double *score, int64_t ld, const uint32_t *lm, int64_t nlm,
                                   int width, int stride, int64_t nwin, double threshold, int64_t gap, void *scratch,
                                   int64_t scratch_bytes, int64_t capacity, int32_t *first, int32_t *last, int32_t *summit,
                                   int32_t *windows, double *peak, void *stream_)
{
    const int n = regions_check(ctx, score, ld, lm, nlm, width, stride, nwin, threshold, gap, scratch, scratch_bytes,
                                "gkmhip_regions_fill");
    if (n < 0) return -n;
    if (capacity < 0 || (capacity > 0 && (!first || !last || !summit || !windows || !peak)))
        return set_err_msg("gkmhip_regions_fill: bad arguments", 2);
    const RegPlan p = regions_plan(nlm, nwin);
    char *s = (char *)scratch;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gkm_launch_enter(ctx)) return rc;
    RegHeader got;
    HIPCHK(hipMemcpyAsync(&got, s, sizeof got, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const RegHeader want = regions_header(ld, nlm, width, stride, nwin, threshold, gap);
    if (got.magic != want.magic || got.nwin != want.nwin || got.nlm != want.nlm || got.shape != want.shape ||
        got.gap != want.gap || got.threshold != want.threshold || got.ld != want.ld || got.count < 0 || got.count > nwin)
        return set_err_msg("gkmhip_regions_fill: the scratch does not hold gkmhip_regions_count's result for these arguments", 2);
    if (capacity < got.count)
        return set_err_msg("gkmhip_regions_fill: " + std::to_string(got.count) + " regions, capacity " +
                           std::to_string(capacity), 2);
    if (got.count == 0) return 0;
    const RegEntries e = regions_entries(s, p);
    const RegArgs a{score, ld, (const uint32_t *)(s + p.cnt), n, stride, nwin, gap, threshold};
    const RegOut out{first, last, summit, windows, peak, got.count};
    if (int rc = gkm_launch_begin(ctx, stream)) return rc;
    hipLaunchKernelGGL(k_regions_fill, dim3((unsigned)((p.nent + RG_WAVES - 1) / RG_WAVES)), dim3(RG_THREADS), 0, stream, a,
                       p.nent, e, out);
    if (int rc = gkm_launch_stop(ctx, stream)) return rc;
    gkm_launch_done(ctx, "k_regions_fill", (double)nwin);
    return 0;
}
