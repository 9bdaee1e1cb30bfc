/*
 * bitslice_cpu_probe.cpp -- runs the per-lane bit-sliced program of gkm_bitslice.h on
 * the CPU for one (row sequence, column sequence) pair.  UNIT-TEST HARNESS for the
 * product's kernel logic (tests/test_bitslice_core.py); it is not linked into
 * gkmkern_pylib.so and is not a fallback path.
 */
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "gkm_bitslice.h"
#include "gkm_pack.h"

using namespace gkmbs;

template <int W, int L, int D>
static void run_pair(const uint8_t *A, int lenA, const uint8_t *B, int lenB, const uint8_t *wd,
                     uint32_t *acc /* [1<<NB] */)
{
    constexpr int NB = planes_for(D);
    constexpr int CAP = segment_capacity(W, L);
    const int nA = lenA - L + 1, nB = lenB - L + 1, T = lenB;
    for (int k = 0; k <= D; k++) acc[k] = 0;
    (void)NB;
    std::vector<uint32_t> sb[2][3];
    for (int st = 0; st < 2; st++)
        for (int pl = 0; pl < 3; pl++) {
            sb[st][pl].resize((size_t)T + W);
            for (int x = 0; x < T + W; x++) sb[st][pl][(size_t)x] = sb_word(B, T, st, x, W, L, pl);
        }
    const uint32_t rcpT = mod_magic((uint32_t)T);
    auto wdist = [&](int dd) { return wd ? (uint32_t)wd[dd] : 1u; };
    /* packed column strands, as the kernel holds them in LDS */
    const int pkw = (T + 15) / 16 + 1;
    std::vector<uint32_t> pkB[2];
    for (int st = 0; st < 2; st++) {
        pkB[st].resize((size_t)pkw);
        for (int x = 0; x < pkw; x++) pkB[st][(size_t)x] = pk_word(B, T, st, x);
    }
    for (int s0 = 0; s0 < nA; s0 += CAP) {
        uint32_t Ahi[W], Alo[W], AV[W];
        for (int w = 0; w < W; w++) {
            Ahi[w] = row_plane_word(A, lenA, s0, w, W, L, 0);
            Alo[w] = row_plane_word(A, lenA, s0, w, W, L, 1);
            AV[w] = row_plane_word(A, lenA, s0, w, W, L, 2);
        }
        /* the lane's packed positions: base i of the segment is sequence position s0 + i */
        uint32_t lanepk[2 * W + 2];
        for (int x = 0; x < 2 * W + 2; x++) {
            uint32_t v = 0u;
            for (int k = 0; k < 16; k++) {
                const int pos = s0 + x * 16 + k;
                if (x * 16 + k < 32 * W && pos < lenA) v |= (uint32_t)A[pos] << (2 * k);
            }
            lanepk[x] = v;
        }
        auto rl = [&](int i0) { return pk_window(lanepk[i0 >> 4], lanepk[(i0 >> 4) + 1], i0); };
        auto cl = [&](int st, int q) { return pk_window(pkB[st][(size_t)(q >> 4)], pkB[st][(size_t)(q >> 4) + 1], q); };
        const int c0 = nA / 2 - s0;
        for (int st = 0; st < 2; st++)
            for (int delta = 0; delta < T; delta++) {
                uint32_t hit[W];
                /* odd shifts exercise the variant that leaves the column-side validity to resolve_hit */
                window_hits<W, L, D>(Ahi, Alo, AV, &sb[st][0][(size_t)delta], &sb[st][1][(size_t)delta],
                                     (delta & 1) ? (const uint32_t *)nullptr : &sb[st][2][(size_t)delta], hit);
                for (int w = 0; w < W; w++) {
                    uint32_t h = hit[w];
                    while (h) {
                        const int bit = __builtin_ctz(h);
                        h &= h - 1u;
                        const HitValue hv = resolve_hit_packed<W>(bit, w, delta, st, (uint32_t)T, rcpT, nB, L, c0, rl, cl, wdist);
                        if (hv.m <= D) acc[hv.m] += hv.v; /* (a wrapped window comes back as m = 0, v = 0) */
                    }
                }
            }
    }
}

#define CASE(WW, LL, DD) \
    if (W == WW && L == LL && d == DD) { run_pair<WW, LL, DD>(A, lenA, B, lenB, wd, acc); ok = 1; }

/* wd: distance-indexed positional weight table (NULL = unweighted) */
extern "C" int bsprobe_profile(int W, int L, int d, const uint8_t *A, int lenA, const uint8_t *B, int lenB,
                               const uint8_t *wd, int32_t *P)
{
    uint32_t acc[16] = {0};
    int ok = 0;
    CASE(10, 11, 3) CASE(10, 10, 3) CASE(10, 12, 4) CASE(10, 8, 4) CASE(10, 9, 4) CASE(10, 12, 6) CASE(10, 11, 5) CASE(10, 12, 5)
    CASE(10, 4, 2) CASE(10, 2, 1) CASE(10, 3, 0) CASE(10, 5, 2) CASE(10, 6, 3) CASE(10, 7, 3)
    CASE(5, 11, 3) CASE(16, 11, 3) CASE(3, 12, 4) CASE(10, 12, 8) CASE(10, 12, 12) CASE(10, 11, 1)
    CASE(10, 9, 5) CASE(10, 10, 5) CASE(10, 10, 6) CASE(10, 11, 6) CASE(10, 11, 7) CASE(10, 12, 7) /* more d > 4 pairs (the device table holds (10,5), (11,5), (12,5), (12,6) of them) */
    if (!ok) return 1;
    for (int m = 0; m <= d; m++) P[m] = (int32_t)acc[m];
    return 0;
}

/* ---- the two entries of one shift side by side (tests/test_group_any.py) ----------------------
 * Runs window_hits (Bv == nullptr, as the kernel calls it) and window_group_any on the same planes: hit_or[g] = OR of the
 * hit words of group g, any[g] = what window_group_any delivers.  Bhi / Blo: W words.  *top_plane: does this (L, d) count
 * matches and threshold on the top plane?  Returns 1 for an (L, d) that is not in the device table. */
template <int W, int L, int D, int GRP>
static void run_group_any(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV, const uint32_t *Bhi, const uint32_t *Blo,
                          uint32_t *hit_or, uint32_t *any)
{
    uint32_t hit[W];
    window_hits<W, L, D>(Ahi, Alo, AV, Bhi, Blo, (const uint32_t *)nullptr, hit);
    for (int g = 0; g < W / GRP; g++) {
        hit_or[g] = 0u;
        for (int k = 0; k < GRP; k++) hit_or[g] |= hit[g * GRP + k];
    }
    window_group_any<W, L, D, GRP>(Ahi, Alo, AV, Bhi, Blo, any);
}

#define GCASE(LL, DD) \
    if (L == LL && d == DD) { run_group_any<10, LL, DD, 5>(Ahi, Alo, AV, Bhi, Blo, hit_or, any); *top_plane = top_plane_serves(LL, DD) ? 1 : 0; return 0; }
#define GCASE_L(LL) GCASE(LL, 0) GCASE(LL, 1) GCASE(LL, 2) GCASE(LL, 3) GCASE(LL, 4)

/* W = 10, groups of five: the table behind gkm_pick_bitslice (gkm_gram_bitslice.hip) */
extern "C" int bsprobe_group_any(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV, const uint32_t *Bhi,
                                 const uint32_t *Blo, uint32_t *hit_or, uint32_t *any, int *top_plane)
{
    GCASE_L(5) GCASE_L(6) GCASE_L(7) GCASE_L(8) GCASE_L(9) GCASE_L(10) GCASE_L(11) GCASE_L(12)
    GCASE(11, 5) GCASE(12, 5) GCASE(12, 6)
    return 1;
}

/* ---- the grouped-validity entry (tests/test_group_validity.py) ----------------------------------
 * window_group_any_grouped on the planes given, with AVg built from AV the way k_gram_bitslice builds it: any_grouped[g];
 * beside it top_or[g] = OR over the group of the top planes with every window valid (window_group_any with AV = ~0), so
 * that the test can state any_grouped == top_or & AVg, and avg[g] itself.  Returns 1 for an (L, d) outside the device
 * table, 2 for one whose threshold is not the top plane (the grouped entry does not exist there). */
template <int W, int L, int D, int GRP>
static int run_group_any_grouped(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV, const uint32_t *Bhi,
                                 const uint32_t *Blo, uint32_t *any_grouped, uint32_t *top_or, uint32_t *avg)
{
    if constexpr (!top_plane_serves(L, D)) {
        return 2;
    } else {
        uint32_t ones[W];
        for (int w = 0; w < W; w++) ones[w] = 0xFFFFFFFFu;
        window_group_any<W, L, D, GRP>(Ahi, Alo, ones, Bhi, Blo, top_or);
        for (int g = 0; g < W / GRP; g++) {
            avg[g] = 0u;
            for (int k = 0; k < GRP; k++) avg[g] |= AV[g * GRP + k];
        }
        window_group_any_grouped<W, L, D, GRP>(Ahi, Alo, avg, Bhi, Blo, any_grouped);
        return 0;
    }
}

#define GGCASE(LL, DD) \
    if (L == LL && d == DD) return run_group_any_grouped<10, LL, DD, 5>(Ahi, Alo, AV, Bhi, Blo, any_grouped, top_or, avg);
#define GGCASE_L(LL) GGCASE(LL, 0) GGCASE(LL, 1) GGCASE(LL, 2) GGCASE(LL, 3) GGCASE(LL, 4)

extern "C" int bsprobe_group_any_grouped(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV,
                                         const uint32_t *Bhi, const uint32_t *Blo, uint32_t *any_grouped, uint32_t *top_or,
                                         uint32_t *avg)
{
    GGCASE_L(5) GGCASE_L(6) GGCASE_L(7) GGCASE_L(8) GGCASE_L(9) GGCASE_L(10) GGCASE_L(11) GGCASE_L(12)
    GGCASE(11, 5) GGCASE(12, 5) GGCASE(12, 6)
    return 1;
}

/* ---- the crossings entry (tests/test_group_crossings.py) -----------------------------------------
 * window_group_any_grouped, window_group_any_crossings (from the middle, what the shift-record kernel runs) and its
 * one-direction form on the planes given; AVg[2] is taken as it comes (any words, not only table-built ones).  Returns 1
 * for an (L, d) outside the device table, 2 for one whose threshold is not the top plane. */
template <int W, int L, int D, int GRP>
static int run_group_any_crossings(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                   const uint32_t *Blo, uint32_t *any_grouped, uint32_t *any_crossings, uint32_t *any_one_way)
{
    if constexpr (!top_plane_serves(L, D)) {
        return 2;
    } else {
        window_group_any_grouped<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_grouped);
        window_group_any_crossings<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_crossings);
        window_group_any_crossings<W, L, D, GRP, false>(Ahi, Alo, AVg, Bhi, Blo, any_one_way);
        return 0;
    }
}

#define XCASE(LL, DD) \
    if (L == LL && d == DD) return run_group_any_crossings<10, LL, DD, 5>(Ahi, Alo, AVg, Bhi, Blo, any_grouped, any_crossings, any_one_way);
#define XCASE_L(LL) XCASE(LL, 0) XCASE(LL, 1) XCASE(LL, 2) XCASE(LL, 3) XCASE(LL, 4)

extern "C" int bsprobe_group_any_crossings(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg,
                                           const uint32_t *Bhi, const uint32_t *Blo, uint32_t *any_grouped,
                                           uint32_t *any_crossings, uint32_t *any_one_way)
{
    XCASE_L(5) XCASE_L(6) XCASE_L(7) XCASE_L(8) XCASE_L(9) XCASE_L(10) XCASE_L(11) XCASE_L(12)
    XCASE(11, 5) XCASE(12, 5) XCASE(12, 6)
    return 1;
}

/* ---- the centres entry (tests/test_group_centres.py) ----------------------------------------------
 * window_group_any_grouped and window_group_any_centres (what the shift-record kernel runs: no counter, each group from its
 * centre window) on the planes given; AVg[2] is taken as it comes.  Return codes as bsprobe_group_any_crossings. */
template <int W, int L, int D, int GRP>
static int run_group_any_centres(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                 const uint32_t *Blo, uint32_t *any_grouped, uint32_t *any_centres)
{
    if constexpr (!top_plane_serves(L, D)) {
        return 2;
    } else {
        window_group_any_grouped<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_grouped);
        window_group_any_centres<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_centres);
        return 0;
    }
}

#define CCASE(LL, DD) \
    if (L == LL && d == DD) return run_group_any_centres<10, LL, DD, 5>(Ahi, Alo, AVg, Bhi, Blo, any_grouped, any_centres);
#define CCASE_L(LL) CCASE(LL, 0) CCASE(LL, 1) CCASE(LL, 2) CCASE(LL, 3) CCASE(LL, 4)

extern "C" int bsprobe_group_any_centres(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg,
                                         const uint32_t *Bhi, const uint32_t *Blo, uint32_t *any_grouped, uint32_t *any_centres)
{
    CCASE_L(5) CCASE_L(6) CCASE_L(7) CCASE_L(8) CCASE_L(9) CCASE_L(10) CCASE_L(11) CCASE_L(12)
    CCASE(11, 5) CCASE(12, 5) CCASE(12, 6)
    return 1;
}

/* ---- the centres entry's two forms (tests/test_shared_trees.py) ------------------------------------
 * window_group_any_grouped, window_group_any_centres as the shift-record kernel runs it (the two centre trees share their
 * overlap, the top half adder folded into the threshold) and its private-trees form (SHARED = false: the build with
 * -DGKM_BS_CENTRES=1) on the planes given; AVg[2] is taken as it comes.  Return codes as bsprobe_group_any_crossings. */
template <int W, int L, int D, int GRP>
static int run_group_any_centres_forms(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                       const uint32_t *Blo, uint32_t *any_grouped, uint32_t *any_shared, uint32_t *any_private)
{
    if constexpr (!top_plane_serves(L, D)) {
        return 2;
    } else {
        window_group_any_grouped<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_grouped);
        window_group_any_centres<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_shared);
        window_group_any_centres<W, L, D, GRP, false>(Ahi, Alo, AVg, Bhi, Blo, any_private);
        return 0;
    }
}

#define FCASE(LL, DD) \
    if (L == LL && d == DD) return run_group_any_centres_forms<10, LL, DD, 5>(Ahi, Alo, AVg, Bhi, Blo, any_grouped, any_shared, any_private);
#define FCASE_L(LL) FCASE(LL, 0) FCASE(LL, 1) FCASE(LL, 2) FCASE(LL, 3) FCASE(LL, 4)

extern "C" int bsprobe_group_any_centres_forms(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg,
                                               const uint32_t *Bhi, const uint32_t *Blo, uint32_t *any_grouped,
                                               uint32_t *any_shared, uint32_t *any_private)
{
    FCASE_L(5) FCASE_L(6) FCASE_L(7) FCASE_L(8) FCASE_L(9) FCASE_L(10) FCASE_L(11) FCASE_L(12)
    FCASE(11, 5) FCASE(12, 5) FCASE(12, 6)
    return 1;
}

/* ---- the centres entry's shift-shared form (tests/test_shift_shared_trees.py) -----------------------
 * window_group_any_grouped and the three forms of window_group_any_centres -- shift-shared (SHIFTED = true, what the shift-record
 * kernel runs), shared and private -- on the planes given; AVg[2] is taken as it comes.  *taken: is the shift-shared form compiled
 * for this (L, d) (shift_shared_serves), or does SHIFTED = true stay on the shared form?  Return codes as
 * bsprobe_group_any_crossings. */
template <int W, int L, int D, int GRP>
static int run_group_any_shift_shared(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                      const uint32_t *Blo, uint32_t *any_grouped, uint32_t *any_shifted, uint32_t *any_shared,
                                      uint32_t *any_private, int *taken)
{
    if constexpr (!top_plane_serves(L, D)) {
        return 2;
    } else {
        window_group_any_grouped<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_grouped);
        window_group_any_centres<W, L, D, GRP, true, true>(Ahi, Alo, AVg, Bhi, Blo, any_shifted);
        window_group_any_centres<W, L, D, GRP>(Ahi, Alo, AVg, Bhi, Blo, any_shared);
        window_group_any_centres<W, L, D, GRP, false>(Ahi, Alo, AVg, Bhi, Blo, any_private);
        *taken = shift_shared_serves(W, L, D, GRP) ? 1 : 0;
        return 0;
    }
}

#define HCASE(LL, DD) \
    if (L == LL && d == DD) return run_group_any_shift_shared<10, LL, DD, 5>(Ahi, Alo, AVg, Bhi, Blo, any_grouped, any_shifted, any_shared, any_private, taken);
#define HCASE_L(LL) HCASE(LL, 0) HCASE(LL, 1) HCASE(LL, 2) HCASE(LL, 3) HCASE(LL, 4)

extern "C" int bsprobe_group_any_shift_shared(int L, int d, const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg,
                                              const uint32_t *Bhi, const uint32_t *Blo, uint32_t *any_grouped,
                                              uint32_t *any_shifted, uint32_t *any_shared, uint32_t *any_private, int *taken)
{
    HCASE_L(5) HCASE_L(6) HCASE_L(7) HCASE_L(8) HCASE_L(9) HCASE_L(10) HCASE_L(11) HCASE_L(12)
    HCASE(11, 5) HCASE(12, 5) HCASE(12, 6)
    return 1;
}

/* the table builders, for the same test: the three planes of a row segment (out[plane * W + w]) ... */
extern "C" void bsprobe_row_planes(const uint8_t *codes, int len, int s0, int W, int L, uint32_t *out)
{
    for (int pl = 0; pl < 3; pl++)
        for (int w = 0; w < W; w++) out[pl * W + w] = row_plane_word(codes, len, s0, w, W, L, pl);
}
/* ... words 0 .. nx-1 of a column strand's two bit planes ... */
extern "C" void bsprobe_sb_words(const uint8_t *codes, int T, int strand, int W, int L, int nx, uint32_t *hi, uint32_t *lo)
{
    for (int x = 0; x < nx; x++) {
        hi[x] = sb_word(codes, T, strand, x, W, L, 0);
        lo[x] = sb_word(codes, T, strand, x, W, L, 1);
    }
}
/* ... and the validity plane that one piece (bit rows b0 .. b0+nb-1, cnt owned windows) contributes to a packed lane */
extern "C" void bsprobe_piece_valid(int b0, int nb, int cnt, int W, uint32_t *out)
{
    for (int w = 0; w < W; w++) {
        out[w] = 0u;
        for (int b = 0; b < 32; b++) out[w] |= piece_bit((const uint8_t *)nullptr, 0, b0, nb, 0, cnt, b, w, W, 2) << b;
    }
}

/* ---- packed lanes: several row sequences against one column sequence ------------------------
 * Packs the rows with gkmpack::pack_rows, checks the packing invariants, builds every lane's
 * planes from its pieces, runs the lane program and attributes each hit to its piece's row.
 * P_out[i*(d+1)+m] for row i.  Returns 0, or a negative code naming the violated invariant. */
/* shift_trip > 0: the hits take the way of k_gram_bitslice's SHIFT RECORDS (gkm_bitslice.h shift_record_visit) -- per shift
 * the two group ORs that the kernel's counting loop computes, one push per shift with a hit, a stack per lane and strand,
 * trips over the shift_trip records on top as soon as the stack holds that many (visit, re-push what is left), the stack
 * emptied at the end of the strand; a visit resolves the hits among the five windows of its (bit row, group).
 * visits_out[0..2]: records pushed, visits made, records put back. */
template <int W, int L, int D>
static int run_packed(const uint8_t *codes, const int64_t *off, const int *rows, int nrows, int col,
                      const uint8_t *wd, int32_t *P_out, int *lanes_used, int max_rows = gkmpack::MAX_ROWS, int own_mult = 1,
                      int rider_w = 0, int shift_trip = 0, long long *visits_out = nullptr)
{
    using namespace gkmpack;
    std::vector<int> nwin((size_t)nrows);
    for (int i = 0; i < nrows; i++) nwin[(size_t)i] = (int)(off[rows[i] + 1] - off[rows[i]]) - L + 1;
    const Packing P = pack_rows(rows, nwin.data(), nrows, W, L, max_rows, 0, own_mult, rider_w);
    *lanes_used = (int)P.lanes_used;
    /* invariants: every window of every row owned exactly once; pieces inside their lane; all
     * pieces of a row in one tile; limits respected */
    std::vector<std::vector<int>> owned((size_t)nrows);
    for (int i = 0; i < nrows; i++) owned[(size_t)i].assign((size_t)nwin[(size_t)i], 0);
    std::vector<int> row_tile((size_t)nrows, -1);
    std::vector<int> lane_bits((size_t)P.ntiles * LANES, 0), lane_np((size_t)P.ntiles * LANES, 0);
    for (const Piece &pc : P.pieces) {
        if (pc.b0 < 0 || pc.nb <= 0 || pc.b0 + pc.nb > 32) return -1;
        if (pc.cnt <= 0 || pc.cnt > pc.nb * W - (L - 1)) return -2;
        if (pc.rider ? pc.b0 < lane_bits[(size_t)pc.lane] : pc.b0 != lane_bits[(size_t)pc.lane]) return -3; /* contiguous, in order */
        lane_bits[(size_t)pc.lane] = pc.b0 + pc.nb;
        if (++lane_np[(size_t)pc.lane] > MAX_PIECES) return -4;
        const int t = pc.lane / LANES;
        const int i = P.tile_out[(size_t)t * MAX_ROWS + pc.slot];
        if (i < 0 || i >= nrows || rows[i] != pc.row || P.tile_row[(size_t)t * MAX_ROWS + pc.slot] != pc.row) return -5;
        if (row_tile[(size_t)i] >= 0 && row_tile[(size_t)i] != t) return -6;
        row_tile[(size_t)i] = t;
        for (int k = 0; k < pc.cnt; k++) {
            if (pc.p0 + k >= nwin[(size_t)i]) return -7;
            owned[(size_t)i][(size_t)(pc.p0 + k)]++;
        }
    }
    for (int i = 0; i < nrows; i++)
        for (int v : owned[(size_t)i])
            if (v != 1) return -8;
    for (int t = 0; t < P.ntiles; t++)
        if (P.tile_nrows[(size_t)t] > MAX_ROWS) return -9;

    /* the computation */
    constexpr int NB = planes_for(D);
    (void)NB;
    const uint8_t *B = codes + off[col];
    const int T = (int)(off[col + 1] - off[col]), nB = T - L + 1;
    std::vector<uint32_t> sb[2][2];
    for (int st = 0; st < 2; st++)
        for (int pl = 0; pl < 2; pl++) {
            sb[st][pl].resize((size_t)T + W);
            for (int x = 0; x < T + W; x++) sb[st][pl][(size_t)x] = sb_word(B, T, st, x, W, L, pl);
        }
    auto wdist = [&](int Dd) { return wd ? (uint32_t)wd[Dd] : 1u; };
    const int pkw = (T + 15) / 16 + 1;
    std::vector<uint32_t> pkB[2];
    for (int st = 0; st < 2; st++) {
        pkB[st].resize((size_t)pkw);
        for (int x = 0; x < pkw; x++) pkB[st][(size_t)x] = pk_word(B, T, st, x);
    }
    const uint32_t rcpT = mod_magic((uint32_t)T);
    std::vector<uint32_t> acc((size_t)nrows * (D + 1), 0u);
    size_t pi = 0;
    while (pi < P.pieces.size()) {
        size_t pj = pi;
        while (pj < P.pieces.size() && P.pieces[pj].lane == P.pieces[pi].lane) pj++;
        uint32_t Ahi[W], Alo[W], AV[W], start_mask = 0u;
        uint32_t lanepk[2 * W + 2]; /* the lane's packed positions (what k_build_rowplanes writes as plane 3) */
        for (int w = 0; w < W; w++) Ahi[w] = Alo[w] = AV[w] = 0u;
        for (int x = 0; x < 2 * W + 2; x++) lanepk[x] = 0u;
        for (size_t k = pi; k < pj; k++) {
            const Piece &pc = P.pieces[k];
            start_mask |= 1u << pc.b0;
            const uint8_t *seq = codes + off[pc.row];
            const int len = (int)(off[pc.row + 1] - off[pc.row]);
            for (int w = 0; w < W; w++)
                for (int b = 0; b < 32; b++) {
                    Ahi[w] |= piece_bit(seq, len, pc.b0, pc.nb, pc.p0, pc.cnt, b, w, W, 0) << b;
                    Alo[w] |= piece_bit(seq, len, pc.b0, pc.nb, pc.p0, pc.cnt, b, w, W, 1) << b;
                    AV[w] |= piece_bit(seq, len, pc.b0, pc.nb, pc.p0, pc.cnt, b, w, W, 2) << b;
                    const int i = b * W + w;
                    lanepk[i >> 4] |= ((piece_bit(seq, len, pc.b0, pc.nb, pc.p0, pc.cnt, b, w, W, 0) << 1) |
                                       piece_bit(seq, len, pc.b0, pc.nb, pc.p0, pc.cnt, b, w, W, 1)) << (2 * (i & 15));
                }
        }
        /* one hit: bit row `bit` of word w of the shift (delta, st); -20 if a flagged window exceeds D */
        auto resolve = [&](int bit, int w, int delta, int st) -> int {
                        const Piece &pc = P.pieces[pi + (size_t)piece_of_bitrow(start_mask, bit)];
                        const uint8_t *seq = codes + off[pc.row];
                        const int len = (int)(off[pc.row + 1] - off[pc.row]), nA = len - L + 1;
                        /* the device keeps c0 = nA/2 - p0 + b0*W per piece: the row l-mer of lane position i0 is
                         * l-mer p = p0 + i0 - b0*W of its sequence, |c0 - i0| away from the centre l-mer */
                        auto rl = [&](int i0) { return pk_window(lanepk[i0 >> 4], lanepk[(i0 >> 4) + 1], i0); };
                        auto cl = [&](int s2, int q) { return pk_window(pkB[s2][(size_t)(q >> 4)], pkB[s2][(size_t)(q >> 4) + 1], q); };
                        const int c0 = nA / 2 - pc.p0 + pc.b0 * W;
                        (void)seq;
                        const HitValue hv = resolve_hit_packed<W>(bit, w, delta, st, (uint32_t)T, rcpT, nB, L, c0, rl, cl, wdist);
                        const int i = P.tile_out[(size_t)(pc.lane / LANES) * MAX_ROWS + pc.slot];
                        if (hv.m <= D) acc[(size_t)i * (D + 1) + hv.m] += hv.v;
                        else if (hv.v != 0u) return -20; /* a true hit can never exceed D */
                        return 0;
        };
        if constexpr (W == 2 * SHIFT_GROUP_WORDS) {
            if (shift_trip > 0) {
                struct Rec { uint32_t any0, any1, origin; };
                uint32_t AVg[2] = {0u, 0u};
                for (int w = 0; w < W; w++) AVg[w / SHIFT_GROUP_WORDS] |= AV[w];
                for (int st = 0; st < 2; st++) {
                    std::vector<Rec> stack;
                    auto trip = [&](size_t c) -> int { /* the c records on top: one visit each, the live ones go back */
                        std::vector<Rec> top(stack.end() - (long)c, stack.end());
                        stack.resize(stack.size() - c);
                        for (Rec r : top) {
                            const ShiftVisit v = shift_record_visit(r.any0, r.any1);
                            const int delta = rec_delta(r.origin);
                            if (rec_w(r.origin) != 0) return -21; /* a shift record's origin carries no word index */
                            uint32_t hit[W];
                            window_hits<W, L, D>(Ahi, Alo, AV, &sb[st][0][(size_t)delta], &sb[st][1][(size_t)delta],
                                                 (const uint32_t *)nullptr, hit);
                            for (int k = 0; k < SHIFT_GROUP_WORDS; k++)
                                if ((hit[v.w0 + k] >> v.bit) & 1u)
                                    if (const int rc = resolve((int)v.bit, (int)v.w0 + k, delta, st)) return rc;
                            if (visits_out) visits_out[1]++;
                            if (shift_record_live(r.any0, r.any1)) {
                                stack.push_back(r);
                                if (visits_out) visits_out[2]++;
                            }
                        }
                        return 0;
                    };
                    for (int delta = 0; delta < T; delta++) {
                        uint32_t any[2];
                        if constexpr (top_plane_serves(L, D)) /* (the shift-record kernel's entry: a superset per group) */
                            window_group_any_centres<W, L, D, SHIFT_GROUP_WORDS, true, true>(Ahi, Alo, AVg, &sb[st][0][(size_t)delta],
                                                                                             &sb[st][1][(size_t)delta], any);
                        else
                            window_group_any<W, L, D, SHIFT_GROUP_WORDS>(Ahi, Alo, AV, &sb[st][0][(size_t)delta],
                                                                         &sb[st][1][(size_t)delta], any);
                        if (shift_record_live(any[0], any[1])) {
                            stack.push_back(Rec{any[0], any[1], pack_meta(delta, 0, 0)});
                            if (visits_out) visits_out[0]++;
                        }
                        while (stack.size() >= (size_t)shift_trip)
                            if (const int rc = trip((size_t)shift_trip)) return rc;
                    }
                    while (!stack.empty()) /* the strand's last trips: full ones, then the partial one */
                        if (const int rc = trip(std::min(stack.size(), (size_t)shift_trip))) return rc;
                }
                pi = pj;
                continue;
            }
        }
        for (int st = 0; st < 2; st++)
            for (int delta = 0; delta < T; delta++) {
                uint32_t hit[W];
                window_hits<W, L, D>(Ahi, Alo, AV, &sb[st][0][(size_t)delta], &sb[st][1][(size_t)delta],
                                     (const uint32_t *)nullptr, hit);
                for (int w = 0; w < W; w++) {
                    uint32_t h = hit[w];
                    while (h) {
                        const int bit = __builtin_ctz(h);
                        h &= h - 1u;
                        if (const int rc = resolve(bit, w, delta, st)) return rc;
                    }
                }
            }
        pi = pj;
    }
    for (size_t k = 0; k < acc.size(); k++) P_out[k] = (int32_t)acc[k];
    return 0;
}

#define PCASE(WW, LL, DD) \
    if (W == WW && L == LL && d == DD) return run_packed<WW, LL, DD>(codes, off, rows, nrows, col, wd, P, lanes_used);

extern "C" int bsprobe_profile_packed(int W, int L, int d, const uint8_t *codes, const int64_t *off, const int *rows,
                                      int nrows, int col, const uint8_t *wd, int32_t *P, int *lanes_used)
{
    PCASE(10, 11, 3) PCASE(20, 11, 3) PCASE(10, 12, 4) PCASE(20, 12, 4) PCASE(20, 10, 3) PCASE(10, 6, 2) PCASE(20, 6, 2)
    PCASE(5, 11, 3)
    return 1;
}

/* The same with the packing of a same-length launch that carries RIDERS (gkm_pack.h RIDER_B0; 64 residents per tile, pieces
 * of whole groups of five, riders of RIDER_W windows): the rider pieces go through the lane program as pieces like any
 * other -- their bits in the planes, their windows attributed to their row. */
#define RCASE(WW, LL, DD) \
    if (W == WW && L == LL && d == DD) \
        return run_packed<WW, LL, DD>(codes, off, rows, nrows, col, wd, P, lanes_used, 64, 5, gkmpack::RIDER_W);
extern "C" int bsprobe_profile_riders(int W, int L, int d, const uint8_t *codes, const int64_t *off, const int *rows,
                                      int nrows, int col, const uint8_t *wd, int32_t *P, int *lanes_used)
{
    RCASE(10, 11, 3) RCASE(10, 10, 3)
    return 1;
}

/* The lane program with SHIFT RECORDS between the counting and the hit path (run_packed's shift_trip), over the packing of a
 * same-length launch: 64 residents per tile, whole groups of five, with riders (riders != 0) or without.  trip = records a
 * trip takes (the kernel: 64, one per lane; here per lane, so small values exercise the re-push order too). */
#define SCASE(LL, DD) \
    if (L == LL && d == DD) \
        return run_packed<10, LL, DD>(codes, off, rows, nrows, col, wd, P, lanes_used, 64, 5, riders ? gkmpack::RIDER_W : 0, trip, visits);
extern "C" int bsprobe_profile_shift_records(int L, int d, const uint8_t *codes, const int64_t *off, const int *rows, int nrows,
                                             int col, const uint8_t *wd, int riders, int trip, int32_t *P, int *lanes_used,
                                             long long *visits)
{
    if (trip <= 0) return 1;
    SCASE(11, 3) SCASE(10, 3) SCASE(12, 4)
    return 1;
}

/* One record through shift_record_visit until it is empty: the (bit row, first word) of every visit, in order; returns the
 * number of visits (at most 64) */
extern "C" int bsprobe_shift_record_drain(uint32_t any0, uint32_t any1, int *bits_out, int *w0_out)
{
    int n = 0;
    while (shift_record_live(any0, any1) && n < 64) {
        const ShiftVisit v = shift_record_visit(any0, any1);
        bits_out[n] = (int)v.bit;
        w0_out[n] = (int)v.w0;
        n++;
    }
    return n;
}
extern "C" unsigned bsprobe_lowest_bit_or_ones(uint32_t x) { return lowest_bit_or_ones(x); }

/* The packing of a same-length launch as gkm_gram.hip plan_bitslice asks for it (W = 10 words, 64 residents per tile, whole
 * groups of five; rider_w = 0: without riders), for tests/test_rider_packing.py.  pieces_out[k][8] = lane, b0, nb, slot,
 * row, p0, cnt, rider; tags_out[k] = the rider pieces' tag words (0 for residents); tile_rows_out[t][MAX_ROWS],
 * tile_outs_out likewise; tile_nrows_out[t].  *check_out = same_length_packing_check.  Returns the number of pieces, or
 * -1 if the arrays are too small; *ntiles_out the tiles. */
extern "C" int packprobe_same_length(const int *rows, const int *nwin, int nrows, int L, int rider_w, int split_jump,
                                     int *pieces_out, int max_pieces, int *tags_out, int *tile_rows_out, int *tile_outs_out,
                                     int *tile_nrows_out, int max_tiles, int *ntiles_out, int *nriders_out, int *check_out)
{
    using namespace gkmpack;
    const int W = 10, own_mult = 5;
    const Packing P = pack_rows(rows, nwin, nrows, W, L, 64, split_jump, own_mult, rider_w);
    *ntiles_out = P.ntiles;
    *nriders_out = P.nriders;
    if ((int)P.pieces.size() > max_pieces || P.ntiles > max_tiles) return -1;
    std::vector<int> rw(P.pieces.size());
    for (size_t k = 0; k < P.pieces.size(); k++) {
        const Piece &pc = P.pieces[k];
        int *o = pieces_out + k * 8;
        o[0] = pc.lane; o[1] = pc.b0; o[2] = pc.nb; o[3] = pc.slot; o[4] = pc.row; o[5] = pc.p0; o[6] = pc.cnt; o[7] = pc.rider;
        tags_out[k] = pc.rider ? (int)pack_rider_tag(pc.slot, pc.p0 - RIDER_B0 * W) : 0;
        rw[k] = nwin[P.tile_out[(size_t)(pc.lane / LANES) * MAX_ROWS + pc.slot]];
    }
    for (int t = 0; t < P.ntiles; t++) {
        tile_nrows_out[t] = P.tile_nrows[(size_t)t];
        for (int r = 0; r < MAX_ROWS; r++) {
            tile_rows_out[t * MAX_ROWS + r] = P.tile_row[(size_t)t * MAX_ROWS + r];
            tile_outs_out[t * MAX_ROWS + r] = P.tile_out[(size_t)t * MAX_ROWS + r];
        }
    }
    *check_out = same_length_packing_check(P, rw.data(), own_mult, rider_w, rider_w > 0 ? RIDER_SLOTS : 64);
    return (int)P.pieces.size();
}

/* Tiles of the packing as plan_bitslice asks for it (W = 10, whole groups of five, no riders) with max_rows row slots per
 * tile: the plan packs with 64 and with MAX_ROWS and takes the wider tiles where they are fewer
 * (tests/test_same_length_plan_host.py) */
extern "C" int packprobe_plan_tiles(const int *rows, const int *nwin, int nrows, int L, int max_rows)
{
    return gkmpack::pack_rows(rows, nwin, nrows, 10, L, max_rows, 0, 5, 0).ntiles;
}

/* One lane's image as k_build_rowplanes builds it from the lane's pieces (pieces[k][8] as above): planes_out[3][W] (hi, lo,
 * window ownership) and pk_out[2 W + 2], the 2-bit packed positions. */
extern "C" void packprobe_lane_image(const uint8_t *codes, const int64_t *off, const int *pieces, int npieces, int W,
                                     uint32_t *planes_out, uint32_t *pk_out)
{
    for (int x = 0; x < 3 * W; x++) planes_out[x] = 0u;
    for (int x = 0; x < 2 * W + 2; x++) pk_out[x] = 0u;
    for (int k = 0; k < npieces; k++) {
        const int *pc = pieces + k * 8;
        const uint8_t *seq = codes + off[pc[4]];
        const int len = (int)(off[pc[4] + 1] - off[pc[4]]);
        for (int w = 0; w < W; w++)
            for (int b = 0; b < 32; b++) {
                uint32_t bits[3];
                for (int pl = 0; pl < 3; pl++) {
                    bits[pl] = piece_bit(seq, len, pc[1], pc[2], pc[5], pc[6], b, w, W, pl);
                    planes_out[pl * W + w] |= bits[pl] << b;
                }
                const int i = b * W + w;
                pk_out[i >> 4] |= ((bits[0] << 1) | bits[1]) << (2 * (i & 15));
            }
    }
}

/* gkm_pack.h same_length_packing_check -- what plan_bitslice calls before a same-length launch -- on a layout handed in as
 * pieces[k][8] (sorted by lane, then bit row), every row with row_windows l-mers: 0, or the code of the first failure */
extern "C" int packprobe_check_layout(const int *pieces, int npieces, int row_windows, int L, int rider_w, int max_slots)
{
    gkmpack::Packing P;
    P.W = 10;
    P.L = L;
    std::vector<int> rw((size_t)npieces, row_windows);
    for (int k = 0; k < npieces; k++) {
        const int *o = pieces + k * 8;
        gkmpack::Piece pc;
        pc.lane = o[0]; pc.b0 = o[1]; pc.nb = o[2]; pc.slot = o[3]; pc.row = o[4]; pc.p0 = o[5]; pc.cnt = o[6]; pc.rider = o[7];
        P.pieces.push_back(pc);
    }
    return gkmpack::same_length_packing_check(P, rw.data(), 5, rider_w, max_slots);
}

extern "C" int packprobe_rider_tag_slot(int tag) { return rider_tag_slot((uint32_t)tag); }
extern "C" int packprobe_rider_tag_pos(int tag) { return rider_tag_pos((uint32_t)tag); }
extern "C" int packprobe_rider_consts(int which)
{
    return which == 0 ? gkmpack::RIDER_B0 : which == 1 ? gkmpack::RIDER_NB : which == 2 ? gkmpack::RIDER_W : gkmpack::RIDER_SLOTS;
}

/* ---- row sharding layout (gkm_shard.h) for tests/test_sharding.py ---- */
#include "gkm_shard.h"

extern "C" int shardprobe_chunk_rows(int n, int world, int chunks) { return gkmshard::chunk_rows(n, world, chunks); }

extern "C" int shardprobe_part(int n, int world, int rank, int chunks, int chunk, int *rows_out)
{
    const std::vector<std::vector<int>> parts = gkmshard::chunked_layout(n, world, rank, chunks);
    const std::vector<int> &p = parts[(size_t)chunk];
    for (size_t i = 0; i < p.size(); i++) rows_out[i] = p[i];
    return (int)p.size();
}

extern "C" void shardprobe_gather_index(int n, int world, int chunks, int64_t *slot_out)
{
    const std::vector<int64_t> s = gkmshard::chunked_gather_index(n, world, chunks);
    for (int i = 0; i < n; i++) slot_out[i] = s[(size_t)i];
}

extern "C" long long shardprobe_packed_chunk_elems(int n, int world, int chunks)
{
    return (long long)gkmshard::packed_chunk_elems(n, world, chunks);
}

extern "C" void shardprobe_packed_gather_offsets(int n, int world, int chunks, int64_t *off_out)
{
    const std::vector<int64_t> s = gkmshard::packed_gather_offsets(n, world, chunks);
    for (int i = 0; i < n; i++) off_out[i] = s[(size_t)i];
}

extern "C" int shardprobe_auto_chunks(int n, int world) { return gkmshard::auto_chunks(n, world); }

/* work items (tile, column) of a triangular launch over `rows` packed with / without closing tiles at jumps in the row
 * list (gkm_pack.h pack_rows split_jump), and the number of tiles; every row must have found a slot */
extern "C" long long packprobe_triangle_items(const int *rows, const int *nwin, int nrows, int W, int L, int max_rows,
                                              int split_jump, int *ntiles_out)
{
    const gkmpack::Packing P = gkmpack::pack_rows(rows, nwin, nrows, W, L, max_rows, split_jump);
    long placed = 0;
    for (int t = 0; t < P.ntiles; t++) placed += P.tile_nrows[(size_t)t];
    if (placed != nrows) return -1;
    if (ntiles_out) *ntiles_out = P.ntiles;
    return gkmpack::triangle_items(P);
}
