/*
 * gkm_bitslice.h -- the bit-sliced "diagonal" formulation of the gkm mismatch profile.
 *
 * What the reference computes with a k-mer tree DFS (src/libgkm.c:315-387) is, for a
 * pair of sequences (a, b), the histogram over all l-mer pairs (p, q) of their Hamming
 * distance m <= d, weighted by w_a[p] * w_b[q].
 *
 * Observation: mm(p, q) = sum_{i<L} [a[p+i] != b[q+i]] is a sliding-window sum along a
 * DIAGONAL (q - p = const) of the base-level mismatch matrix.  So instead of comparing
 * l-mers one by one (>= 5 integer ops per comparison) we
 *   1. hold a row SEGMENT of up to 32*W bases as two bit planes (hi/lo bit of the 2-bit
 *      base code) in a STRIDED layout: base i of the segment is bit (i / W) of word (i % W);
 *   2. for a cyclic shift `delta` of the column sequence b (period T = len(b)) take the
 *      same strided layout of b[(i + delta) mod T]  -- these words are precomputed once per
 *      column sequence ("SB table"), are uniform across a wavefront and live in SGPRs;
 *   3. mismatch bits Z[w] = (Ahi[w]^Bhi[w]) | (Alo[w]^Blo[w]): 32 base comparisons in 3 ops;
 *   4. in the strided layout "next base" = "next word", so the L-window sum over bases
 *      i..i+L-1 is a sum over L CONSECUTIVE WORDS (no funnel shifts); it is evaluated
 *      bit-sliced (one bit plane per binary digit of the count, 32 windows per op) by a
 *      sliding power-of-two tree  w2[x]=Z[x]+Z[x+1], w4[x]=w2[x]+w2[x+2], w8[x]=w4[x]+w4[x+4];
 *   5. counts are kept in NB planes + a sticky overflow plane; windows with count <= d and
 *      a valid start on both sides are the HITS (about 0.1-0.4 % of all windows on iid
 *      sequences), the only places where weights are touched.  window_hits thresholds a count of
 *      MISMATCHES (count <= d: no plane from bitlen(d) up is set); the kernel's entry,
 *      window_group_any, counts MATCHES plus a constant bias wherever that makes the threshold the
 *      top count plane alone ((L, d) = (11,3), (10,3), (12,4) among others), and hands back the
 *      OR of the hits over a group of words: one op per word for threshold, validity and OR.
 * Cost: ~1.1-1.4 integer VALU ops per l-mer comparison instead of ~5-6.
 *
 * Everything here is plain C++ on uint32_t so that the very same code runs per lane on
 * the GPU and in the CPU unit test (tests/test_bitslice_core.py via csrc/bitslice_cpu_probe.cpp).
 */
#ifndef GKM_BITSLICE_H
#define GKM_BITSLICE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GKM_HD __host__ __device__ __forceinline__
#else
#define GKM_HD inline
#endif

namespace gkmbs {

/* number of count planes needed to represent 0..d exactly */
constexpr int planes_for(int d) { return d <= 1 ? 1 : d <= 3 ? 2 : d <= 7 ? 3 : 4; }

/* window starts a full row segment of W words contributes (its last L-1 bases only
 * complete windows of the segment's own starts; the next segment begins here) */
constexpr int segment_capacity(int W, int L) { return 32 * W - (L - 1); }

/* ------------------------------------------------------------------ lop3 */
/* Any 3-input bitwise function in one full-rate VALU op: gfx950's v_bitop3_b32.  TT is the
 * truth table f(0xF0, 0xCC, 0xAA).  (v_and_or_b32 / v_or3_b32 issue at HALF rate on MI355X,
 * v_bitop3_b32 at full rate -- tools/valu_peak.hip -- so every 3-input op below is a lop3.) */
template <int TT>
GKM_HD uint32_t lop3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    uint32_t r = 0u;
    for (int k = 0; k < 8; k++)
        if ((TT >> k) & 1) r |= ((k & 4) ? a : ~a) & ((k & 2) ? b : ~b) & ((k & 1) ? c : ~c);
    return r;
#endif
}
constexpr int TT_XOR3 = 0x96;     /* a ^ b ^ c */
constexpr int TT_MAJ = 0xE8;      /* majority(a, b, c) */
constexpr int TT_OR3 = 0xFE;      /* a | b | c */
constexpr int TT_A_OR_BXC = 0xF6; /* a | (b ^ c) */
constexpr int TT_NA_B_C = 0x08;   /* ~a & b & c */

constexpr int bitlen(int v)
{
    int n = 0;
    while (v) { n++; v >>= 1; }
    return n;
}

/* Bit-sliced count whose value is known (at compile time) to lie in 0..MX.  Only the planes
 * that can be non-zero exist; `ovf` exists (is meaningful) iff MX does not fit NB planes. */
template <int NB, int MX>
struct Cnt {
    static constexpr int P = bitlen(MX) < NB ? bitlen(MX) : NB;
    static constexpr bool OV = MX >= (1 << NB);
    uint32_t b[P > 0 ? P : 1];
    uint32_t ovf;
};

template <int PX, int PY, bool CIN>
constexpr bool carry_into(int i)
{
    return i == 0 ? CIN : (((i - 1 < PX) ? 1 : 0) + ((i - 1 < PY) ? 1 : 0) + (carry_into<PX, PY, CIN>(i - 1) ? 1 : 0)) >= 2;
}

template <int I, int NB, int M1, int M2, bool CIN>
GKM_HD void add_plane(const Cnt<NB, M1> &x, const Cnt<NB, M2> &y, uint32_t &c, Cnt<NB, M1 + M2 + (CIN ? 1 : 0)> &r)
{
    using X = Cnt<NB, M1>;
    using Y = Cnt<NB, M2>;
    using R = Cnt<NB, M1 + M2 + (CIN ? 1 : 0)>;
    if constexpr (I < R::P) {
        constexpr bool hx = I < X::P, hy = I < Y::P, hc = carry_into<X::P, Y::P, CIN>(I);
        constexpr int nin = (hx ? 1 : 0) + (hy ? 1 : 0) + (hc ? 1 : 0);
        /* the carry out of this plane is wanted by the next plane, or by ovf if this is plane NB-1 */
        constexpr bool want_c = nin >= 2 && ((I + 1 < R::P) || (I + 1 == NB && R::OV));
        if constexpr (nin == 3) {
            const uint32_t xi = x.b[I], yi = y.b[I], ci = c;
            r.b[I] = lop3<TT_XOR3>(xi, yi, ci);
            if constexpr (want_c) c = lop3<TT_MAJ>(xi, yi, ci);
        } else if constexpr (nin == 2) {
            const uint32_t u = hx ? x.b[hx ? I : 0] : y.b[hy ? I : 0];
            const uint32_t v = hc ? c : y.b[hy ? I : 0];
            r.b[I] = u ^ v;
            if constexpr (want_c) c = u & v;
        } else if constexpr (nin == 1) {
            r.b[I] = hx ? x.b[hx ? I : 0] : (hy ? y.b[hy ? I : 0] : c);
        } else {
            r.b[I] = 0u;
        }
    }
}

/* x + y (+ a one-bit carry-in plane): 2 ops per full-adder plane, 2 per half-adder plane */
template <bool CIN, int NB, int M1, int M2>
GKM_HD Cnt<NB, M1 + M2 + (CIN ? 1 : 0)> cnt_add(const Cnt<NB, M1> &x, const Cnt<NB, M2> &y, uint32_t cin = 0u)
{
    using X = Cnt<NB, M1>;
    using Y = Cnt<NB, M2>;
    using R = Cnt<NB, M1 + M2 + (CIN ? 1 : 0)>;
    R r;
    uint32_t c = cin;
    add_plane<0, NB, M1, M2, CIN>(x, y, c, r);
    add_plane<1, NB, M1, M2, CIN>(x, y, c, r);
    add_plane<2, NB, M1, M2, CIN>(x, y, c, r);
    add_plane<3, NB, M1, M2, CIN>(x, y, c, r);
    r.ovf = 0u;
    if constexpr (R::OV) {
        /* carry out of plane NB-1 exists iff that plane had >= 2 inputs */
        constexpr bool hc = R::P == NB && (((NB - 1 < X::P) ? 1 : 0) + ((NB - 1 < Y::P) ? 1 : 0) +
                                           (carry_into<X::P, Y::P, CIN>(NB - 1) ? 1 : 0)) >= 2;
        constexpr int terms = (X::OV ? 1 : 0) + (Y::OV ? 1 : 0) + (hc ? 1 : 0);
        if constexpr (terms == 3) r.ovf = lop3<TT_OR3>(x.ovf, y.ovf, c);
        else if constexpr (terms == 2) r.ovf = X::OV ? (x.ovf | (Y::OV ? y.ovf : c)) : (y.ovf | c);
        else if constexpr (terms == 1) r.ovf = X::OV ? x.ovf : (Y::OV ? y.ovf : c);
    }
    return r;
}

/* truth table of [value(b2 b1 b0) > D] for a lop3 over three count planes */
constexpr int tt_gt3(int D)
{
    int tt = 0;
    for (int k = 0; k < 8; k++)
        if (k > D) tt |= 1 << k;
    return tt;
}
/* truth table of [ovf | value(b1 b0) > D] with inputs (b1, b0, ovf) */
constexpr int tt_gt2_or(int D)
{
    int tt = 0;
    for (int k = 0; k < 8; k++)
        if ((k & 1) || ((k >> 1) > D)) tt |= 1 << k;
    return tt;
}

/* mask of positions where the count is NOT <= D (too many mismatches or overflowed) */
template <int D, int NB, int MX>
GKM_HD uint32_t cnt_exceeds(const Cnt<NB, MX> &v)
{
    using V = Cnt<NB, MX>;
    if constexpr (MX <= D) {
        return 0u;
    } else if constexpr (V::P <= 2) {
        const uint32_t b1 = V::P > 1 ? v.b[V::P > 1 ? 1 : 0] : 0u, b0 = V::P > 0 ? v.b[0] : 0u;
        if constexpr (D >= 3) return V::OV ? v.ovf : 0u;
        else return lop3<tt_gt2_or(D)>(b1, b0, V::OV ? v.ovf : 0u);
    } else if constexpr (V::P == 3) {
        if constexpr (D >= 7) return V::OV ? v.ovf : 0u;
        else {
            const uint32_t gt = lop3<tt_gt3(D)>(v.b[2], v.b[1], v.b[0]);
            return V::OV ? (gt | v.ovf) : gt;
        }
    } else if constexpr (((D + 1) & D) == 0 && D < 8) {
        /* D + 1 a power of two: "count > D" is the OR of the planes from log2(D+1) up */
        uint32_t gt;
        if constexpr (D == 7) gt = v.b[3];
        else if constexpr (D == 3) gt = v.b[3] | v.b[2];
        else if constexpr (D == 1) gt = lop3<TT_OR3>(v.b[3], v.b[2], v.b[1]);
        else gt = lop3<TT_OR3>(v.b[3], v.b[2], v.b[1]) | v.b[0];
        return V::OV ? (gt | v.ovf) : gt;
    } else {
        uint32_t gt;
        if constexpr (D >= 15) gt = 0u;
        else if constexpr (D >= 8) gt = v.b[3] & lop3<tt_gt3(D - 8)>(v.b[2], v.b[1], v.b[0]);
        else gt = v.b[3] | lop3<tt_gt3(D)>(v.b[2], v.b[1], v.b[0]);
        return V::OV ? (gt | v.ovf) : gt;
    }
}

constexpr int TT_A_AND_BXC = 0x60; /* a & (b ^ c) */
constexpr int TT_BXC_AND_AXC = 0x42; /* (b ^ c) & (a ^ c) */

/* Sum of N one-bit planes as an exact bit-sliced count, used once per shift for the first
 * window.  Column compression: the N planes of weight 1 are folded three at a time by full
 * adders (x ^ y ^ z stays in the column, maj(x, y, z) moves to the next), a half adder takes a
 * leftover pair; the N/2 carries are the next column.  A full adder takes one plane off the
 * total, so this is the minimum number of them: L = 11 -> 7 full adders + 1 half adder = 16
 * ops (the balanced tree of two-operand additions it replaces took 22). */
template <int N>
struct ColumnSum {
    static constexpr int NC = N / 2; /* carries out of a column of N planes */
    static GKM_HD uint32_t run(const uint32_t *x, uint32_t *carry)
    {
        uint32_t s = x[0];
        int nc = 0;
#pragma unroll
        for (int i = 1; i + 1 < N; i += 2) {
            carry[nc++] = lop3<TT_MAJ>(s, x[i], x[i + 1]);
            s = lop3<TT_XOR3>(s, x[i], x[i + 1]);
        }
        if constexpr (N % 2 == 0) {
            carry[nc++] = s & x[N - 1];
            s ^= x[N - 1];
        }
        return s;
    }
};

template <int I, int NB, int MX, int N>
GKM_HD void plane_sum_columns(const uint32_t *x, Cnt<NB, MX> &r)
{
    if constexpr (N >= 1 && I < Cnt<NB, MX>::P) {
        uint32_t carry[ColumnSum<N>::NC > 0 ? ColumnSum<N>::NC : 1];
        r.b[I] = ColumnSum<N>::run(x, carry);
        plane_sum_columns<I + 1, NB, MX, ColumnSum<N>::NC>(carry, r);
    }
}

template <int NB, int N>
struct PlaneSum {
    static_assert(bitlen(N) <= NB, "PlaneSum: the count must fit its planes");
    static GKM_HD Cnt<NB, N> run(const uint32_t *z)
    {
        Cnt<NB, N> r;
        r.ovf = 0u;
        plane_sum_columns<0, NB, N, N>(z, r);
        return r;
    }
};

/*
 * One cyclic shift of one column strand against one row segment.
 *   Ahi/Alo/AV : the segment's planes, W words each (per lane)
 *   Bhi/Blo/Bv : SB words x = delta .. delta+W-1 of the column strand (wave-uniform)
 * For w in [0,W): hit[w] = windows (bit b <-> segment base b*W + w) with <= D mismatches
 * whose start is valid on both sides.  With Bv == nullptr the column-side validity (the
 * window must not wrap around the end of the strand) is NOT applied here: the ~L/T of
 * windows concerned then yield a few candidate hits more, which resolve_hit() rejects --
 * one operand and one scalar-operand instruction less per word in the hot loop.
 * The exact count of a hit is recomputed from the l-mer tables when the hit is consumed
 * (cheaper than carrying the count planes along).
 *
 * Window counts: the first window (w = 0) is summed with an adder tree; every further window
 * differs from its left neighbour by one base entering and one leaving, so the exact
 * bit-sliced count is stepped by an up/down counter, 2 ops per count plane (1 for the last):
 *     t_0 = Zin ^ Zout;  b_i ^= t_i;  t_{i+1} = t_i & (b_i_old ^ Zout)
 * (carry when counting up through a 1, borrow when counting down through a 0).
 */
template <int W, int L, int D>
GKM_HD void window_hits(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV, const uint32_t *Bhi,
                        const uint32_t *Blo, const uint32_t *Bv, uint32_t *hit)
{
    static_assert(L >= 2 && L <= 12, "L out of range");
    constexpr int P = bitlen(L); /* planes of an exact count 0..L */
    constexpr int NX = W + L - 1;
    uint32_t Z[NX];
#pragma unroll
    for (int w = 0; w < W; w++) Z[w] = lop3<TT_A_OR_BXC>(Ahi[w] ^ Bhi[w], Alo[w], Blo[w]);
#pragma unroll
    for (int x = W; x < NX; x++) Z[x] = Z[x - W] >> 1; /* word x == word x-W one bit up */

    Cnt<P, L> cnt = PlaneSum<P, L>::run(Z);
#pragma unroll
    for (int w = 0; w < W; w++) {
        if (w > 0) {
            const uint32_t zout = Z[w - 1], zin = Z[w + L - 1];
            /* plane 0 straight from (b_0, Zin, Zout): b_0 ^ Zin ^ Zout and the carry/borrow
             * (Zin ^ Zout) & (b_0 ^ Zout), one lop3 each -- no separate Zin ^ Zout */
            const uint32_t old0 = cnt.b[0];
            cnt.b[0] = lop3<TT_XOR3>(old0, zin, zout);
            uint32_t t = lop3<TT_BXC_AND_AXC>(old0, zin, zout);
#pragma unroll
            for (int i = 1; i < P; i++) {
                const uint32_t old = cnt.b[i];
                cnt.b[i] = old ^ t;
                if (i + 1 < P) t = lop3<TT_A_AND_BXC>(t, old, zout);
            }
        }
        hit[w] = Bv ? lop3<TT_NA_B_C>(cnt_exceeds<D>(cnt), AV[w], Bv[w]) : (~cnt_exceeds<D>(cnt) & AV[w]);
    }
}

/*
 * The same shift as window_hits, but delivering what the kernel's hit list wants: per group of GRP consecutive words the
 * OR over the group of "window has <= D mismatches and a valid row-side start" (no column-side validity: window_hits with
 * Bv == nullptr is the specification -- any[g] == hit[g*GRP] | .. | hit[g*GRP + GRP-1] wherever AV is a plane the tables
 * build, see below).
 *
 * Where the bias allows it the count is kept in MATCHES: with M = L - c matches, c <= D is M >= L - D, and with the
 * constant beta = 2^(P-1) - (L - D) added once per shift (P = bitlen(L) planes), "hit" is M + beta >= 2^(P-1): THE TOP
 * PLANE ALONE, provided 0 <= beta and L + beta < 2^P (no wrap).  beta = 0 costs nothing, beta = 1 enters the first
 * window's column sum as a carry-in (ColumnSumBiased); larger biases keep the mismatch count.  (11,3): beta 0; (10,3):
 * beta 1; (12,4): beta 0.  Threshold, row validity and the group's OR are then ONE op per word, any | (top & AV[w]),
 * where the mismatch count needs ~(b3 | b2) & AV[w] per word and two three-input ORs per group of five.
 *   - match bits are the mismatch expression with the inverted truth table: one xor and one lop3 per word, as before;
 *   - the up/down counter does not care what it counts;
 *   - Z[x] = Z[x - W] >> 1 now shifts a MISMATCH into bit row 31 of the extension words (window_hits shifts a match in).
 *     Both are fiction about bases behind the lane's 32 * W; only windows i >= segment_capacity(W, L) see them, and no
 *     piece owns those (row_plane_word: i < cap; piece_bit: li < cnt <= nb * W - (L - 1)), so AV is 0 there and the two
 *     entries agree on every bit that a table-built AV lets through (tests/test_group_any.py).
 */
constexpr bool top_plane_serves(int L, int D)
{
    const int beta = (1 << (bitlen(L) - 1)) - (L - D);
    return (beta == 0 || beta == 1) && L + beta < (1 << bitlen(L));
}
constexpr int top_plane_bias(int L, int D) { return (1 << (bitlen(L) - 1)) - (L - D); }

constexpr int TT_NOT_A_OR_BXC = 0x09; /* ~(a | (b ^ c)) */
constexpr int TT_A_OR_BC = 0xF8;      /* a | (b & c) */
constexpr int TT_XNOR_AB = 0xC3;      /* ~(a ^ b) */

/* ColumnSum with an optional carry-in of one: N planes + CIN.  Even N: the leftover half adder takes the one as its third
 * input (x ^ y ^ 1, maj(x, y, 1)): the same two ops.  Odd N: s + 1 = (~s, carry s): one op more. */
template <int N, bool CIN>
struct ColumnSumBiased {
    static constexpr int NC = (N + (CIN ? 1 : 0)) / 2;
    static GKM_HD uint32_t run(const uint32_t *x, uint32_t *carry)
    {
        uint32_t s = x[0];
        int nc = 0;
#pragma unroll
        for (int i = 1; i + 1 < N; i += 2) {
            carry[nc++] = lop3<TT_MAJ>(s, x[i], x[i + 1]);
            s = lop3<TT_XOR3>(s, x[i], x[i + 1]);
        }
        if constexpr (N % 2 == 0) {
            carry[nc++] = CIN ? (s | x[N - 1]) : (s & x[N - 1]);
            s = CIN ? lop3<TT_XNOR_AB>(s, x[N - 1], x[N - 1]) : (s ^ x[N - 1]);
        } else if constexpr (CIN) {
            carry[nc++] = s;
            s = ~s;
        }
        return s;
    }
};

template <int I, int NB, int MX, int N, bool CIN>
GKM_HD void plane_sum_columns_biased(const uint32_t *x, Cnt<NB, MX> &r)
{
    if constexpr (N >= 1 && I < Cnt<NB, MX>::P) {
        using CS = ColumnSumBiased<N, CIN>;
        uint32_t carry[CS::NC > 0 ? CS::NC : 1];
        r.b[I] = CS::run(x, carry);
        plane_sum_columns_biased<I + 1, NB, MX, CS::NC, false>(carry, r);
    }
}

template <int W, int L, int D, int GRP>
GKM_HD void window_group_any(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AV, const uint32_t *Bhi,
                             const uint32_t *Blo, uint32_t *any)
{
    static_assert(L >= 2 && L <= 12, "L out of range");
    static_assert(W % GRP == 0, "a shift is a whole number of groups");
    if constexpr (!top_plane_serves(L, D)) {
        uint32_t hit[W];
        window_hits<W, L, D>(Ahi, Alo, AV, Bhi, Blo, (const uint32_t *)nullptr, hit);
#pragma unroll
        for (int w0 = 0; w0 < W; w0 += GRP) {
            uint32_t a = hit[w0];
#pragma unroll
            for (int g = 1; g + 1 < GRP; g += 2) a = lop3<TT_OR3>(a, hit[w0 + g], hit[w0 + g + 1]);
            if (GRP % 2 == 0) a |= hit[w0 + GRP - 1];
            any[w0 / GRP] = a;
        }
    } else {
        constexpr int P = bitlen(L);
        constexpr int BETA = top_plane_bias(L, D);
        constexpr int NX = W + L - 1;
        uint32_t Z[NX]; /* MATCH bits */
#pragma unroll
        for (int w = 0; w < W; w++) Z[w] = lop3<TT_NOT_A_OR_BXC>(Ahi[w] ^ Bhi[w], Alo[w], Blo[w]);
#pragma unroll
        for (int x = W; x < NX; x++) Z[x] = Z[x - W] >> 1; /* word x == word x-W one bit up; bit row 31: a mismatch */

        Cnt<P, L + BETA> cnt; /* matches + BETA: 0 .. L + BETA < 2^P, exact in P planes */
        static_assert(Cnt<P, L + BETA>::P == P && !Cnt<P, L + BETA>::OV, "the biased count fills exactly its planes");
        cnt.ovf = 0u;
        plane_sum_columns_biased<0, P, L + BETA, L, BETA == 1>(Z, cnt);
#pragma unroll
        for (int w = 0; w < W; w++) {
            if (w > 0) { /* the up/down counter of window_hits, stepping a count of matches */
                const uint32_t zout = Z[w - 1], zin = Z[w + L - 1];
                const uint32_t old0 = cnt.b[0];
                cnt.b[0] = lop3<TT_XOR3>(old0, zin, zout);
                uint32_t t = lop3<TT_BXC_AND_AXC>(old0, zin, zout);
#pragma unroll
                for (int i = 1; i < P; i++) {
                    const uint32_t old = cnt.b[i];
                    cnt.b[i] = old ^ t;
                    if (i + 1 < P) t = lop3<TT_A_AND_BXC>(t, old, zout);
                }
            }
            /* threshold + row validity + the group's OR: one op */
            const uint32_t top = cnt.b[P - 1];
            if (w % GRP == 0) any[w / GRP] = top & AV[w];
            else any[w / GRP] = lop3<TT_A_OR_BC>(any[w / GRP], top, AV[w]);
        }
    }
}

/*
 * window_group_any's top-plane path with the row validity applied once per GROUP instead of once per word:
 *     AVg[g] = AV[g*GRP] | .. | AV[g*GRP + GRP-1]        (built once per wave by the caller)
 *     any[g] = (top[g*GRP] | .. | top[g*GRP + GRP-1]) & AVg[g]
 * For GRP = 5 that is two three-input ORs and one AND per group where window_group_any spends one op per word, and W / GRP
 * registers of validity instead of W.  Only for (L, D) whose threshold is the top plane (top_plane_serves).
 *
 * What it delivers is a SUPERSET of window_group_any's any[g]: bit row b of group g is flagged when SOME window of the five
 * has <= D mismatches and SOME window of the five is owned -- not necessarily the same one.  It is for a consumer that
 * evaluates every window of a flagged (bit row, group) itself and lets the windows nobody owns add nothing, which is what
 * the same-length variant of k_gram_bitslice does (its trip tests m <= d per window and reads the row weight by position
 * from a table with L - 1 zero bytes behind the row's last l-mer).  The extra flags are confined to groups that are owned
 * in part: with table-built planes whose pieces own multiples of GRP windows unless they finish their row, only the group
 * that holds the row's last l-mer nB - 1 is such a group, and the windows it adds are positions nB .. nB + GRP - 2 of the
 * row (tests/test_group_validity.py).  The several-pieces variants, whose row weights are indexed by distance and have
 * no zero guard, keep window_group_any.
 */
template <int W, int L, int D, int GRP>
GKM_HD void window_group_any_grouped(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                     const uint32_t *Blo, uint32_t *any)
{
    static_assert(L >= 2 && L <= 12, "L out of range");
    static_assert(W % GRP == 0, "a shift is a whole number of groups");
    static_assert(top_plane_serves(L, D), "the grouped form exists for the top-plane (L, D) pairs only");
    constexpr int P = bitlen(L);
    constexpr int BETA = top_plane_bias(L, D);
    constexpr int NX = W + L - 1;
    uint32_t Z[NX]; /* MATCH bits, as in window_group_any */
#pragma unroll
    for (int w = 0; w < W; w++) Z[w] = lop3<TT_NOT_A_OR_BXC>(Ahi[w] ^ Bhi[w], Alo[w], Blo[w]);
#pragma unroll
    for (int x = W; x < NX; x++) Z[x] = Z[x - W] >> 1;

    Cnt<P, L + BETA> cnt;
    static_assert(Cnt<P, L + BETA>::P == P && !Cnt<P, L + BETA>::OV, "the biased count fills exactly its planes");
    cnt.ovf = 0u;
    plane_sum_columns_biased<0, P, L + BETA, L, BETA == 1>(Z, cnt);
    uint32_t top[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        if (w > 0) {
            const uint32_t zout = Z[w - 1], zin = Z[w + L - 1];
            const uint32_t old0 = cnt.b[0];
            cnt.b[0] = lop3<TT_XOR3>(old0, zin, zout);
            uint32_t t = lop3<TT_BXC_AND_AXC>(old0, zin, zout);
#pragma unroll
            for (int i = 1; i < P; i++) {
                const uint32_t old = cnt.b[i];
                cnt.b[i] = old ^ t;
                if (i + 1 < P) t = lop3<TT_A_AND_BXC>(t, old, zout);
            }
        }
        top[w] = cnt.b[P - 1];
        if (w % GRP == GRP - 1) { /* the group is complete: OR of its top planes, three at a time, then its validity */
            const int w0 = w - (GRP - 1);
            uint32_t a = top[w0];
#pragma unroll
            for (int g = 1; g + 1 < GRP; g += 2) a = lop3<TT_OR3>(a, top[w0 + g], top[w0 + g + 1]);
            if (GRP % 2 == 0) a |= top[w0 + GRP - 1];
            any[w0 / GRP] = a & AVg[w0 / GRP];
        }
    }
}

/*
 * window_group_any_grouped without ever stepping the top count plane: the same any[], bit for bit, on every bit.
 *
 * The counter's step of the top plane is b_top[w+1] = b_top[w] ^ t[w+1], with t the carry/borrow into it, which the step of
 * the planes below computes anyway.  Over any run of consecutive words, then,
 *     OR_w b_top[w] == b_top[first] | OR of t over the steps inside the run:
 * if no t fires every b_top of the run is equal; if one fires, b_top differs on its two sides and one of the two is set.  A
 * Boolean identity on arbitrary words: it does not care what the counter counts or what bit row 31 of the extension words
 * holds.  So the top plane of the FIRST window is all that is ever kept of it.
 *
 * FROM THE MIDDLE (MIDDLE = true): the first window is word GRP's (the adder tree runs over Z[GRP .. GRP+L-1]); one chain of
 * steps goes up to word W-1, a second one, from a copy of the lower planes, down to word 0 (stepping down, the word that
 * enters is Z[w-1] and the one that leaves Z[w+L-1]: the same truth tables).  With P = bitlen(L) planes a step is
 * 2 (P - 1) ops, a chain's last step P - 1 (its plane updates are dead):
 *     any[1] = (b_top[GRP] | t_up[1] | .. | t_up[GRP-1]) & AVg[1]
 *     any[0] = ((b_top[GRP] ^ t_dn[0]) | t_dn[1] | .. | t_dn[GRP-1]) & AVg[0]      (b_top[GRP-1] = b_top[GRP] ^ t_dn[0])
 * three 3-input ops each at GRP = 5.  W = 10, P = 4: 7 steps of 6 + 2 of 3 + 6 = 54 where the stepped top plane took
 * 8 x 7 + 4 + 6 = 66.
 * ONE DIRECTION (MIDDLE = false): the first window is word 0's, one chain up to word W-1:
 *     any[0] = (b_top[0] | t[1] | .. | t[GRP-1]) & AVg[0]
 *     any[1] = ((b_top[0] ^ t[1] ^ .. ^ t[GRP]) | t[GRP+1] | .. | t[W-1]) & AVg[1]
 * W = 10, P = 4: 8 x 6 + 3 + 3 + 5 = 59.  It holds one copy of the lower planes; kept as the form to fall back to where the
 * other does not fit its registers, and as a second route to the same bits for the CPU test.
 */
constexpr int TT_AXB_OR_C = 0xBE;  /* (a ^ b) | c */
constexpr int TT_AB_AND_C = 0xA8;  /* (a | b) & c */

/* one step of the up/down counter's planes below the top one (lo[0 .. P-2]); returns the carry/borrow into the top plane.
 * `last`: the chain ends here, the planes are not needed again */
template <int P>
GKM_HD uint32_t count_step_crossing(uint32_t *lo, uint32_t zin, uint32_t zout, bool last)
{
    const uint32_t old0 = lo[0];
    if (!last) lo[0] = lop3<TT_XOR3>(old0, zin, zout);
    uint32_t t = lop3<TT_BXC_AND_AXC>(old0, zin, zout);
#pragma unroll
    for (int i = 1; i < P - 1; i++) {
        const uint32_t old = lo[i];
        if (!last) lo[i] = old ^ t;
        t = lop3<TT_A_AND_BXC>(t, old, zout);
    }
    return t;
}
/* (a | t[0] | .. | t[N-1]) & v, three inputs at a time */
template <int N>
GKM_HD uint32_t or_terms_and(uint32_t a, const uint32_t *t, uint32_t v)
{
#pragma unroll
    for (int i = 0; i + 1 < N; i += 2) a = lop3<TT_OR3>(a, t[i], t[i + 1]);
    if constexpr (N % 2 == 1) return lop3<TT_AB_AND_C>(a, t[N - 1], v);
    else return a & v;
}

template <int W, int L, int D, int GRP, bool MIDDLE = true>
GKM_HD void window_group_any_crossings(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                       const uint32_t *Blo, uint32_t *any)
{
    static_assert(L >= 2 && L <= 12, "L out of range");
    static_assert(W == 2 * GRP && GRP >= 3, "a shift is two groups");
    static_assert(top_plane_serves(L, D), "the crossings form exists for the top-plane (L, D) pairs only");
    constexpr int P = bitlen(L);
    static_assert(P >= 2, "a top plane and at least one below it");
    constexpr int BETA = top_plane_bias(L, D);
    constexpr int NX = W + L - 1;
    constexpr int C = MIDDLE ? GRP : 0; /* the word whose window the adder tree sums */
    uint32_t Z[NX]; /* MATCH bits, as in window_group_any */
#pragma unroll
    for (int w = 0; w < W; w++) Z[w] = lop3<TT_NOT_A_OR_BXC>(Ahi[w] ^ Bhi[w], Alo[w], Blo[w]);
#pragma unroll
    for (int x = W; x < NX; x++) Z[x] = Z[x - W] >> 1;

    Cnt<P, L + BETA> cnt;
    static_assert(Cnt<P, L + BETA>::P == P && !Cnt<P, L + BETA>::OV, "the biased count fills exactly its planes");
    cnt.ovf = 0u;
    plane_sum_columns_biased<0, P, L + BETA, L, BETA == 1>(Z + C, cnt);
    const uint32_t top = cnt.b[P - 1];
    uint32_t up[P - 1];
#pragma unroll
    for (int i = 0; i < P - 1; i++) up[i] = cnt.b[i];

    if constexpr (MIDDLE) {
        uint32_t dn[P - 1];
#pragma unroll
        for (int i = 0; i < P - 1; i++) dn[i] = cnt.b[i];
        uint32_t tu[GRP - 1], td[GRP];
#pragma unroll
        for (int s = 0; s < GRP - 1; s++) { /* to word C + 1 + s */
            const int w = C + 1 + s;
            tu[s] = count_step_crossing<P>(up, Z[w + L - 1], Z[w - 1], s == GRP - 2);
        }
#pragma unroll
        for (int s = 0; s < GRP; s++) { /* down to word C - 1 - s: Z[w] enters, Z[w + L] leaves */
            const int w = C - 1 - s;
            td[s] = count_step_crossing<P>(dn, Z[w], Z[w + L], s == GRP - 1);
        }
        any[1] = or_terms_and<GRP - 1>(top, tu, AVg[1]);
        any[0] = or_terms_and<GRP - 2>(lop3<TT_AXB_OR_C>(top, td[0], td[1]), td + 2, AVg[0]);
    } else {
        uint32_t t[W - 1]; /* t[w - 1]: into the top plane on the step to word w */
#pragma unroll
        for (int w = 1; w < W; w++) t[w - 1] = count_step_crossing<P>(up, Z[w + L - 1], Z[w - 1], w == W - 1);
        any[0] = or_terms_and<GRP - 1>(top, t, AVg[0]);
        /* b_top[GRP] = b_top[0] ^ (the steps to words 1 .. GRP): GRP + 1 terms, three at a time */
        uint32_t e = top;
#pragma unroll
        for (int i = 0; i + 1 < GRP; i += 2) e = lop3<TT_XOR3>(e, t[i], t[i + 1]);
        if constexpr (GRP % 2 == 0) any[1] = or_terms_and<GRP - 1>(e, t + GRP, AVg[1]);
        else any[1] = or_terms_and<GRP - 2>(lop3<TT_AXB_OR_C>(e, t[GRP - 1], t[GRP]), t + GRP + 1, AVg[1]);
    }
}

/*
 * window_group_any_grouped without ANY counter: the same any[], bit for bit, on every bit.
 *
 * What a group delivers is the OR over its five windows of "biased count >= 2^(P-1)", i.e. whether the LARGEST of the five
 * counts reaches the top plane.  The five windows of group w0 .. w0+4 lie at most two steps from the centre window
 * C = w0 + 2, and a step changes a count by e = zin - zout in {-1, 0, +1}:
 *     up:    e1 = Z[C+L]  - Z[C],       e2 = Z[C+L+1] - Z[C+1]          B[C+1] = B[C] + e1,  B[C+2] = B[C] + e1 + e2
 *     down:  f1 = Z[C-1]  - Z[C+L-1],   f2 = Z[C-2]   - Z[C+L-2]        B[C-1] = B[C] + f1,  B[C-2] = B[C] + f1 + f2
 * so the group's largest count is B[C] + M with M = max(0, e1, e1 + e2, f1, f1 + f2) in {0, 1, 2}.  The centre window is
 * summed exactly by the adder tree (planes b[0 .. P-1], beta <= B[C] <= L + beta < 2^P: no wrap, as in window_group_any),
 * and B[C] + M >= 2^(P-1) holds iff B[C] >= 2^(P-1), or B[C] = 2^(P-1) - 1 and M >= 1, or B[C] = 2^(P-1) - 2 and M = 2:
 *     OR over the group of (B >= 2^(P-1))  ==  b[P-1] | (b[P-2] & .. & b[1] & ((b[0] & [M >= 1]) | [M = 2]))
 * ([M = 2] implies [M >= 1], so the last term needs no ~b[0]).  An identity on arbitrary words once more: every B it speaks
 * of is the sum of the same L words of Z that the stepped counter reaches, the extension words' fiction included.
 * Per side, with (zin1, zout1) the first step's words and (zin2, zout2) the second's, three ops:
 *     p        = zin2 & ~zout2                                         the second step counts up
 *     [M >= 1] = (zin1 & ~zout1) | (~(zin1 ^ zout1) & p)               up at once, or level and then up
 *     [M = 2]  = zin1 & ~zout1 & p
 * and four to combine: u = ([M>=1]up | [M>=1]dn) & b[0];  v = [M=2]up | [M=2]dn | u;  x = b[P-2] & .. & b[1] & v;
 * any = (b[P-1] | x) & AVg.  Ten ops per group beside its adder tree where the two chains of the crossings form and their ORs
 * take 54 per shift beside one tree: W = 10, L = 11: 2 x (16 + 10) = 52 against 16 + 54 = 70, with no chain of dependent steps and no second
 * copy of the lower planes.  GRP = 5 only: a window further than two steps from the centre would need M up to 3 and a
 * third plane in the comparison.
 */
constexpr int TT_A_ANDN_B = 0x30;      /* a & ~b (c unused) */
constexpr int TT_UP_OR_LEVEL_C = 0xB2; /* (a & ~b) | (~(a ^ b) & c) */
constexpr int TT_A_ANDN_B_C = 0x20;    /* a & ~b & c */
constexpr int TT_AND3 = 0x80;          /* a & b & c */

/*
 * SHARED TREES (SHARED = true, what the kernel runs): the two centre windows Z[C0 .. C0+L-1] and Z[C1 .. C1+L-1], C1 = C0 + GRP,
 * have the n = L - GRP words Z[C1 .. C0+L-1] in common, and a column sum does not care in which order its planes are folded.  So
 * the overlap's words are folded three at a time ONCE, by floor(n / 3) full adders; each centre's column 0 then takes its GRP
 * exclusive words, the shared sums and the overlap's leftover words, and its column 1 takes that column's carries and the shared
 * carries.  A bias of one is common to both centres as well: where the overlap leaves a word over it rides there (two leftover
 * words: their half adder with a third input of one, as in ColumnSumBiased; one: w + 1 = (~w, carry w)), else in each centre's
 * column 0 as before.  L = 11: FA(Z7, Z8, Z9), FA(Z10, Z11, Z12), then per centre 3 full adders in column 0 (5 + 2 planes) and 2
 * in column 1 (3 + 2 carries): 4 + 2 x 10 ops where two private trees take 2 x 14 below their top half adder.  L = 10, bias 1:
 * FA(Z7, Z8, Z9) and the biased half adder of Z10, Z11: the same 4 + 2 x 10.
 * THE TOP HALF ADDER FOLDED INTO THE THRESHOLD: where the column of plane P-2 holds exactly two planes p and q (L = 10, 11 and
 * others: top_pair_folds), b[P-2] = p ^ q and b[P-1] = p & q, and with y = b[P-3] & .. & b[1] & v the group's word is
 *     b[P-1] | (b[P-2] & y)  =  (p & q) | ((p ^ q) & y)  =  maj(p, q, y)
 * so neither plane is ever formed: y, maj, & AVg -- three ops where the half adder, x and the last op took four.  Other shapes
 * (L = 12, d = 4: three planes in that column, a full adder) keep their last stage.
 * Per shift at W = 10, L = 11: 20 + 10 + 4 + 2 x (10 + 6 + 2 + 3) + 6 = 82 where the private trees come to 88.  Both are the
 * same function of Z, bit for bit on arbitrary words (tests/test_shared_trees.py); SHARED = false is the private form, kept
 * for the A/B build (-DGKM_BS_CENTRES=1) and as the second route of that test.
 */
constexpr bool top_pair_folds(int I, int P, int N) /* column I holds N planes: does column P-2 come to hold exactly two? */
{
    return I > P - 2 ? false : I == P - 2 ? N == 2 : top_pair_folds(I + 1, P, N / 2);
}
/* planes I .. of a count from the N planes of column I, column compression as in ColumnSum; with FOLD the pair of column P-2 is
 * handed back in pq instead of being added */
template <int I, int P, int N, bool FOLD>
GKM_HD void centre_planes(const uint32_t *x, uint32_t *b, uint32_t *pq)
{
    if constexpr (FOLD && I == P - 2) {
        static_assert(N == 2, "the fold is for a column of exactly two planes");
        pq[0] = x[0];
        pq[1] = x[1];
    } else if constexpr (I < P) {
        static_assert(N >= 1, "a plane of the count has at least one input");
        uint32_t carry[ColumnSum<N>::NC > 0 ? ColumnSum<N>::NC : 1];
        b[I] = ColumnSum<N>::run(x, carry);
        centre_planes<I + 1, P, ColumnSum<N>::NC, FOLD>(carry, b, pq);
    }
}

/*
 * SHIFT-SHARED TREES (SHIFTED = true, what the kernel runs where shift_shared_serves): the shared form shares the words the two
 * centre windows have in common AS WORDS.  It does not use that an extension word is a shifted copy of a match word, Z[x] =
 * Z[x - W] >> 1: for L >= W the second centre's GRP top words Z[HALF+L .. HALF+L+GRP-1] are the words Z[HALF+L-W ..] of the first
 * centre one bit row on, and a column sum is bitwise, so the planes of their sum are the planes of the first centre's sum shifted.
 * With NH = L - W head words per centre, S the five words behind the first centre's heads and U the five words that end it:
 *     c0 = Z[HALF .. HALF+NH-1]         + S        + U (+ beta)      S = Z[HALF+NH .. HALF+NH+GRP-1]  (match words, all below W)
 *     c1 = Z[HALF+GRP .. HALF+GRP+NH-1] + (S >> 1) + U (+ beta)      U = Z[HALF+L-GRP .. HALF+L-1]
 * L = 11: c0 = z2 + (z3 + .. + z7) + (z8 + z9 + z'0 + z'1 + z'2), c1 = z7 + (z'3 + .. + z'7) + the same; L = 10: no heads.
 * S and U are summed once, two full adders each (planes s; k1, k2 and u; m1, m2), the three planes of S are shifted, and per centre
 * column 0 is one full adder over {head, s or s >> 1, u} (L = 10: the half adder of s, u with the bias of one as its third input)
 * and column 1 two full adders over {k1, k2 (shifted for c1), m1, m2, that carry}: 4 + 3 + 4 + 2 x 6 = 23 ops where the shared form
 * takes 4 + 2 x 10, and the extension word Z[HALF+L+HALF] (Z15 at L = 11, Z14 at L = 10) has no reader left: per shift at W = 10,
 * L = 11, 20 + 9 + 23 + 2 x (6 + 2 + 3) + 6 = 80.  Column 1 ends in two planes as before, so the fold of the top pair is unchanged.
 * Bit row 31: s >> 1 reads five mismatches there, which is what the five shifted words Z[x - W] >> 1 read -- the same fiction, so
 * the identity holds on every bit of arbitrary words (tests/test_shift_shared_trees.py).  Taken for L - W <= 1, the shapes whose
 * listing was seen to get shorter; every other pair stays on the shared form.
 */
constexpr bool shift_shared_serves(int W, int L, int D, int GRP)
{
    return top_plane_serves(L, D) && W == 2 * GRP && L >= W && L - W <= 1;
}

template <int W, int L, int D, int GRP, bool SHARED = true, bool SHIFTED = false>
GKM_HD void window_group_any_centres(const uint32_t *Ahi, const uint32_t *Alo, const uint32_t *AVg, const uint32_t *Bhi,
                                     const uint32_t *Blo, uint32_t *any)
{
    static_assert(L >= 2 && L <= 12, "L out of range");
    static_assert(W == 2 * GRP && GRP == 5, "a shift is two groups of five: every window within two steps of its group's centre");
    static_assert(top_plane_serves(L, D), "the centres form exists for the top-plane (L, D) pairs only");
    constexpr int P = bitlen(L);
    static_assert(P >= 3, "a top plane, plane 0 and at least one between them");
    constexpr int BETA = top_plane_bias(L, D);
    constexpr int NX = W + L - 1;
    constexpr int HALF = GRP / 2;
    uint32_t Z[NX]; /* MATCH bits, as in window_group_any */
#pragma unroll
    for (int w = 0; w < W; w++) Z[w] = lop3<TT_NOT_A_OR_BXC>(Ahi[w] ^ Bhi[w], Alo[w], Blo[w]);
#pragma unroll
    for (int x = W; x < NX; x++) Z[x] = Z[x - W] >> 1;

    /* the overlap of the two centre windows, folded once (SHARED): NS planes for each centre's column 0, NY for its column 1 */
    constexpr bool SS = SHIFTED && shift_shared_serves(W, L, D, GRP); /* the shift-shared form; else the form SHARED names */
    constexpr bool SH = SHARED && L >= GRP && !SS;
    constexpr int OV0 = GRP + HALF;                      /* the overlap's first word: the second centre */
    constexpr int NOV = SH ? L - GRP : 0;                /* its words Z[OV0 .. HALF+L-1] */
    constexpr int NF = NOV / 3, REST = NOV - 3 * NF;     /* full adders, words left over */
    constexpr bool BIAS_SH = SH && BETA == 1 && REST > 0; /* the one rides in the overlap's leftover */
    constexpr int NS = NF + (BIAS_SH ? 1 : REST), NY = NF + (BIAS_SH ? 1 : 0);
    constexpr int N0 = GRP + NS;                         /* planes of a centre's column 0: its own words and the shared sums */
    constexpr bool CIN0 = BETA == 1 && !BIAS_SH;         /* ... and the one, where the overlap could not take it */
    using CS0 = ColumnSumBiased<N0, CIN0>;
    constexpr int N1 = CS0::NC + NY;                     /* planes of its column 1 */
    /* the shift-shared form: NH head words per centre, S behind the first centre's heads, U the first centre's last GRP words */
    constexpr int NH = SS ? L - W : 0;
    constexpr int XS = HALF + NH, XU = HALF + L - GRP;
    using CSS = ColumnSumBiased<NH + 2, BETA == 1>;      /* a centre's column 0: its heads, s or s >> 1, u and the one */
    constexpr int NK = ColumnSum<GRP>::NC;               /* carries of S, and of U */
    constexpr int N1S = 2 * NK + CSS::NC;                /* planes of its column 1 */
    constexpr bool FOLD = SS ? top_pair_folds(1, P, N1S) : SH && top_pair_folds(1, P, N1);
    uint32_t s0[2] = {0u, 0u}, sk[2][NK], su = 0u, sm[NK];
    if constexpr (SS) {
        static_assert(XS + GRP <= W && XU + GRP <= NX, "S is made of match words, U lies inside both centre windows");
        s0[0] = ColumnSum<GRP>::run(Z + XS, sk[0]);
        s0[1] = s0[0] >> 1; /* the sum of the words one bit row on: its planes one bit row on */
#pragma unroll
        for (int i = 0; i < NK; i++) sk[1][i] = sk[0][i] >> 1;
        su = ColumnSum<GRP>::run(Z + XU, sm);
    }
    uint32_t ss[NS > 0 ? NS : 1], sy[NY > 0 ? NY : 1];
    if constexpr (SH) {
#pragma unroll
        for (int i = 0; i < NF; i++) {
            const uint32_t a = Z[OV0 + 3 * i], b = Z[OV0 + 3 * i + 1], c = Z[OV0 + 3 * i + 2];
            ss[i] = lop3<TT_XOR3>(a, b, c);
            sy[i] = lop3<TT_MAJ>(a, b, c);
        }
        if constexpr (BIAS_SH && REST == 2) { /* a + b + 1 */
            const uint32_t a = Z[OV0 + 3 * NF], b = Z[OV0 + 3 * NF + 1];
            ss[NF] = lop3<TT_XNOR_AB>(a, b, b);
            sy[NF] = a | b;
        } else if constexpr (BIAS_SH) { /* a + 1 */
            ss[NF] = ~Z[OV0 + 3 * NF];
            sy[NF] = Z[OV0 + 3 * NF];
        } else {
#pragma unroll
            for (int i = 0; i < REST; i++) ss[NF + i] = Z[OV0 + 3 * NF + i];
        }
    }

#pragma unroll
    for (int g = 0; g < W / GRP; g++) {
        const int C = g * GRP + HALF; /* the group's centre word: C - 2 >= 0, C + L + 1 <= NX - 1 */
        uint32_t b[P], pq[2] = {0u, 0u};
        if constexpr (SS) {
            /* column 0: the centre's heads, the sum of S (group 1: one bit row on) and of U; column 1: their carries and its own */
            const int H0 = g == 0 ? HALF : HALF + GRP;
            uint32_t c0[NH + 2], cc[CSS::NC], c1[N1S];
#pragma unroll
            for (int i = 0; i < NH; i++) c0[i] = Z[H0 + i];
            c0[NH] = s0[g];
            c0[NH + 1] = su;
            b[0] = CSS::run(c0, cc);
#pragma unroll
            for (int i = 0; i < NK; i++) {
                c1[i] = sk[g][i];
                c1[NK + i] = sm[i];
            }
#pragma unroll
            for (int i = 0; i < CSS::NC; i++) c1[2 * NK + i] = cc[i];
            centre_planes<1, P, N1S, FOLD>(c1, b, pq);
        } else if constexpr (SH) {
            /* column 0: the centre's own GRP words (group 0: below the overlap, group 1: above it) and the shared sums */
            const int X0 = g == 0 ? HALF : HALF + L;
            uint32_t c0[N0], c1[N1];
#pragma unroll
            for (int i = 0; i < GRP; i++) c0[i] = Z[X0 + i];
#pragma unroll
            for (int i = 0; i < NS; i++) c0[GRP + i] = ss[i];
            b[0] = CS0::run(c0, c1);
#pragma unroll
            for (int i = 0; i < NY; i++) c1[CS0::NC + i] = sy[i];
            centre_planes<1, P, N1, FOLD>(c1, b, pq);
        } else {
            Cnt<P, L + BETA> cnt;
            static_assert(Cnt<P, L + BETA>::P == P && !Cnt<P, L + BETA>::OV, "the biased count fills exactly its planes");
            cnt.ovf = 0u;
            plane_sum_columns_biased<0, P, L + BETA, L, BETA == 1>(Z + C, cnt);
#pragma unroll
            for (int i = 0; i < P; i++) b[i] = cnt.b[i];
        }
        /* up: Z[C+L], Z[C+L+1] enter, Z[C], Z[C+1] leave; down: Z[C-1], Z[C-2] enter, Z[C+L-1], Z[C+L-2] leave */
        const uint32_t pu = lop3<TT_A_ANDN_B>(Z[C + L + 1], Z[C + 1], Z[C + 1]);
        const uint32_t m1u = lop3<TT_UP_OR_LEVEL_C>(Z[C + L], Z[C], pu);
        const uint32_t m2u = lop3<TT_A_ANDN_B_C>(Z[C + L], Z[C], pu);
        const uint32_t pd = lop3<TT_A_ANDN_B>(Z[C - 2], Z[C + L - 2], Z[C + L - 2]);
        const uint32_t m1d = lop3<TT_UP_OR_LEVEL_C>(Z[C - 1], Z[C + L - 1], pd);
        const uint32_t m2d = lop3<TT_A_ANDN_B_C>(Z[C - 1], Z[C + L - 1], pd);
        const uint32_t u = lop3<TT_AB_AND_C>(m1u, m1d, b[0]);
        uint32_t x = lop3<TT_OR3>(m2u, m2d, u);
        /* the planes between plane 0 and the top one (with the fold: below the pair's), two at a time */
        constexpr int TOPMID = FOLD ? P - 3 : P - 2;
#pragma unroll
        for (int i = 1; i + 1 <= TOPMID; i += 2) x = lop3<TT_AND3>(b[i], b[i + 1], x);
        if constexpr (TOPMID >= 1 && TOPMID % 2 == 1) x &= b[TOPMID];
        if constexpr (FOLD) any[g] = lop3<TT_MAJ>(pq[0], pq[1], x) & AVg[g];
        else any[g] = lop3<TT_AB_AND_C>(b[P - 1], x, AVg[g]);
    }
}

/* ------------------------------------------------------------------ tables */
/* Word w of a ROW SEGMENT plane.  Segment base i = b*W + w is sequence position s0 + i.
 * plane 0/1: hi/lo bit of the base code (0 beyond the end of the sequence);
 * plane 2: window-start validity: the l-mer starting at s0+i exists (s0+i <= len-L) and
 * belongs to this segment (i < segment_capacity). */
GKM_HD uint32_t row_plane_word(const uint8_t *codes, int len, int s0, int w, int W, int L, int plane)
{
    uint32_t v = 0u;
    const int cap = 32 * W - (L - 1);
    for (int b = 0; b < 32; b++) {
        const int i = b * W + w, pos = s0 + i;
        uint32_t bit;
        if (plane == 2) bit = (pos <= len - L && i < cap) ? 1u : 0u;
        else bit = (pos < len) ? ((uint32_t)(codes[pos] >> (1 - plane)) & 1u) : 0u;
        v |= bit << b;
    }
    return v;
}

/* Packed lanes (gkm_pack.h): the bit that one PIECE -- bit rows [b0, b0+nb) of a lane holding
 * sequence positions p0.. with cnt owned window starts -- contributes to bit row b, word w of
 * plane 0/1 (hi/lo bit of the base code, 0 beyond the sequence) or plane 2 (window start owned
 * by the piece).  Bit rows outside the piece contribute 0. */
GKM_HD uint32_t piece_bit(const uint8_t *codes, int len, int b0, int nb, int p0, int cnt, int b, int w, int W,
                          int plane)
{
    if (b < b0 || b >= b0 + nb) return 0u;
    const int li = (b - b0) * W + w;
    if (plane == 2) return li < cnt ? 1u : 0u;
    const int pos = p0 + li;
    return pos < len ? ((uint32_t)(codes[pos] >> (1 - plane)) & 1u) : 0u;
}
/* piece k of a lane owns bit row b: k = (number of piece starts at or below b) - 1, from the
 * lane's mask of piece-start bit rows */
GKM_HD int piece_of_bitrow(uint32_t start_mask, int b)
{
    return __builtin_popcount(start_mask & (0xFFFFFFFFu >> (31 - b))) - 1;
}

/* Word x of a COLUMN STRAND table ("SB"): bit b describes strand base (b*W + x) mod T,
 * i.e. what segment base i = b*W + w meets under the cyclic shift delta = x - w.
 * strand 0 = the sequence, strand 1 = its reverse complement (libgkm.c:877-888).
 * plane 2: that base starts an l-mer that does not wrap (q <= T-L). */
GKM_HD uint32_t sb_word(const uint8_t *codes, int T, int strand, int x, int W, int L, int plane)
{
    uint32_t v = 0u;
    int q = x % T;
    const int step = W % T;
    for (int b = 0; b < 32; b++) {
        uint32_t bit;
        if (plane == 2) bit = (q <= T - L) ? 1u : 0u;
        else {
            const uint32_t code = strand ? (3u - codes[T - 1 - q]) : codes[q];
            bit = (code >> (1 - plane)) & 1u;
        }
        v |= bit << b;
        q += step;
        if (q >= T) q -= T;
    }
    return v;
}

/* ------------------------------------------------------------------- hits */
/* exact x mod T for x < 2^32 / T, with rcp = ceil(2^32 / T) (T >= 2) */
GKM_HD uint32_t mod_magic(uint32_t T) { return 0xFFFFFFFFu / T + 1u; }
GKM_HD uint32_t mod_small(uint32_t x, uint32_t T, uint32_t rcp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return x - __umulhi(x, rcp) * T;
#else
    return x - (uint32_t)(((uint64_t)x * rcp) >> 32) * T;
#endif
}

/* Positional weights as a function of the distance to the sequence's centre l-mer:
 * w(n, p) = wd[|n/2 - p|] (libgkm.c:912-925 depends on n and p only through that
 * distance), so ONE small table serves every sequence length. */
GKM_HD uint32_t dist_weight(const uint8_t *wd, int center, int p)
{
    const int dd = center - p;
    return wd[dd < 0 ? -dd : dd];
}

/* l-mer table entry: the L bases as 2 bits each (first base in the highest pair, as a
 * number in base 4) in bits 0..23, the positional weight of that l-mer in bits 24..31 */
GKM_HD uint32_t lmer_entry(const uint8_t *codes, int len, int L, int strand, int p, uint32_t weight)
{
    uint32_t v = 0u;
    for (int i = 0; i < L; i++) {
        const uint32_t c = strand ? (3u - codes[len - 1 - (p + i)]) : codes[p + i];
        v = (v << 2) | c;
    }
    return v | (weight << 24);
}
GKM_HD int lmer_mismatch(uint32_t x, uint32_t y)
{
    uint32_t t = (x ^ y) & 0x00FFFFFFu;
    t = (t | (t >> 1)) & 0x00555555u;
    return __builtin_popcount(t);
}

/* Resolve one hit: bit b of the hit word of (delta, w, strand) against a row segment.
 *   row window start  p = s0 + b*W + w,  column l-mer q = (b*W + w + delta) mod T on `strand`
 * Returns m = Hamming distance of the two l-mers (<= d for a true hit) and v = wa*wb, the
 * amount the reference adds to mmprofile[m] (libgkm.c:338); the weights ride in the top
 * byte of the l-mer table entries (forward: wt[q], reverse strand: wt_rc[q] = wt[n-1-q],
 * libgkm.c:924).
 *   rowlm(i0)        table entry of the row's l-mer at segment offset i0
 *   collm(strand, q) table entry of the column strand's l-mer q */
struct HitValue {
    int m;
    uint32_t v;
};
template <int W, class RowLm, class ColLm>
GKM_HD HitValue resolve_hit(int b, int w, int delta, int strand, uint32_t T, uint32_t rcpT, int nB, RowLm rowlm,
                            ColLm collm)
{
    HitValue r;
    const int i0 = b * W + w;
    const uint32_t x = (uint32_t)(i0 + delta);
    int q;
    if (T >= (uint32_t)(32 * W)) { /* x < 2T: one conditional subtraction (uniform test) */
        const uint32_t y = x - T;
        q = (int)(y < x ? y : x);
    } else {
        q = (int)mod_small(x, T, rcpT);
    }
    if (q >= nB) { /* window wraps around the end of the strand: not an l-mer (see window_hits) */
        r.m = 0;
        r.v = 0u;
        return r;
    }
    const uint32_t ea = rowlm(i0), eb = collm(strand, q);
    r.m = lmer_mismatch(ea, eb);
    r.v = (ea >> 24) * (eb >> 24);
    return r;
}

/* ---- 2-bit packed strands: what the hit path reads -------------------------------------------
 * 16 bases per 32-bit word, base i of a strand in bits 2(i%16)..2(i%16)+1 of word i/16, zeros beyond
 * the end.  The l-mer starting at base pos is the low 2L bits of the 64-bit value (word[pos/16 + 1] :
 * word[pos/16]) >> 2(pos%16) -- one funnel shift (v_alignbit_b32) on two neighbouring words.  A hit
 * gathers two words of the row lane's packed positions (64 lanes x 21 words per tile: a few cache
 * lines, L1 resident) and two words of the column strand from LDS, instead of one 4-byte table entry
 * per l-mer and side: the per-l-mer tables made every gather touch 64 different cache lines, and the
 * vector memory pipeline, not the VALU, set the pace of the hit path (config 2: 18 of 91 ms). */
GKM_HD uint32_t pk_word(const uint8_t *codes, int len, int strand, int x)
{
    uint32_t v = 0u;
    for (int k = 0; k < 16; k++) {
        const int i = x * 16 + k;
        if (i >= len) break;
        const uint32_t c = strand ? (3u - codes[len - 1 - i]) : codes[i];
        v |= c << (2 * k);
    }
    return v;
}
/* the same with the strand continued cyclically behind its end (base i = base i mod len) */
GKM_HD uint32_t pk_word_cyclic(const uint8_t *codes, int len, int strand, int x)
{
    uint32_t v = 0u;
    int i = (x * 16) % len;
    for (int k = 0; k < 16; k++) {
        const uint32_t c = strand ? (3u - codes[len - 1 - i]) : codes[i];
        v |= c << (2 * k);
        if (++i == len) i = 0;
    }
    return v;
}
GKM_HD uint32_t pk_window(uint32_t lo, uint32_t hi, int pos)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(2 * (pos & 15)));
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (2 * (pos & 15)));
#endif
}
/* Hamming distance of the first L bases of two packed windows */
GKM_HD int pk_mismatch(uint32_t a, uint32_t b, int L)
{
    uint32_t t = (a ^ b) & ((1u << (2 * L)) - 1u);
    t = (t | (t >> 1)) & 0x55555555u;
    return __builtin_popcount(t);
}

/* Resolve one hit from packed data: bit b of the hit word of (delta, w, strand) against a row lane.
 *   lane position i0 = b*W + w; column l-mer q = (i0 + delta) mod T on `strand` (rejected if it wraps)
 *   roww(i0)        32-bit packed window of the row LANE's positions starting at i0
 *   colw(strand, q) 32-bit packed window of the column strand starting at base q
 *   wdist(D)        positional weight at distance D from the centre l-mer (libgkm.c:912-925); 1 if unweighted
 *   c0              (l-mers of the row)/2 - p0 + b0*W of the piece that owns the bit row, so that the
 *                   row l-mer's distance to its sequence's centre l-mer is |c0 - i0|
 * The reverse strand's weights are the forward ones mirrored: wt_rc[q] = wt[nB-1-q] (libgkm.c:924). */
template <int W, class RowWin, class ColWin, class Wdist>
GKM_HD HitValue resolve_hit_packed(int b, int w, int delta, int strand, uint32_t T, uint32_t rcpT, int nB, int L, int c0,
                                   RowWin roww, ColWin colw, Wdist wdist)
{
    HitValue r;
    r.m = 0;
    r.v = 0u;
    const int i0 = b * W + w;
    const uint32_t x = (uint32_t)(i0 + delta);
    int q;
    if (T >= (uint32_t)(32 * W)) { /* x < 2T: one conditional subtraction (uniform test) */
        const uint32_t y = x - T;
        q = (int)(y < x ? y : x);
    } else {
        q = (int)mod_small(x, T, rcpT);
    }
    if (q >= nB) return r; /* window wraps around the end of the strand: not an l-mer (see window_hits) */
    r.m = pk_mismatch(roww(i0), colw(strand, q), L);
    const int da = c0 - i0, qd = strand ? nB - 1 - q : q, db = nB / 2 - qd;
    r.v = wdist(da < 0 ? -da : da) * wdist(db < 0 ? -db : db);
    return r;
}

/* Origin word of a hit record.  The layout is chosen for the instruction count of the trip that consumes it, priced
 * with the issue rates measured on gfx950 (tools/valu_ops.hip, profiles/r3_valu_ops.txt: v_and / v_or / v_add / v_sub /
 * v_xor / v_not / v_mov / v_lshrrev / v_ashrrev / v_bitop3 issue every ~2.2 cycles per SIMD; everything else -- v_lshlrev
 * (also by a constant: 4.16, which is why the kernel doubles with v_add_u32 x, x), v_bfe, v_mad_u32_u24, v_min, v_sad,
 * v_alignbit, v_ffbl, v_bcnt, compares, SDWA -- every ~4.2; an SGPR operand costs a stream made of nothing else 4.2 too,
 * but nothing in a mix with VGPR-only instructions: 2.2 is what tools/issue_model.py prices it at):
 *   bits  0..3   word index w within the shift (0..W-1; a trip adds the word's offset in its group)       ms & 15
 *   bit   4      strand (0 forward, 1 reverse complement), bit 5: strand & [the column has an even number of l-mers]
 *                (the reverse strand's weights are the forward ones mirrored, wt_rc[q] = wt[nB-1-q] = wd[|q + even -
 *                nB/2|], libgkm.c:924) -- used by the CPU model of the hit path (bitslice_cpu_probe.cpp) only: since
 *                round 5 the kernel empties its hit list between the two strands, the strand is wave-uniform inside a
 *                trip and the kernel leaves both bits 0
 *   bits  7..12  source lane; ms & 0x1F80 is the byte offset of that lane's packed positions (128 bytes per lane)
 *   bits 21..31  shift delta (0..2046): ms >> 21
 *   (k_gram_bitslice's same-length variant also keeps, set once per wave by the source lane:
 *   bits  4..6   piece index of the lane within its row (the lane holds sequence positions pi * capacity ..)
 *   bits 13..18  row slot of the lane; (ms >> 11) & 0xFC is its byte offset in a profile row -- bits 13..19 and 0x1FC where
 *                tiles carry riders and a tile's profiles have 128 slots) */
constexpr uint32_t META_LANE_SHIFT = 7;
constexpr uint32_t META_PIECE_SHIFT = 4;
constexpr uint32_t META_SLOT_SHIFT = 13;
GKM_HD uint32_t pack_meta(int delta, int w, int strand, int even_adj = 0)
{
    return (uint32_t)w | ((uint32_t)strand << 4) | ((uint32_t)(strand & even_adj) << 5) | ((uint32_t)delta << 21);
}
/* The same-length variant with RIDERS (gkm_pack.h RIDER_B0): a lane's second tag word describes the rider piece in its top
 * two bit rows -- row slot * 4 in bits 2..8 (the byte offset in a profile row, second copy included), and from bit 9 up,
 * signed, what lane position i0 has to be moved by to become the l-mer's position in the rider (piece k of a layout with
 * W words: k * rider_w - RIDER_B0 * W), so that a trip's row weight is still at "base + i0". */
constexpr uint32_t RIDER_TAG_POS_SHIFT = 9;
GKM_HD uint32_t pack_rider_tag(int slot, int pos_base) { return ((uint32_t)pos_base << RIDER_TAG_POS_SHIFT) | ((uint32_t)slot << 2); }
GKM_HD int rider_tag_slot(uint32_t t) { return (int)((t >> 2) & 127u); }
GKM_HD int rider_tag_pos(uint32_t t) { return (int)((int32_t)t >> RIDER_TAG_POS_SHIFT); }
GKM_HD int rec_w(uint32_t r) { return (int)(r & 15u); }
GKM_HD int rec_delta(uint32_t r) { return (int)(r >> 21); }
GKM_HD int rec_strand(uint32_t r) { return (int)((r >> 4) & 1u); }
GKM_HD int rec_lane(uint32_t r) { return (int)((r >> META_LANE_SHIFT) & 63u); }

/* ---- SHIFT RECORDS (k_gram_bitslice PK = 6, 7): one record per lane and SHIFT instead of one per lane and group of five
 * words.  A record is three words: any0 and any1, the group ORs of the shift's two groups of five words (W = 10: which bit
 * rows of the lane hold a hit somewhere in words 0..4 / 5..9), and the origin word, which then carries no word index (its
 * bits 0..3 stay 0).  One compaction per shift in the counting loop; the trip that consumes the record finds the group:
 *   push    a lane with any0 | any1 != 0 appends (any0, any1, origin);
 *   visit   group g = any0 ? 0 : 1, the lowest bit row b of that group's word, cleared there; the visit resolves the five
 *           windows at lane positions W b + 5 g .. + 4 exactly as a group record's visit does;
 *   re-push if any0 | any1 is still non-zero the three words go back to the list.
 * Every (bit row, group) flagged by the shift is visited exactly once, group 0's bit rows in ascending order first, then
 * group 1's: popcount(any0) + popcount(any1) visits per record.  The same function runs per lane in the kernel's trip and in
 * the CPU model (bitslice_cpu_probe.cpp; tests/test_shift_records.py). */
constexpr int SHIFT_GROUP_WORDS = 5;
GKM_HD bool shift_record_live(uint32_t any0, uint32_t any1) { return (any0 | any1) != 0u; }
/* position of the lowest set bit, 0xFFFFFFFF for 0 (v_ffbl_b32's own convention; __builtin_ctz(0) is undefined and the
 * generic cttz costs a second instruction) */
GKM_HD uint32_t lowest_bit_or_ones(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x ? (uint32_t)__builtin_ctz(x) : 0xFFFFFFFFu;
#endif
}
struct ShiftVisit {
    uint32_t bit; /* the bit row visited (0xFFFFFFFF for an empty record: a lane without one in a partial trip) */
    uint32_t w0;  /* first word of the group visited: 0 or SHIFT_GROUP_WORDS */
};
/* one visit: takes the bit row out of (any0, any1) in place; the caller pushes the record again while shift_record_live */
GKM_HD ShiftVisit shift_record_visit(uint32_t &any0, uint32_t &any1)
{
    const bool second = any0 == 0u;
    ShiftVisit v;
    v.bit = lowest_bit_or_ones(second ? any1 : any0);
    v.w0 = second ? (uint32_t)SHIFT_GROUP_WORDS : 0u;
    const uint32_t rest1 = any1 & (any1 - 1u);
    any0 &= any0 - 1u; /* (0 stays 0) */
    any1 = second ? rest1 : any1;
    return v;
}

} /* namespace gkmbs */
#endif
