/*
 * gkm_pack.h -- host-side packing of row sequences into the lanes of the bit-sliced kernel.
 *
 * A lane of the kernel holds 32 "bit rows" of W consecutive sequence positions each (bit b of
 * word w <-> lane position b*W + w, gkm_bitslice.h).  A PIECE is a run of bit rows of one lane
 * given to one row sequence: bit rows [b0, b0+nb) hold sequence positions p0 .. p0+nb*W-1 and
 * own the `cnt` l-mer windows that start at p0 .. p0+cnt-1 (a window must lie inside its
 * piece, so cnt <= nb*W - (L-1); the next piece of the same sequence starts at p0+cnt and
 * therefore overlaps by L-1 bases).  Packing several pieces per lane keeps the lanes full for
 * any length distribution (one 300-bp row needs 15 of the 32 bit rows at W = 20).
 *
 * All pieces of a row live in ONE tile (64 lanes) so that the kernel can accumulate a row's
 * mismatch profile in LDS by "row slot".  Plain C++ (no HIP) so the packing is unit-tested on
 * the CPU (bitslice_cpu_probe.cpp).
 */
#ifndef GKM_PACK_H
#define GKM_PACK_H

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gkmpack {

constexpr int LANES = 64;
constexpr int MAX_PIECES = 4;   /* pieces per lane */
constexpr int MAX_ROWS = 128;   /* row slots per tile (a caller may ask pack_rows for fewer) */
/* RIDERS (same-length problems, pack_rows rider_w > 0).  A 300-bp row fills bit rows 0..29 of its lane; bit rows 30 and 31
 * would carry zeros through every instruction of every shift.  A rider is a further row of the tile that lives in those
 * two bit rows of MANY lanes: it is cut into pieces of rider_w owned windows, piece k = bases k * rider_w .. + 2 W - 1 of
 * the rider in bit rows RIDER_B0, RIDER_B0 + 1 of one lane (the second bit row is the L - 1 bases of overlap), 29 lanes
 * for 290 windows at rider_w = 10.  Two riders in 58 of the 64 lanes: 66 rows per tile instead of 64. */
constexpr int RIDER_B0 = 30, RIDER_NB = 2;
constexpr int RIDER_W = 10;     /* windows a rider piece owns: a multiple of the groups of five the kernel resolves */
constexpr int MAX_RIDERS = 16;  /* riders per tile: row slots stay below RIDER_SLOTS */
constexpr int RIDER_SLOTS = 64 + MAX_RIDERS; /* row slots per tile of the tile-transposed output when tiles carry riders */

struct Piece {
    int32_t lane;  /* global lane index = tile * 64 + lane in tile */
    int32_t b0;    /* first bit row */
    int32_t nb;    /* number of bit rows */
    int32_t slot;  /* row slot inside the tile */
    int32_t row;   /* sequence index */
    int32_t p0;    /* first sequence position (= first window start) of the piece */
    int32_t cnt;   /* window starts owned by the piece */
    int32_t rider; /* 1: a rider piece (bit rows RIDER_B0, RIDER_B0 + 1 of a lane whose own piece ends below them) */
};

struct Packing {
    int W = 0, L = 0, ntiles = 0;
    std::vector<Piece> pieces;          /* sorted by lane, then b0 */
    std::vector<int32_t> tile_row;      /* [ntiles * MAX_ROWS] sequence index of each row slot (-1 = unused) */
    std::vector<int32_t> tile_out;      /* [ntiles * MAX_ROWS] output row (position in the caller's row list) */
    std::vector<int32_t> tile_nrows;    /* [ntiles] residents and riders */
    std::vector<int32_t> tile_nres;     /* [ntiles] residents: the riders take the row slots from here on */
    int nriders = 0;
    std::vector<int32_t> tile_amax;     /* [ntiles] largest sequence index in the tile */
    long lanes_used = 0;
};

/* rows: ascending sequence indices; nwin[i]: l-mer windows of rows[i] (>= 1).
 * Greedy first-fit in row order (the order matters: a tile only visits columns j <= its largest
 * row, so tiles should hold neighbouring rows).
 * split_jump: a JUMP of at least that many rows in the list (the folded row blocks of a multi-GPU rank: rows 0..624, then
 * 9375..9999) closes the current tile.  Every work item of a tile is 64 lanes x one column for ALL columns up to the
 * tile's largest row, so low rows that share a tile with high ones ride along through thousands of columns they do not
 * need: rank 0 of an 8-way split of config 2 ran 109 660 work items instead of 100 760 (round 5,
 * profiles/r5_small_launch_blocks.txt).  Whether splitting pays depends on the list (it can also cost a tile); the caller
 * packs both ways and keeps the one with fewer work items (triangle_items).
 * own_mult: a piece that does not finish its row owns a multiple of that many windows (the same-length kernel variant
 * evaluates GROUPS of five consecutive lane positions at once and needs every group owned whole or not at all).
 * rider_w > 0: once a tile takes no further resident (max_rows of them, or no lane left), the next rows of the list ride
 * in bit rows RIDER_B0.. of its lanes, rider_w windows per piece, for as long as whole rows fit (see RIDER_B0): only
 * lanes that hold exactly one piece which ends at or below RIDER_B0 carry a rider piece, a tile takes no resident after
 * a rider (row slots and the tile's column range stay in row order), and max_rows bounds the residents.  rider_w = 0
 * packs exactly as before there were riders. */
inline Packing pack_rows(const int *rows, const int *nwin, int nrows, int W, int L, int max_rows = MAX_ROWS, int split_jump = 0,
                         int own_mult = 1, int rider_w = 0)
{
    Packing P;
    P.W = W;
    P.L = L;
    /* a rider piece owns rider_w windows inside its RIDER_NB bit rows, whole groups of own_mult */
    if (rider_w > RIDER_NB * W - (L - 1) || rider_w > W || rider_w % own_mult != 0) rider_w = 0;
    const int min_bits = (L + W - 1) / W;       /* bit rows needed for a single window */
    int tile = 0, lane = 0, freeb = 32, npl = 0; /* cursor: lane in tile, free bit rows, pieces in lane */
    int tile_rows = 0, tile_res = 0;             /* rows / residents of the open tile */
    int lane_used[LANES] = {0}, lane_np[LANES] = {0}, rider_lane = 0; /* bit rows and pieces per lane of the open tile */
    auto new_lane = [&]() { lane++; freeb = 32; npl = 0; };
    auto close_tile = [&]() {
        P.tile_nrows.push_back(tile_rows);
        P.tile_nres.push_back(tile_res);
        tile++;
        lane = 0; freeb = 32; npl = 0; tile_rows = 0; tile_res = 0; rider_lane = 0;
        for (int l = 0; l < LANES; l++) lane_used[l] = lane_np[l] = 0;
    };
    /* row i as a rider of the open tile: one piece in each of the next lanes that have the two bit rows to spare */
    auto try_rider = [&](int i) {
        if (rider_w <= 0 || tile_res == 0 || tile_rows - tile_res >= MAX_RIDERS || tile_rows >= MAX_ROWS) return false;
        const int np = (nwin[i] + rider_w - 1) / rider_w;
        int pick[LANES], found = 0, l = rider_lane;
        for (; l < LANES && found < np; l++)
            if (lane_np[l] == 1 && lane_used[l] <= RIDER_B0) pick[found++] = l;
        if (found < np) return false;
        for (int k = 0; k < np; k++) {
            Piece pc;
            pc.lane = tile * LANES + pick[k];
            pc.b0 = RIDER_B0;
            pc.nb = RIDER_NB;
            pc.slot = tile_rows;
            pc.row = rows[i];
            pc.p0 = k * rider_w;
            pc.cnt = nwin[i] - pc.p0 < rider_w ? nwin[i] - pc.p0 : rider_w;
            pc.rider = 1;
            P.pieces.push_back(pc);
        }
        rider_lane = l;
        P.tile_row[(size_t)tile * MAX_ROWS + tile_rows] = rows[i];
        P.tile_out[(size_t)tile * MAX_ROWS + tile_rows] = i;
        tile_rows++;
        P.nriders++;
        return true;
    };
    auto open_tile_storage = [&]() {
        if ((int)P.tile_row.size() < (tile + 1) * MAX_ROWS) {
            P.tile_row.resize((size_t)(tile + 1) * MAX_ROWS, -1);
            P.tile_out.resize((size_t)(tile + 1) * MAX_ROWS, 0);
        }
    };
    for (int i = 0; i < nrows; i++) {
        /* split_jump > 0: a jump of at least that many rows in the list closes the tile (see the function's header) */
        if (split_jump > 0 && i > 0 && tile_rows > 0 && rows[i] - rows[i - 1] >= split_jump) close_tile();
        for (int attempt = 0; attempt < 2; attempt++) {
            if (tile_res >= max_rows || tile_rows > tile_res) { /* no further resident: a rider, or the next tile */
                open_tile_storage();
                if (try_rider(i)) break;
                close_tile();
            }
            open_tile_storage();
            /* remember the cursor so the row can be undone if it does not fit in this tile */
            const size_t mark = P.pieces.size();
            const int s_lane = lane, s_free = freeb, s_npl = npl;
            int remaining = nwin[i], p0 = 0;
            bool fits = true;
            while (remaining > 0) {
                const int need = (remaining + L - 1 + W - 1) / W;
                /* do not split off a sliver: every split costs L-1 overlapping bases and makes the
                 * tile take the several-pieces-per-lane path; a partial piece must hold >= 3W windows
                 * (config 2 with 10-window slivers in the 2 spare bit rows: 119 ms instead of 113) */
                const int want = need < freeb ? need : freeb;
                const int room = want * W - (L - 1); /* windows a piece of `want` bit rows can own */
                const int cnt_here = room >= remaining ? remaining : room / own_mult * own_mult;
                if (freeb < min_bits || npl >= MAX_PIECES || (want < need && cnt_here < 3 * W)) {
                    new_lane();
                    if (lane >= LANES) { fits = false; break; }
                    continue;
                }
                Piece pc;
                pc.lane = tile * LANES + lane;
                pc.b0 = 32 - freeb;
                pc.nb = want;
                pc.slot = tile_rows;
                pc.row = rows[i];
                pc.p0 = p0;
                pc.cnt = cnt_here;
                pc.rider = 0;
                P.pieces.push_back(pc);
                lane_used[lane] += want;
                lane_np[lane]++;
                freeb -= want;
                npl++;
                p0 += cnt_here;
                remaining -= cnt_here;
            }
            if (fits) {
                P.tile_row[(size_t)tile * MAX_ROWS + tile_rows] = rows[i];
                P.tile_out[(size_t)tile * MAX_ROWS + tile_rows] = i;
                tile_rows++;
                tile_res++;
                break;
            }
            /* undo and retry in a fresh tile (a row needs at most 7 lanes, it always fits there) -- unless it rides here */
            for (size_t k = mark; k < P.pieces.size(); k++) {
                lane_used[P.pieces[k].lane % LANES] -= P.pieces[k].nb;
                lane_np[P.pieces[k].lane % LANES]--;
            }
            P.pieces.resize(mark);
            lane = s_lane; freeb = s_free; npl = s_npl;
            if (try_rider(i)) break;
            close_tile();
        }
    }
    if (tile_rows > 0 || P.tile_nrows.empty()) close_tile();
    P.ntiles = (int)P.tile_nrows.size();
    if (P.nriders > 0) /* (the riders' pieces were appended behind their tile's residents) */
        std::stable_sort(P.pieces.begin(), P.pieces.end(), [](const Piece &a, const Piece &b) {
            return a.lane != b.lane ? a.lane < b.lane : a.b0 < b.b0;
        });
    P.tile_row.resize((size_t)P.ntiles * MAX_ROWS, -1);
    P.tile_out.resize((size_t)P.ntiles * MAX_ROWS, 0);
    P.tile_amax.assign((size_t)P.ntiles, -1);
    long lanes = 0;
    int last_lane = -1;
    for (const Piece &pc : P.pieces) {
        int &am = P.tile_amax[(size_t)(pc.lane / LANES)];
        if (pc.row > am) am = pc.row;
        if (pc.lane != last_lane) { lanes++; last_lane = pc.lane; }
    }
    P.lanes_used = lanes;
    return P;
}

/* work items of a launch that visits, for every tile, the columns 0 .. its largest row (the triangle) */
inline long long triangle_items(const Packing &P)
{
    long long items = 0;
    for (int t = 0; t < P.ntiles; t++) items += (long long)P.tile_amax[(size_t)t] + 1;
    return items;
}

/* relative cost of running the kernel with this packing: lanes x (per-word cost x W + fixed
 * per-shift cost), in VALU instructions per shift (18 per word, ~25 per shift: DESIGN.md §5) */
inline double packing_cost(const Packing &P) { return (double)P.ntiles * LANES * (18.0 * P.W + 25.0); }

/* What the same-length kernel variant (k_gram_bitslice, PK = 4 and 5) asks of a piece, checked before every launch
 * (gkm_gram.hip plan_bitslice).  row_windows: l-mers of the piece's row.  0 = fine, 1 = not the layout the origin word and
 * the tags describe, 2 = a group of own_mult windows that the piece owns in part reaches past the L - 1 zero bytes behind the
 * row's last l-mer in the positional weight table (the counting loop applies row validity per group).
 *   resident  starts at bit row 0 and at a multiple of the lane capacity; owns at most the capacity (positions at or above
 *             it are unowned whole groups), and a multiple of own_mult unless it finishes its row;
 *   rider     bit rows RIDER_B0, RIDER_B0 + 1; starts at a multiple of rider_w in its row and owns exactly rider_w windows
 *             unless it finishes the row -- all of them in bit row RIDER_B0, each with its L bases inside the two bit rows;
 *   either    the windows that round its last group up to own_mult number at most L - 1 and lie behind the row's end. */
inline int same_length_piece_check(const Piece &pc, int row_windows, int W, int L, int own_mult, int rider_w)
{
    const int cap = (32 * W - (L - 1)) / own_mult * own_mult;
    const bool finishes = pc.p0 + pc.cnt == row_windows;
    const int over = (pc.cnt + own_mult - 1) / own_mult * own_mult - pc.cnt;
    if (pc.cnt <= 0 || pc.p0 < 0 || pc.p0 + pc.cnt > row_windows) return 1;
    if (!pc.rider) {
        if (pc.b0 != 0 || pc.p0 % cap != 0 || pc.p0 / cap > 7 || (pc.cnt % own_mult != 0 && !finishes)) return 1;
        if (pc.cnt > cap) return 2;
    } else {
        if (rider_w <= 0 || rider_w % own_mult != 0 || rider_w > W || rider_w + L - 1 > RIDER_NB * W) return 1;
        if (pc.b0 != RIDER_B0 || pc.nb != RIDER_NB || pc.p0 % rider_w != 0 || pc.cnt > rider_w || (pc.cnt != rider_w && !finishes))
            return 1;
    }
    if (over != 0 && (!finishes || over > L - 1)) return 2;
    return 0;
}

/* ... and of the packing as a whole: every lane holds at most one resident piece and at most one rider piece, the rider
 * piece above the resident's last bit row, in a tile whose rows number at most max_slots.  0 or the code of the first
 * piece that fails (3: lanes). */
inline int same_length_packing_check(const Packing &P, const int *row_windows_by_piece, int own_mult, int rider_w, int max_slots)
{
    for (size_t k = 0; k < P.pieces.size(); k++) {
        const Piece &pc = P.pieces[k];
        const int rc = same_length_piece_check(pc, row_windows_by_piece[k], P.W, P.L, own_mult, rider_w);
        if (rc) return rc;
        if (pc.slot < 0 || pc.slot >= max_slots) return 3;
        const bool same_lane = k > 0 && P.pieces[k - 1].lane == pc.lane;
        if (!pc.rider && same_lane) return 3;
        if (pc.rider && (!same_lane || P.pieces[k - 1].rider || P.pieces[k - 1].b0 + P.pieces[k - 1].nb > RIDER_B0)) return 3;
    }
    return 0;
}

} /* namespace gkmpack */
#endif
