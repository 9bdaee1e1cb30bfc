"""Riders of the same-length Gram kernel, host side (gkm_pack.h pack_rows rider_w, RIDER_B0): rows that live in bit rows 30
and 31 of the lanes whose own piece ends below them, ten owned windows per lane.  Through bitslice_cpu_probe.so:
the layout (every row in exactly one tile, the pieces' ownership, planes / packed positions / tags rebuilt from it), the
tile counts, byte-identity with the packing without riders where no bit rows are to spare, the pre-launch check that
gkm_gram.hip plan_bitslice calls (gkm_pack.h same_length_packing_check: the function itself, on good layouts and on
broken ones), and the lane program run on the CPU over a layout with riders against the oracle."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers

W = 10
MAX_ROWS = 128
SHAPES = [(300, 11), (300, 10), (600, 10)]


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    return lib


def _consts(probe):
    return [probe.packprobe_rider_consts(i) for i in range(4)]   # RIDER_B0, RIDER_NB, RIDER_W, RIDER_SLOTS


def _pack(probe, rows, length, L, rider_w, split_jump=0):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    nwin = np.full(len(rows), length - L + 1, dtype=np.int32)
    max_pieces, max_tiles = 64 * (len(rows) // 16 + 4), len(rows) // 16 + 4
    pieces = np.zeros((max_pieces, 8), dtype=np.int32)
    tags = np.zeros(max_pieces, dtype=np.int32)
    trow = np.zeros((max_tiles, MAX_ROWS), dtype=np.int32)
    tout = np.zeros((max_tiles, MAX_ROWS), dtype=np.int32)
    tn = np.zeros(max_tiles, dtype=np.int32)
    nt, nr, chk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(-1)
    vp = ctypes.c_void_p
    npc = probe.packprobe_same_length(rows.ctypes.data_as(vp), nwin.ctypes.data_as(vp), len(rows), L, rider_w, split_jump,
                                      pieces.ctypes.data_as(vp), max_pieces, tags.ctypes.data_as(vp),
                                      trow.ctypes.data_as(vp), tout.ctypes.data_as(vp), tn.ctypes.data_as(vp), max_tiles,
                                      ctypes.byref(nt), ctypes.byref(nr), ctypes.byref(chk))
    assert npc >= 0
    return dict(pieces=pieces[:npc], tags=tags[:npc], tile_row=trow[:nt.value], tile_out=tout[:nt.value],
                tile_nrows=tn[:nt.value], ntiles=nt.value, nriders=nr.value, check=chk.value)


@pytest.mark.parametrize("length,L", SHAPES)
def test_layout_with_riders(probe, length, L):
    """150 rows with a jump in the list: every row in exactly one tile as a resident or as a rider, every window owned once,
    rider pieces of RIDER_W windows except a rider's last, planes / packed positions / tags rebuilt from the layout give
    back the row's bases and ownership, and the pre-launch check accepts it."""
    B0, NB, RW, SLOTS = _consts(probe)
    rows = np.concatenate([np.arange(0, 100), np.arange(300, 350)]).astype(np.int32)
    nwin = length - L + 1
    rng = np.random.default_rng(length * 100 + L)
    n = 350
    seqs = [rng.integers(0, 4, length).astype(np.uint8) for _ in range(n)]
    codes = np.concatenate(seqs)
    off = np.arange(n + 1, dtype=np.int64) * length
    for split in (0, 64):
        lay = _pack(probe, rows, length, L, RW, split)
        assert lay["check"] == 0
        pcs, tags = lay["pieces"], lay["tags"]
        # every row of the list in exactly one slot of one tile
        seen = []
        for t in range(lay["ntiles"]):
            nr = lay["tile_nrows"][t]
            assert 0 < nr <= SLOTS
            seen += list(lay["tile_row"][t, :nr])
            assert (rows[lay["tile_out"][t, :nr]] == lay["tile_row"][t, :nr]).all()
            assert (lay["tile_row"][t, nr:] == -1).all()
            assert (np.diff(lay["tile_row"][t, :nr]) > 0).all()          # row order: the tile's column range stays tight
        assert sorted(seen) == sorted(rows) and len(seen) == len(rows)
        # windows owned exactly once; a row's pieces in one tile; riders above the residents' slots
        owned = {int(r): np.zeros(nwin, dtype=np.int32) for r in rows}
        tile_of = {}
        for (lane, b0, nb, slot, row, p0, cnt, rider), tag in zip(pcs, tags):
            t = lane // 64
            assert lay["tile_row"][t, slot] == row
            assert tile_of.setdefault(int(row), t) == t
            owned[int(row)][p0:p0 + cnt] += 1
            if rider:
                assert (b0, nb) == (B0, NB) and p0 % RW == 0
                assert cnt == RW or (p0 + cnt == nwin and 0 < cnt < RW)
                assert probe.packprobe_rider_tag_slot(int(tag)) == slot
                # a trip's row weight is at "base + i0": lane position B0 * W + w is l-mer p0 + w of the rider
                assert probe.packprobe_rider_tag_pos(int(tag)) + B0 * W == p0
            else:
                assert b0 == 0 and tag == 0
        assert all((v == 1).all() for v in owned.values())
        if length == 300:
            assert lay["nriders"] > 0
        else:
            assert lay["nriders"] == 0      # 600 bp at L = 10: 32 lanes with three spare bit rows, a rider needs 60
        # the lanes' images, rebuilt as k_build_rowplanes does
        vp = ctypes.c_void_p
        for lane in np.unique(pcs[:, 0]):
            mine = np.ascontiguousarray(pcs[pcs[:, 0] == lane])
            assert len(mine) <= 2 and not mine[0, 7] and (len(mine) == 1 or (mine[1, 7] and mine[0, 2] <= B0))
            planes = np.zeros((3, W), dtype=np.uint32)
            pk = np.zeros(2 * W + 2, dtype=np.uint32)
            probe.packprobe_lane_image(codes.ctypes.data_as(vp), off.ctypes.data_as(vp), mine.ctypes.data_as(vp), len(mine), W,
                                       planes.ctypes.data_as(vp), pk.ctypes.data_as(vp))
            own = np.zeros(32 * W, dtype=bool)
            base = np.zeros(32 * W, dtype=np.uint8)
            for (_, b0, nb, slot, row, p0, cnt, rider) in mine:
                own[b0 * W:b0 * W + cnt] = True
                m = min(nb * W, length - p0)
                base[b0 * W:b0 * W + m] = seqs[row][p0:p0 + m]
            i = np.arange(32 * W)
            bit = lambda pl: (planes[pl][i % W] >> (i // W).astype(np.uint32)) & 1
            assert (bit(2).astype(bool) == own).all()
            assert ((bit(0) << 1 | bit(1)).astype(np.uint8) == base).all()
            assert (((pk[i >> 4] >> (2 * (i & 15)).astype(np.uint32)) & 3).astype(np.uint8) == base).all()


def test_seventy_rows_of_300_bp_make_66_plus_4(probe):
    B0, NB, RW, SLOTS = _consts(probe)
    for L in (11, 10):
        lay = _pack(probe, np.arange(70), 300, L, RW)
        assert list(lay["tile_nrows"]) == [66, 4] and lay["nriders"] == 2 and lay["check"] == 0
        riders = lay["pieces"][lay["pieces"][:, 7] == 1]
        assert sorted(set(riders[:, 4])) == [64, 65] and sorted(set(riders[:, 3])) == [64, 65]
        assert len(riders) == 2 * -(-(300 - L + 1) // RW)            # 29 lanes each at L = 11, 30 at L = 10
        assert len(set(riders[:, 0])) == len(riders)                  # one rider piece per lane
    # 10 000 rows: 152 tiles instead of 157
    assert _pack(probe, np.arange(10000), 300, 11, RW)["ntiles"] == 152
    assert _pack(probe, np.arange(10000), 300, 11, 0)["ntiles"] == 157
    # 67 rows: both riders whole in the first tile, one row left
    assert list(_pack(probe, np.arange(67), 300, 11, RW)["tile_nrows"]) == [66, 1]
    assert list(_pack(probe, np.arange(65), 300, 11, RW)["tile_nrows"]) == [65]
    # Two-lane residents never meet riders: a second lane with four or more bit rows to spare takes the next row's first
    # piece (330 bp: 310 + 10 windows, then 290 of the next row in the same lane -- several pieces per lane, the packed
    # variants), and one with two or three (570-600 bp) is one of 32 such lanes where a rider needs 56-60
    for length in (330, 450, 570, 590, 600):
        lay = _pack(probe, np.arange(80), length, 11, RW)
        assert lay["nriders"] == 0, length


@pytest.mark.parametrize("length,L", [(320, 11), (310, 11), (600, 10), (300, 12)])
def test_no_spare_bit_rows_no_change(probe, length, L):
    """320 bp at L = 11 uses all 32 bit rows, 310 bp needs 31 (one spare: not enough), a 600-bp row's second lane has three to
    spare but a tile has only 32 such lanes, L = 12 leaves no room for a piece's overlap: byte-identical to the packing
    without riders."""
    RW = _consts(probe)[2]
    rows = np.concatenate([np.arange(0, 150), np.arange(400, 470)])
    a, b = _pack(probe, rows, length, L, RW, 64), _pack(probe, rows, length, L, 0, 64)
    assert a["nriders"] == 0 and a["check"] == 0 and b["check"] == 0
    for key in ("pieces", "tags", "tile_row", "tile_out", "tile_nrows"):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("L,d", [(11, 3), (10, 3)])
def test_lane_program_over_a_layout_with_riders_matches_oracle(probe, L, d):
    """70 rows of 300 bp packed with riders (66 + 4), run through the lane program on the CPU: the rider pieces' windows are
    found by the same counting code and attributed to the riders' rows."""
    from oracle import oracle as O
    rng = np.random.default_rng(17 * L + d)
    n = 70
    seqs = [rng.integers(0, 4, 300).astype(np.uint8) for _ in range(n)]
    seqs[65] = seqs[3].copy()
    seqs[64][:] = 0                                    # a poly-A rider: every window a hit against itself
    codes = np.concatenate(seqs)
    off = np.arange(n + 1, dtype=np.int64) * 300
    rows = np.arange(n, dtype=np.int32)
    vp = ctypes.c_void_p
    for t in (2, 4):
        wd = None
        if t == 4:
            wt = O.position_weights(t, 2 * 151 + 1)
            wd = np.ascontiguousarray(wt[151:])
        opt = O.make_opt(t, L, L - d, d)
        for col in (3, 64, 69):
            P = np.zeros((n, d + 1), dtype=np.int32)
            used = ctypes.c_int(0)
            rc = probe.bsprobe_profile_riders(W, L, d, codes.ctypes.data_as(vp), off.ctypes.data_as(vp), rows.ctypes.data_as(vp),
                                              n, col, wd.ctypes.data_as(vp) if wd is not None else None,
                                              P.ctypes.data_as(vp), ctypes.byref(used))
            assert rc == 0, "packing invariant %d violated" % rc
            assert used.value == 64 + 4
            for i in (0, 3, 63, 64, 65, 66, 69):
                want = np.zeros(d + 1, dtype=np.int32)
                O.lib().gkmo_profile(ctypes.byref(opt), seqs[i].ctypes.data_as(vp), 300, seqs[col].ctypes.data_as(vp), 300,
                                     want.ctypes.data_as(vp))
                assert (P[i] == want).all(), (t, col, i)


def test_the_pre_launch_check_refuses_broken_layouts(probe):
    """gkm_pack.h same_length_packing_check, the function plan_bitslice calls: 0 on what pack_rows builds, and the right code
    on layouts broken one rule at a time (1: not the layout the tags describe, 2: a group owned in part reaches past the
    weight table's zero guard, 3: lanes or slots)."""
    B0, NB, RW, SLOTS = _consts(probe)
    vp = ctypes.c_void_p

    def check(pcs, nwin, L, rider_w=RW, slots=SLOTS):
        pcs = np.ascontiguousarray(pcs, dtype=np.int32)
        return probe.packprobe_check_layout(pcs.ctypes.data_as(vp), len(pcs), nwin, L, rider_w, slots)

    for L in (11, 10):
        nwin = 300 - L + 1
        good = _pack(probe, np.arange(70), 300, L, RW)["pieces"]
        assert check(good, nwin, L) == 0
        first = int(np.flatnonzero(good[:, 7] == 1)[0])            # the first rider piece (p0 = 0, cnt = RW)
        last = int(np.flatnonzero(good[:, 7] == 1)[-1])            # the last piece of the second rider

        def broken(k, col, val):
            b = good.copy()
            b[k, col] = val
            return b

        assert check(broken(first, 1, B0 - 1), nwin, L) == 1       # not in bit rows 30, 31
        assert check(broken(first, 2, 1), nwin, L) == 1            # one bit row: no room for the overlap
        assert check(broken(first, 6, RW - 3), nwin, L) == 1       # short without finishing the row
        assert check(broken(first, 5, 3), nwin, L) == 1            # not at a multiple of RW in its row
        assert check(broken(first, 6, RW + 1), nwin, L) == 1       # more windows than bit row 30 holds
        assert check(good, nwin, L, rider_w=0) == 1                # rider pieces in a launch that takes none
        assert check(broken(first, 3, SLOTS), nwin, L) == 3        # a slot the output has no room for
        assert check(broken(first - 1, 2, B0 + 1), nwin, L) == 3   # the resident below reaches into bit row 30
        two = np.insert(good, first + 1, good[first], axis=0)
        assert check(two, nwin, L) == 3                            # two rider pieces in one lane
        assert check(np.delete(good, first - 1, axis=0), nwin, L) == 3   # a rider piece in a lane without a resident
        assert check(np.insert(good, 1, good[0], axis=0), nwin, L) == 3  # two residents in one lane
        # (a group that needs more zeros than L - 1 cannot be built at groups of five and L >= 5: code 2 is reached through
        # the capacity); told that the rows are longer, the riders' last pieces no longer finish them
        cap = (32 * W - (L - 1)) // 5 * 5
        assert check(broken(0, 6, cap + 5), cap + 5, L) == 2       # a resident that owns positions at or above the capacity
        assert good[last, 5] + good[last, 6] == nwin
        if nwin % 5:                                               # (L = 10: 291 windows, the last pieces own one)
            assert check(good, nwin + 5, L) == 1
