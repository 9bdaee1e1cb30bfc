"""Shift records on the CPU (gkm_bitslice.h shift_record_live / shift_record_visit: what k_gram_bitslice PK = 6 and 7 put
between the counting loop and the hit path), through bitslice_cpu_probe.so:

  - one record through visit after visit: every (bit row, group) the two words flag is visited exactly once, group 0's bit
    rows first, ascending, then group 1's;
  - on random planes and on planes the tables build, the visits of a shift's record cover every (bit row, group) in which
    window_hits -- the specification -- finds a hit;
  - push, visit and re-push between the lane program's counting and its hit path, over the packing of a same-length launch,
    against the oracle's profiles for (11,3), (10,3) and (12,4): T = L .. L + 4, dense rows whose records carry both groups
    and many bit rows, rider pieces, trips of 1, 3 and 64 records."""
import ctypes
import os

import numpy as np
import pytest

from tests import dense_inputs as D
from tests import helpers

W, GRP = 10, 5
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_shift_record_drain.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    lib.bsprobe_lowest_bit_or_ones.argtypes = [ctypes.c_uint32]
    lib.bsprobe_lowest_bit_or_ones.restype = ctypes.c_uint32
    lib.bsprobe_group_any.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 8
    lib.bsprobe_row_planes.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    lib.bsprobe_sb_words.argtypes = [vp] + [ctypes.c_int] * 5 + [vp] * 2
    lib.bsprobe_profile_shift_records.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp,
                                                  ctypes.c_int, ctypes.c_int, vp, vp, vp]
    return lib


def _bits(x):
    return [b for b in range(32) if (int(x) >> b) & 1]


def _drain(probe, any0, any1):
    bits, w0 = np.full(64, -1, dtype=np.int32), np.full(64, -1, dtype=np.int32)
    n = probe.bsprobe_shift_record_drain(int(any0), int(any1), bits.ctypes.data, w0.ctypes.data)
    return list(zip(bits[:n].tolist(), w0[:n].tolist()))


def test_a_record_is_visited_bit_row_by_bit_row(probe):
    rng = np.random.default_rng(5)
    words = [0, 1, 0x80000000, 0xFFFFFFFF, 0xC0000000, 0x3FFFFFFF, 0x55555555]
    words += [int(x) for x in rng.integers(0, 2 ** 32, 40, dtype=np.uint64)]
    words += [int(a & b & c) for a, b, c in rng.integers(0, 2 ** 32, (40, 3), dtype=np.uint64)]    # sparse ones
    for any0 in words:
        for any1 in words:
            want = [(b, 0) for b in _bits(any0)] + [(b, GRP) for b in _bits(any1)]
            assert _drain(probe, any0, any1) == want, (hex(any0), hex(any1))
    assert _drain(probe, 0, 0) == []
    assert probe.bsprobe_lowest_bit_or_ones(0) == 0xFFFFFFFF and probe.bsprobe_lowest_bit_or_ones(0x80000000) == 31


@pytest.mark.parametrize("L,d", [(11, 3), (10, 3), (12, 4)])
def test_visits_cover_the_hits_of_window_hits(probe, L, d):
    """hit_or[g] = OR of window_hits' words of group g (the specification), any[g] what the counting loop hands the push:
    the record's visits are exactly the flagged (bit row, group) pairs, and no pair with a hit is missing."""
    rng = np.random.default_rng(100 * L + d)
    hit_or, any_ = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    top = ctypes.c_int(0)
    cases = []
    for _ in range(60):                                   # random planes, random validity
        ahi, alo, bhi, blo = (rng.integers(0, 2 ** 32, W, dtype=np.uint64).astype(np.uint32) for _ in range(4))
        av = rng.integers(0, 2 ** 32, W, dtype=np.uint64).astype(np.uint32)
        for i in range(32 * W - (L - 1), 32 * W):           # nobody owns a window at or above the lane capacity 32 W - (L - 1)
            av[i % W] &= ~np.uint32(1 << (i // W))
        cases.append((ahi, alo, av, bhi, blo))
    planes = np.zeros(3 * W, dtype=np.uint32)
    for row, col in ((D.repeat((D.A, D.T), 300), D.repeat((D.A, D.T), 300)), (D.homopolymer(D.A, 300), D.spliced(300, L, 3)),
                     (D.spliced(300, L, 4), D.spliced(300, L, 4)), (D.repeat(D.unit_of(3, 1), 200), D.repeat(D.unit_of(3, 1), L + 2))):
        probe.bsprobe_row_planes(row.ctypes.data, len(row), 0, W, L, planes.ctypes.data)
        T = len(col)
        hi, lo = np.zeros(T + W, np.uint32), np.zeros(T + W, np.uint32)
        for strand in (0, 1):
            probe.bsprobe_sb_words(col.ctypes.data, T, strand, W, L, T + W, hi.ctypes.data, lo.ctypes.data)
            for delta in range(0, T, 7):
                cases.append((planes[:W].copy(), planes[W:2 * W].copy(), planes[2 * W:].copy(), hi[delta:delta + W].copy(),
                              lo[delta:delta + W].copy()))
    both = many = 0
    for ahi, alo, av, bhi, blo in cases:
        assert probe.bsprobe_group_any(L, d, ahi.ctypes.data, alo.ctypes.data, av.ctypes.data, bhi.ctypes.data, blo.ctypes.data,
                                       hit_or.ctypes.data, any_.ctypes.data, ctypes.addressof(top)) == 0
        visits = _drain(probe, any_[0], any_[1])
        assert visits == [(b, 0) for b in _bits(any_[0])] + [(b, GRP) for b in _bits(any_[1])]
        assert len(set(visits)) == len(visits)
        for g in range(2):
            assert all((b, g * GRP) in visits for b in _bits(hit_or[g]))
        both += bool(any_[0]) and bool(any_[1])
        many += len(visits) > 8
    assert both > 10 and many > 10                        # records with both groups, records with many bit rows


def _oracle_profile(O, opt, a, b, d):
    want = np.zeros(d + 1, dtype=np.int32)
    O.lib().gkmo_profile(ctypes.byref(opt), a.ctypes.data_as(vp), len(a), b.ctypes.data_as(vp), len(b), want.ctypes.data_as(vp))
    return want


def _run(probe, L, d, seqs, col, wd, riders, trip):
    n, T = len(seqs), len(seqs[0])
    codes = np.concatenate(seqs)
    off = np.arange(n + 1, dtype=np.int64) * T
    rows = np.arange(n, dtype=np.int32)
    P = np.zeros((n, d + 1), dtype=np.int32)
    used = ctypes.c_int(0)
    visits = np.zeros(3, dtype=np.int64)
    rc = probe.bsprobe_profile_shift_records(L, d, codes.ctypes.data, off.ctypes.data, rows.ctypes.data, n, col,
                                             wd.ctypes.data if wd is not None else None, riders, trip, P.ctypes.data,
                                             ctypes.addressof(used), visits.ctypes.data)
    assert rc == 0, "code %d" % rc
    pushed, visited, again = (int(x) for x in visits)
    assert visited == pushed + again                       # every visit takes a fresh record or one that was put back
    return P, pushed, again


def _weights(O, t):
    if t != 4:
        return None
    return np.ascontiguousarray(O.position_weights(t, 2 * 151 + 1)[151:])


@pytest.mark.parametrize("L,d", [(11, 3), (10, 3), (12, 4)])
def test_shortest_columns_match_the_oracle(probe, L, d):
    """T = L .. L + 4: one to five windows per sequence, every shift wraps around the strand's end."""
    from oracle import oracle as O
    for T in range(L, L + 5):
        rng = np.random.default_rng(31 * T + d)
        seqs = [rng.integers(0, 4, T).astype(np.uint8) for _ in range(6)]
        seqs += [D.homopolymer(D.A, T), D.repeat((D.A, D.T), T), seqs[0].copy(), D.rc(seqs[1])]
        for t in (2, 4):
            opt, wd = O.make_opt(t, L, L - d, d), _weights(O, t)
            for col in (0, 6, 7, 9):
                for trip in (1, 64):
                    P, _, _ = _run(probe, L, d, seqs, col, wd, 0, trip)
                    for i in range(len(seqs)):
                        assert (P[i] == _oracle_profile(O, opt, seqs[i], seqs[col], d)).all(), (T, t, col, trip, i)


@pytest.mark.parametrize("L,d", [(11, 3), (10, 3), (12, 4)])
def test_dense_rows_match_the_oracle(probe, L, d):
    """Two-letter and low-complexity rows of 300 bases against such columns: a shift's record carries both groups and up to
    30 bit rows, so most visits take a record that was put back; trips of 1, 3 and 64 records visit them in different
    orders and add up to the same profiles."""
    from oracle import oracle as O
    T = 300
    seqs = [D.homopolymer(D.A, T), D.repeat((D.A, D.T), T), D.repeat((D.A, D.C), T), D.repeat(D.unit_of(3, 2), T),
            D.spliced(T, L, 9), D.spliced(T, L, 10), D.repeat(D.unit_of(L, 2), T)]
    seqs.append(D.substituted(seqs[4], d, L, 1))
    for t in (2, 4):
        opt, wd = O.make_opt(t, L, L - d, d), _weights(O, t)
        for col in (1, 3, 4):
            want = [_oracle_profile(O, opt, s, seqs[col], d) for s in seqs]
            for trip in (1, 3, 64):
                P, pushed, again = _run(probe, L, d, seqs, col, wd, 0, trip)
                assert again > pushed                      # records with several bit rows went back more often than not
                for i in range(len(seqs)):
                    assert (P[i] == want[i]).all(), (t, col, trip, i)


@pytest.mark.parametrize("L,d", [(11, 3), (10, 3)])
def test_rider_pieces_match_the_oracle(probe, L, d):
    """70 rows of 300 bases packed as a launch with riders packs them (64 residents, rows 64 and 65 in bit rows 30 and 31):
    the riders' windows arrive in the same records as the residents' and are attributed to the riders' rows."""
    from oracle import oracle as O
    rng = np.random.default_rng(17 * L + d)
    n = 70
    seqs = [rng.integers(0, 4, 300).astype(np.uint8) for _ in range(n)]
    seqs[65] = seqs[3].copy()
    seqs[64][:] = 0                                        # a poly-A rider: every window a hit against itself
    seqs[2] = D.repeat((D.A, D.T), 300)
    for t in (2, 4):
        opt, wd = O.make_opt(t, L, L - d, d), _weights(O, t)
        for col in (3, 64, 2):
            P, pushed, again = _run(probe, L, d, seqs, col, wd, 1, 64)
            assert pushed > 0
            for i in (0, 2, 3, 63, 64, 65, 66, 69):
                assert (P[i] == _oracle_profile(O, opt, seqs[i], seqs[col], d)).all(), (t, col, i)
