"""window_group_any (gkm_bitslice.h) -- what the hot kernel's counting loop calls -- against its specification: the OR per
group of five words of window_hits' hit words (column-side validity left to the trip, as the kernel calls it).

Where the bias beta = 2^(P-1) - (L - d), P = bitlen(L), is 0 or 1 and L + beta < 2^P, window_group_any counts MATCHES and
a hit is the top plane of the biased count; everywhere else it is window_hits followed by the OR.  TOP_PLANE below states
which (L, d) of the device table take which path; the three bench workloads -- (11,3), (10,3), (12,4) -- must take the
top-plane one.

The two entries are required to agree on every bit that a validity plane AV built by the tables lets through: windows
i < segment_capacity(W, L).  Beyond it they MAY differ: the extension words' bit row 31 is shifted in as a match by
window_hits and as a mismatch by window_group_any; both are fiction about bases behind the lane, and row_plane_word /
piece_bit never own such a window (asserted here)."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers

W, GRP = 10, 5
# the table behind gkm_pick_bitslice (gkm_gram_bitslice.hip): 5 <= L <= 12 x d <= 4, plus three d > 4 pairs
TABLE = [(L, d) for L in range(5, 13) for d in range(5)] + [(11, 5), (12, 5), (12, 6)]


def _bitlen(v):
    return int(v).bit_length()


def _top_plane(L, d):
    beta = (1 << (_bitlen(L) - 1)) - (L - d)
    return beta in (0, 1) and L + beta < (1 << _bitlen(L))


# beta = 0: (5,1) (6,2) (7,3) (8,0) (9,1) (10,2) (11,3) (12,4); beta = 1: (5,2) (6,3) (8,1) (9,2) (10,3) (11,4) (12,5);
# (7,4) has beta = 1 but 7 + 1 does not fit three planes
TOP_PLANE = {(5, 1), (6, 2), (7, 3), (8, 0), (9, 1), (10, 2), (11, 3), (12, 4),
             (5, 2), (6, 3), (8, 1), (9, 2), (10, 3), (11, 4), (12, 5)}


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    lib.bsprobe_row_planes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.bsprobe_sb_words.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    lib.bsprobe_piece_valid.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return lib


def _cap(L):
    return 32 * W - (L - 1)


def _cap_words(L):
    """AV with every window start i = b * W + w < segment_capacity set."""
    out = np.zeros(W, dtype=np.uint32)
    for w in range(W):
        for b in range(32):
            if b * W + w < _cap(L):
                out[w] |= np.uint32(1 << b)
    return out


def _cap_groups(L):
    """per group: the bit rows whose five windows all lie inside the capacity"""
    cw = _cap_words(L)
    return np.array([np.bitwise_and.reduce(cw[g * GRP:(g + 1) * GRP]) for g in range(W // GRP)], dtype=np.uint32)


class _Runner:
    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.hit_or = np.zeros(W // GRP, dtype=np.uint32)
        self.any = np.zeros(W // GRP, dtype=np.uint32)
        self.top = ctypes.c_int(-1)
        self._ho, self._an, self._tp = self.hit_or.ctypes.data, self.any.ctypes.data, ctypes.addressof(self.top)

    def __call__(self, ahi, alo, av, bhi, blo):
        """addresses of W words each -> (OR of window_hits per group, window_group_any), copies"""
        rc = self.probe.bsprobe_group_any(self.L, self.d, ahi, alo, av, bhi, blo, self._ho, self._an, self._tp)
        assert rc == 0, (self.L, self.d)
        return self.hit_or, self.any


def test_which_pairs_take_the_top_plane_path(probe):
    assert {(L, d) for (L, d) in TABLE if _top_plane(L, d)} == TOP_PLANE
    assert {(11, 3), (10, 3), (12, 4)} <= TOP_PLANE
    z = np.zeros(W, dtype=np.uint32)
    for L, d in TABLE:
        r = _Runner(probe, L, d)
        r(z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data)
        assert bool(r.top.value) == ((L, d) in TOP_PLANE), (L, d)
    # a pair outside the device table is refused, not served by something else
    r = _Runner(probe, 4, 1)
    assert probe.bsprobe_group_any(4, 1, *([z.ctypes.data] * 5), r._ho, r._an, r._tp) == 1


def test_no_table_built_validity_plane_owns_a_window_beyond_the_capacity(probe):
    """row_plane_word (one sequence per lane) and piece_bit (packed lanes, any piece the packer may emit: cnt <= nb * W -
    (L - 1), bit rows inside the lane) set no validity bit at i >= segment_capacity -- the only windows on which the two
    entries may differ."""
    rng = np.random.default_rng(5)
    out = np.zeros(3 * W, dtype=np.uint32)
    pv = np.zeros(W, dtype=np.uint32)
    for L in range(5, 13):
        inside = _cap_words(L)
        for n in (L, L + 4, 300, _cap(L) + L - 1, _cap(L) + L, 600, 2047):
            codes = rng.integers(0, 4, n).astype(np.uint8)
            for s0 in range(0, n - L + 1, _cap(L)):
                probe.bsprobe_row_planes(codes.ctypes.data, n, s0, W, L, out.ctypes.data)
                assert not (out[2 * W:] & ~inside).any(), (L, n, s0)
        for b0 in range(32):
            for nb in range(1, 32 - b0 + 1):
                top = nb * W - (L - 1)
                if top <= 0:
                    continue
                for cnt in {1, top, max(1, top - 1), max(1, top // 2)}:
                    probe.bsprobe_piece_valid(b0, nb, cnt, W, pv.ctypes.data)
                    assert not (pv & ~inside).any(), (L, b0, nb, cnt)
                    assert sum(bin(int(x)).count("1") for x in pv) == cnt


@pytest.mark.parametrize("L,d", TABLE)
def test_random_planes_random_validity_inside_the_capacity(probe, L, d):
    rng = np.random.default_rng(100 * L + d)
    r = _Runner(probe, L, d)
    inside = _cap_words(L)
    flagged = 0
    for trial in range(3000):
        p = rng.integers(0, 1 << 32, (5, W), dtype=np.uint64).astype(np.uint32)
        if trial % 3 == 1:      # near-identical planes: many windows at and around the threshold
            noise = rng.integers(0, 1 << 32, (3, 2, W), dtype=np.uint64).astype(np.uint32)
            p[3] = p[0] ^ (noise[0, 0] & noise[1, 0] & noise[2, 0])
            p[4] = p[1] ^ (noise[0, 1] & noise[1, 1] & noise[2, 1])
        if trial % 3 == 2:
            p[2] = 0xFFFFFFFF
        p[2] &= inside
        p = np.ascontiguousarray(p)
        a = p.ctypes.data
        ho, an = r(a, a + 4 * W, a + 8 * W, a + 12 * W, a + 16 * W)
        assert (ho == an).all(), (trial, [hex(int(x)) for x in ho], [hex(int(x)) for x in an])
        flagged += int(ho.any())
    assert flagged > 100       # the comparison saw hits, not only empty words


@pytest.mark.parametrize("L,d", TABLE)
def test_all_match_and_all_mismatch_planes(probe, L, d):
    """Counts 0 and L in every window: the bias at both ends of its range.  With every validity bit set -- more than the
    tables ever set -- the entries still agree on all bit rows whose windows lie inside the capacity; what the
    extension words' bit row 31 holds decides the rest."""
    rng = np.random.default_rng(7 * L + d)
    r = _Runner(probe, L, d)
    inside, ginside = _cap_words(L), _cap_groups(L)
    ones = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    for kind in ("zeros", "ones", "random"):
        hi = {"zeros": np.zeros(W, np.uint32), "ones": ones.copy(),
              "random": rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)}[kind]
        lo = hi[::-1].copy()
        for match in (True, False):
            bhi, blo = (hi, lo) if match else (~hi, lo)
            for av in (inside, ones):
                p = np.ascontiguousarray(np.stack([hi, lo, av, bhi, blo]))
                a = p.ctypes.data
                ho, an = r(a, a + 4 * W, a + 8 * W, a + 12 * W, a + 16 * W)
                if av is inside:
                    assert (ho == an).all(), (kind, match)
                    want = np.array([np.bitwise_or.reduce(inside[g * GRP:(g + 1) * GRP]) for g in range(W // GRP)])
                    assert (an == (want if match else 0)).all(), (kind, match)   # L matches: a hit; L mismatches: none (d < L)
                else:
                    assert (((ho ^ an) & ginside) == 0).all(), (kind, match)


@pytest.mark.parametrize("L,d", TABLE)
def test_planes_built_by_the_tables_over_all_shifts(probe, L, d):
    rng = np.random.default_rng(31 * L + d)
    r = _Runner(probe, L, d)
    lens = (L, L + 4, 300, 600)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    seqs[2][40:140] = seqs[3][200:300]            # a shared stretch: dense hits along one diagonal
    seqs[3][500:560] = 0                          # poly-A
    seqs[2][250:] = 0
    planes = np.zeros(3 * W, dtype=np.uint32)
    flagged = 0
    for B in seqs:
        T = len(B)
        sb = [(np.zeros(T + W, np.uint32), np.zeros(T + W, np.uint32)) for _ in range(2)]
        for st in range(2):
            probe.bsprobe_sb_words(B.ctypes.data, T, st, W, L, T + W, sb[st][0].ctypes.data, sb[st][1].ctypes.data)
        for A in seqs:
            for s0 in range(0, len(A) - L + 1, _cap(L)):
                probe.bsprobe_row_planes(A.ctypes.data, len(A), s0, W, L, planes.ctypes.data)
                pa = planes.ctypes.data
                for st in range(2):
                    bh, bl = sb[st][0].ctypes.data, sb[st][1].ctypes.data
                    for delta in range(T):
                        ho, an = r(pa, pa + 4 * W, pa + 8 * W, bh + 4 * delta, bl + 4 * delta)
                        if ho[0] != an[0] or ho[1] != an[1]:
                            raise AssertionError((len(A), T, s0, st, delta, [hex(int(x)) for x in ho], [hex(int(x)) for x in an]))
                        flagged += 1 if (ho[0] | ho[1]) else 0
    assert flagged > 50
