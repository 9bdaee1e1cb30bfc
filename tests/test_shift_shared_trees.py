"""window_group_any_centres with SHIFT-SHARED TREES (gkm_bitslice.h, SHIFTED = true; what k_gram_bitslice PK = 6, 7 run) against
its shared form (round 18's, the -DGKM_BS_CENTRES=2 build), its private form (-DGKM_BS_CENTRES=1) and window_group_any_grouped
(the stepped counter of the group-record kernels), bit for bit on all 32 bits of both groups.

The shift-shared form sums the five words S behind the first centre's heads once and hands the second centre the three planes of
that sum shifted one bit row on, in place of the five extension words Z[x] = Z[x - W] >> 1 that the shared form adds one by one; U,
the five words both centres end / begin with, is summed once as well.  A column sum is bitwise, so this is an identity on
arbitrary words, bit row 31 (where both read five mismatches) included.  Held for every (L, d) at which the form is compiled --
shift_shared_serves: the top-plane pairs with L = 10 or 11, read back from the probe -- on

  - random planes at match densities from iid (0.25) to dense (0.95) and independent random planes, with the validity words of
    tests/test_group_crossings.py;
  - the CONSTRUCTED words of tests/test_shared_trees.py: the centre window's biased count at 2^(P-1) - 2, 2^(P-1) - 1 and
    >= 2^(P-1) while the largest step M to an off-centre window is 0, 1 and 2; all nine cases in both groups wherever d >= 2
    allows them (the infeasible cells of d < 2 do not arise: the four pairs have d >= 2);
  - EDGE ROWS: match words whose bit rows 31 and 0 are the complement of their neighbours 30 and 1, whose bit row 31 or 0 alone is
    set or alone is clear, and single-row words for every row: a shift in the wrong direction moves row 1 into row 0 where row 31's
    neighbour belongs, and a top bit that is lost or wrapped round shows in row 31 or row 0 of the second group.

Every other top-plane pair stays on the shared form under SHIFTED = true (the constexpr predicate decides); that is held too."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.test_group_any import TOP_PLANE, W, GRP
from tests.test_group_centres import _restated, _window_counts
from tests.test_group_crossings import DENSITIES, _pair_at_density, _rand32, _validities, _words
from tests.test_shared_trees import ROWS, _constructed_shift, _feasible, _nine

NG = W // GRP
TAKEN = [(10, 2), (10, 3), (11, 3), (11, 4)]   # shift_shared_serves at W = 10: top-plane pairs with 0 <= L - W <= 1
OTHERS = sorted(TOP_PLANE - set(TAKEN))
TRIALS = 40


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any_shift_shared.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 10
    return lib


class _Forms:
    """One shift through the grouped entry and the three forms of the centres entry on the same planes."""

    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.out = np.zeros((4, NG), dtype=np.uint32)
        self.taken = ctypes.c_int(-1)

    def __call__(self, ahi, alo, avg, bhi, blo):
        """five uint32 arrays (W, W, NG, W, W words) -> (grouped, shift-shared, shared, private)"""
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (ahi, alo, avg, bhi, blo)]
        assert [len(x) for x in arrs] == [W, W, NG, W, W]
        o = self.out.ctypes.data
        self.out[:] = 0xDEADBEEF
        rc = self.probe.bsprobe_group_any_shift_shared(self.L, self.d, *[x.ctypes.data for x in arrs],
                                                       *[o + 4 * NG * i for i in range(4)], ctypes.addressof(self.taken))
        assert rc == 0, (self.L, self.d)
        return tuple(self.out[i].copy() for i in range(4))

    def equal(self, ahi, alo, avg, bhi, blo, counts=None):
        g, h, s, p = self(ahi, alo, avg, bhi, blo)
        assert (h == s).all() and (h == p).all() and (h == g).all(), (self.L, self.d, avg, g, h, s, p)
        if counts is not None:
            assert (h == _restated(self.L, self.d, counts, avg)).all(), (self.L, self.d, avg, h)
        return h


def _from_match(rng, match):
    """row and column planes whose match bits are exactly `match` (a mismatch flips hi, or lo where kind is clear)"""
    ahi, alo, kind = _rand32(rng, W), _rand32(rng, W), _rand32(rng, W)
    mm = ~match
    return ahi, alo, ahi ^ (mm & kind), alo ^ (mm & ~kind)


def test_the_form_is_compiled_for_the_pairs_listed(probe):
    z = np.zeros(W, dtype=np.uint32)
    assert set(TAKEN) <= TOP_PLANE and len(TOP_PLANE) == 15
    for L, d in sorted(TOP_PLANE):
        r = _Forms(probe, L, d)
        r(z, z, z[:NG], z, z)
        assert r.taken.value == (1 if (L, d) in TAKEN else 0), (L, d)
    out = np.zeros(4 * NG, dtype=np.uint32)
    a, o, t = z.ctypes.data, out.ctypes.data, ctypes.c_int(0)
    tail = [o, o + 4 * NG, o + 8 * NG, o + 12 * NG, ctypes.addressof(t)]
    assert probe.bsprobe_group_any_shift_shared(11, 2, a, a, a, a, a, *tail) == 2
    assert probe.bsprobe_group_any_shift_shared(4, 1, a, a, a, a, a, *tail) == 1


@pytest.mark.parametrize("L,d", TAKEN)
def test_four_forms_equal_on_random_words(probe, L, d):
    rng = np.random.default_rng(20000 * L + d)
    r = _Forms(probe, L, d)
    flagged = np.zeros(NG, dtype=np.int64)
    planes = []
    for p in DENSITIES:
        planes += [_pair_at_density(rng, p) for _ in range(TRIALS)]
    for _ in range(TRIALS):
        planes.append(tuple(_rand32(rng, W) for _ in range(4)))
        planes.append((_rand32(rng, W), _words(rng, W, 0.9), _words(rng, W, 0.05), _rand32(rng, W)))
    for i, (ahi, alo, bhi, blo) in enumerate(planes):
        counts = _window_counts(L, ahi, alo, bhi, blo) if i % 5 == 0 else None
        for avg in _validities(rng):
            flagged += (r.equal(ahi, alo, avg, bhi, blo, counts) != 0)
    assert r.taken.value == 1
    assert (flagged > 100).all(), flagged


@pytest.mark.parametrize("L,d", TAKEN)
def test_four_forms_equal_on_the_nine_threshold_cases(probe, L, d):
    rng = np.random.default_rng(21000 * L + d)
    r = _Forms(probe, L, d)
    seen = np.zeros((3, 3, NG), dtype=np.int64)
    rows = np.array(list(ROWS))
    for shift in range(60):
        ahi, alo, bhi, blo = _constructed_shift(rng, L, d)
        counts = _window_counts(L, ahi, alo, bhi, blo)
        seen += _nine(L, d, counts[:, rows])
        for avg in _validities(rng)[:3]:
            r.equal(ahi, alo, avg, bhi, blo, counts)
    print(L, d, seen.tolist())
    assert d >= 2 and all(_feasible(L, d, below, m) for below in range(3) for m in range(3))
    assert (seen > 0).all(), seen   # all nine, in both groups


def _edge_row_matches(rng):
    """match words (W of them per case) whose bit rows 31 and 0 stand apart from their neighbours"""
    top, bot = np.uint32(1 << 31), np.uint32(1)
    ones, zero = np.full(W, 0xFFFFFFFF, np.uint32), np.zeros(W, np.uint32)
    cases = [ones & ~top, ones & ~bot, ones & ~(top | bot), zero | top, zero | bot, zero | top | bot, ones, zero]
    for b in range(32):     # one row set in every word, and one row clear: where it lands after the shift is all there is
        cases += [np.full(W, 1 << b, np.uint32), np.full(W, 0xFFFFFFFF ^ (1 << b), np.uint32)]
    for p in DENSITIES + (0.6, 0.75, 0.85):
        for _ in range(12):
            m = _words(rng, W, p)
            # row 31 := ~row 30, row 0 := ~row 1
            m = (m & np.uint32(0x7FFFFFFE)) | ((~m << np.uint32(1)) & top) | ((~m >> np.uint32(1)) & bot)
            cases.append(m.astype(np.uint32))
            # only the edge rows vary: a dense or empty body with random rows 0 and 31
            body = np.uint32(0x7FFFFFFE) if rng.random() < 0.7 else np.uint32(0)
            cases.append((body | (_rand32(rng, W) & (top | bot))).astype(np.uint32))
    return cases


@pytest.mark.parametrize("L,d", TAKEN)
def test_four_forms_equal_on_edge_rows(probe, L, d):
    rng = np.random.default_rng(22000 * L + d)
    r = _Forms(probe, L, d)
    edge = np.uint32(0x80000001)
    vals = [np.full(NG, 0xFFFFFFFF, np.uint32), np.full(NG, edge, np.uint32), np.array([0x80000000, 1], np.uint32)]
    differ = np.zeros((2, NG), dtype=np.int64)   # [row 0 / row 31, group]: the edge row's flag differs from its neighbour's
    for match in _edge_row_matches(rng):
        ahi, alo, bhi, blo = _from_match(rng, match)
        assert ((~((ahi ^ bhi) | (alo ^ blo))) == match).all()
        counts = _window_counts(L, ahi, alo, bhi, blo)
        for avg in vals:
            h = r.equal(ahi, alo, avg, bhi, blo, counts)
            if avg is vals[0]:
                differ[0] += ((h ^ (h >> np.uint32(1))) & np.uint32(1)) != 0
                differ[1] += (((h >> np.uint32(31)) ^ (h >> np.uint32(30))) & np.uint32(1)) != 0
    # the inputs do what they are for: in both groups the edge rows' answers differ from their neighbours' many times
    assert (differ >= 20).all(), differ


@pytest.mark.parametrize("L,d", OTHERS)
def test_other_pairs_stay_on_the_shared_form(probe, L, d):
    rng = np.random.default_rng(23000 * L + d)
    r = _Forms(probe, L, d)
    for p in DENSITIES:
        for _ in range(6):
            ahi, alo, bhi, blo = _pair_at_density(rng, p)
            for avg in _validities(rng)[:3]:
                r.equal(ahi, alo, avg, bhi, blo)
    assert r.taken.value == 0
