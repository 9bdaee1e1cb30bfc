"""window_group_any_centres with SHARED TREES (gkm_bitslice.h; what k_gram_bitslice PK = 6, 7 run) against
window_group_any_grouped (the stepped counter of the group-record kernels) and against its own private-trees form (SHARED =
false, the -DGKM_BS_CENTRES=1 build), bit for bit on all 32 bits of both groups.

The shared form folds the words that the two centre windows have in common once (floor((L - 5) / 3) full adders; a bias of one
rides in the overlap's leftover words where there are any) and, where the column of plane P-2 holds exactly two planes p and q,
never forms the two top planes: b[P-1] | (b[P-2] & y) = maj(p, q, y).  Both are identities on arbitrary words, so the three
functions must agree whatever the planes and the validity words.  Held for every (L, d) whose threshold is the top plane (the
15 pairs of tests/test_group_any.TOP_PLANE; all have L >= 5):

  - random planes at match densities from iid (0.25) to dense (0.95) and independent random planes, with the validity words of
    tests/test_group_crossings.py;
  - CONSTRUCTED words that put the centre window's biased count B[C] at 2^(P-1) - 2, at 2^(P-1) - 1 and at 2^(P-1) or above
    (L - d - 2, L - d - 1, L - d matches) while the largest step M to an off-centre window of the group is 0, 1 and 2: the nine
    combinations the threshold distinguishes -- the fold rewrites exactly the term that tells them apart.  The combinations are
    counted from integer window sums (tests/test_group_centres._window_counts: no bit-slicing) and all nine must have
    occurred in both groups.  M = m needs m words of the centre window to leave as mismatches, so a window with B[C] matches
    can only have M <= L - B[C]: at d = 0 (>=, 1), (>=, 2) and (-1, 2) cannot exist, at d = 1 (>=, 2) cannot; those cells are
    asserted empty and every other one non-empty.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.test_group_any import TOP_PLANE, W, GRP
from tests.test_group_centres import _restated, _window_counts
from tests.test_group_crossings import DENSITIES, _pair_at_density, _rand32, _validities, _words

NG = W // GRP
PAIRS = sorted(TOP_PLANE)
TRIALS = 40
ROWS = range(0, 32, 3)   # bit rows that carry a constructed segment: W + L - 1 <= 21 words each, 30 apart


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any_centres_forms.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    return lib


class _Forms:
    """One shift through the grouped entry and both forms of the centres entry on the same planes."""

    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.out = np.zeros((3, NG), dtype=np.uint32)

    def __call__(self, ahi, alo, avg, bhi, blo):
        """five uint32 arrays (W, W, NG, W, W words) -> (grouped, shared trees, private trees)"""
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (ahi, alo, avg, bhi, blo)]
        assert [len(x) for x in arrs] == [W, W, NG, W, W]
        o = self.out.ctypes.data
        self.out[:] = 0xDEADBEEF
        rc = self.probe.bsprobe_group_any_centres_forms(self.L, self.d, *[x.ctypes.data for x in arrs], o, o + 4 * NG, o + 8 * NG)
        assert rc == 0, (self.L, self.d)
        return self.out[0].copy(), self.out[1].copy(), self.out[2].copy()


def test_every_top_plane_pair_is_covered(probe):
    assert len(PAIRS) == 15 and min(L for L, _ in PAIRS) >= 5
    assert {(5, 1), (5, 2), (6, 2), (7, 3), (8, 1), (9, 2), (10, 3), (11, 3), (12, 4), (12, 5)} <= TOP_PLANE
    z = np.zeros(W, dtype=np.uint32)
    out = np.zeros(3 * NG, dtype=np.uint32)
    a, o = z.ctypes.data, out.ctypes.data
    for L, d in PAIRS:
        assert probe.bsprobe_group_any_centres_forms(L, d, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG) == 0, (L, d)
    assert probe.bsprobe_group_any_centres_forms(11, 2, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG) == 2
    assert probe.bsprobe_group_any_centres_forms(4, 1, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG) == 1


@pytest.mark.parametrize("L,d", PAIRS)
def test_three_forms_equal_on_random_words(probe, L, d):
    rng = np.random.default_rng(8000 * L + d)
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
            g, s, p = r(ahi, alo, avg, bhi, blo)
            assert (g == s).all() and (p == s).all(), (L, d, i, avg, g, s, p)
            if counts is not None:
                assert (s == _restated(L, d, counts, avg)).all(), (L, d, i, avg, s)
            flagged += (g != 0)
    assert (flagged > 100).all(), flagged


def _feasible(L, d, below, m):
    """can a centre window with L - d - below matches have a largest step of m?  m of its words must leave as mismatches"""
    return d + below >= m


def _constructed_shift(rng, L, d):
    """-> planes of one shift whose bit rows ROWS each hold one constructed segment: group g's centre window with L - d - below
    matches, and the four words beside it set so that the largest step is exactly m, on the up or on the down side"""
    z = (rng.random(32 * W + 2 * W) < 0.5).astype(np.uint8)          # linear: base b * W + w is bit row b of word w
    for b in ROWS:
        g, below, m = int(rng.integers(0, NG)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
        if not _feasible(L, d, below, m):
            continue
        c0 = b * W + g * GRP + GRP // 2                               # the centre window: z[c0 .. c0 + L - 1]
        win = np.zeros(L, dtype=np.uint8)
        up = bool(rng.integers(0, 2))
        leaving = list(range(m)) if up else list(range(L - m, L))     # the words that leave on the way to the largest count
        free = [i for i in range(L) if i not in leaving]
        win[rng.choice(free, L - d - below, replace=False)] = 1
        z[c0:c0 + L] = win
        z[c0 - 2:c0] = 0
        z[c0 + L:c0 + L + 2] = 0
        if up:
            z[c0 + L:c0 + L + m] = 1
        elif m:
            z[c0 - m:c0] = 1
    zw = z[:32 * W].reshape(32, W).T.astype(np.uint64)                # (W, 32): match bits of word w
    match = (zw << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    ahi, alo = _rand32(rng, W), _rand32(rng, W)
    kind = _rand32(rng, W)                                            # a mismatch flips hi, or lo where kind is clear
    mm = ~match
    return ahi, alo, ahi ^ (mm & kind), alo ^ (mm & ~kind)


def _nine(L, d, counts):
    """-> int array [below, m, group]: bit rows whose centre window has L - d - below matches (below = 0: or more) and whose
    group's largest count lies m above the centre's (m = 0, 1, 2), from the integer window sums"""
    thr = L - d
    out = np.zeros((3, 3, NG), dtype=np.int64)
    for g in range(NG):
        c = g * GRP + GRP // 2
        m = counts[c - 2:c + 3].max(axis=0) - counts[c]
        assert m.min() >= 0 and m.max() <= 2
        for below in range(3):
            centre = counts[c] >= thr if below == 0 else counts[c] == thr - below
            for k in range(3):
                out[below, k, g] = (centre & (m == k)).sum()
    return out


@pytest.mark.parametrize("L,d", PAIRS)
def test_three_forms_equal_on_the_nine_threshold_cases(probe, L, d):
    rng = np.random.default_rng(9000 * L + d)
    r = _Forms(probe, L, d)
    seen = np.zeros((3, 3, NG), dtype=np.int64)
    rows = np.array(list(ROWS))
    for shift in range(60):
        ahi, alo, bhi, blo = _constructed_shift(rng, L, d)
        counts = _window_counts(L, ahi, alo, bhi, blo)
        seen += _nine(L, d, counts[:, rows])
        for avg in _validities(rng)[:3]:
            g, s, p = r(ahi, alo, avg, bhi, blo)
            assert (g == s).all() and (p == s).all(), (L, d, shift, avg, g, s, p)
            assert (s == _restated(L, d, counts, avg)).all(), (L, d, shift, avg, s)
    print(L, d, seen.tolist())
    for below in range(3):
        for m in range(3):
            if _feasible(L, d, below, m):
                assert (seen[below, m] > 0).all(), (L, d, below, m, seen)
            else:
                assert (seen[below, m] == 0).all(), (L, d, below, m, seen)
    # d >= 2, the shapes the kernels run most (10,3), (11,3), (12,4) among them: all nine, in both groups
    assert d < 2 or (seen > 0).all(), seen
