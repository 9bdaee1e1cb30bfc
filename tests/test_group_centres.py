"""window_group_any_centres (gkm_bitslice.h) -- the counting loop of the shift-record kernels -- against
window_group_any_grouped, which the group-record kernels keep and tests/test_group_validity.py pins, and against a numpy
restatement that passes through no counter at all.

The centres form steps nothing: per group of five words it sums the CENTRE window exactly (the adder tree) and asks whether
the largest of the five counts reaches the top plane: B[C] + M with M = max(0, e1, e1 + e2, f1, f1 + f2) in {0, 1, 2}, e / f the
two steps up / down from the centre.  That is a Boolean identity on arbitrary words, so it must agree with the stepped counter
on ALL 32 bits of both groups, whatever the planes and whatever the validity words.  Held here for every (L, d) whose
threshold is the top plane (the 15 pairs of tests/test_group_any.TOP_PLANE), with the plane and validity generators of
tests/test_group_crossings.py: match densities from iid (0.25) to dense (0.95), independent random planes, constant planes;
validity words all ones, all zero, random and sparse.

Second route: Z with its `>> 1` extension words, the per-window sums, the threshold `>= L - d`, the OR per group and the AND
with AVg, all in numpy integers.  The same restatement counts the cases that are specific to this form -- the centre window
exactly ONE and exactly TWO below the threshold while the group is flagged only through an off-centre window, on the up side
and on the down side, in both groups -- and every pair must have met each of them."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.test_group_any import TOP_PLANE, TABLE, W, GRP
from tests.test_group_crossings import DENSITIES, _pair_at_density, _rand32, _validities, _words

NG = W // GRP
PAIRS = sorted(TOP_PLANE)
TRIALS = 150


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any_centres.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 7
    return lib


class _Two:
    """One shift through the grouped entry and the centres entry on the same planes."""

    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.out = np.zeros((2, NG), dtype=np.uint32)

    def __call__(self, ahi, alo, avg, bhi, blo):
        """five uint32 arrays (W, W, NG, W, W words) -> (grouped, centres)"""
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (ahi, alo, avg, bhi, blo)]
        assert [len(x) for x in arrs] == [W, W, NG, W, W]
        o = self.out.ctypes.data
        self.out[:] = 0xDEADBEEF
        rc = self.probe.bsprobe_group_any_centres(self.L, self.d, *[x.ctypes.data for x in arrs], o, o + 4 * NG)
        assert rc == 0, (self.L, self.d)
        return self.out[0].copy(), self.out[1].copy()


def _window_counts(L, ahi, alo, bhi, blo):
    """counts[w, b]: matching bases of the window at word w, bit row b, as gkm_bitslice.h lays a shift out: word x >= W is
    word x - W one bit row up, with a mismatch entering bit row 31.  No counter, no bit-slicing: integers."""
    mism = (ahi ^ bhi) | (alo ^ blo)
    z = ((~mism)[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)        # (W, 32) match bits
    zz = np.zeros((W + L - 1, 32), dtype=np.int64)
    zz[:W] = z
    for x in range(W, W + L - 1):                                                   # (at L = 12 word 2 W is word 0 two rows up)
        zz[x, :31] = zz[x - W, 1:]
    return np.stack([zz[w:w + L].sum(axis=0) for w in range(W)])                    # (W, 32)


def _pack(bits):
    return int((bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum())


def _restated(L, d, counts, avg):
    hit = counts >= L - d
    return np.array([_pack(hit[g * GRP:(g + 1) * GRP].any(axis=0)) & int(avg[g]) for g in range(NG)], dtype=np.uint32)


def _off_centre_cases(L, d, counts):
    """-> int array [below, side, group], below = 0 / 1: the centre window exactly one / two under the threshold; side = 0
    (up: words C + 1, C + 2) / 1 (down: C - 1, C - 2): bit rows whose group is flagged through that side alone"""
    thr = L - d
    hit = counts >= thr
    out = np.zeros((2, 2, NG), dtype=np.int64)
    for g in range(NG):
        c = g * GRP + GRP // 2
        up, dn = hit[c + 1:c + 3].any(axis=0), hit[c - 2:c].any(axis=0)
        for below in (0, 1):
            centre = counts[c] == thr - 1 - below
            out[below, 0, g] = (centre & up & ~dn).sum()
            out[below, 1, g] = (centre & dn & ~up).sum()
    return out


def test_the_centres_entry_exists_for_the_top_plane_pairs_only(probe):
    z = np.zeros(W, dtype=np.uint32)
    out = np.zeros(2 * NG, dtype=np.uint32)
    a, o = z.ctypes.data, out.ctypes.data
    for L, d in TABLE:
        rc = probe.bsprobe_group_any_centres(L, d, a, a, a, a, a, o, o + 4 * NG)
        assert rc == (0 if (L, d) in TOP_PLANE else 2), (L, d)
    assert probe.bsprobe_group_any_centres(4, 1, a, a, a, a, a, o, o + 4 * NG) == 1
    assert probe.bsprobe_group_any_centres(3, 0, a, a, a, a, a, o, o + 4 * NG) == 1
    assert len(PAIRS) == 15 and {(5, 1), (5, 2), (6, 3), (8, 0), (10, 3), (11, 3), (12, 4), (12, 5)} <= TOP_PLANE


@pytest.mark.parametrize("L,d", PAIRS)
def test_equal_on_every_bit_from_iid_to_dense(probe, L, d):
    rng = np.random.default_rng(6000 * L + d)
    r = _Two(probe, L, d)
    flagged = np.zeros(NG, dtype=np.int64)
    cases = np.zeros((2, 2, NG), dtype=np.int64)
    full = 0
    for p in DENSITIES:
        for trial in range(TRIALS):
            ahi, alo, bhi, blo = _pair_at_density(rng, p)
            restate = trial % 3 == 0       # the second route on every third shift
            counts = _window_counts(L, ahi, alo, bhi, blo)
            cases += _off_centre_cases(L, d, counts)
            for avg in _validities(rng):
                g, c = r(ahi, alo, avg, bhi, blo)
                assert (g == c).all(), (L, d, p, trial, avg, g, c)
                if restate:
                    assert (c == _restated(L, d, counts, avg)).all(), (L, d, p, trial, avg, c)
                flagged += (g != 0)
                full += int((g == avg).all() and avg.all())
    # the comparison saw hits in both groups, and shifts where every valid bit row of both groups is flagged
    assert (flagged > 100).all() and full > 0, (flagged, full)
    # ... and what only this form has: a centre one / two below the threshold, the group flagged from one side alone
    assert (cases > 0).all(), cases


@pytest.mark.parametrize("L,d", PAIRS)
def test_equal_on_arbitrary_planes(probe, L, d):
    """Independent random planes (no relation between row and column), and the constant ones: all bases equal on both
    sides (every window matches everywhere), all bases different (none does), and each plane constant on its own."""
    rng = np.random.default_rng(7000 * L + d)
    r = _Two(probe, L, d)
    ones, zero = np.full(W, 0xFFFFFFFF, np.uint32), np.zeros(W, np.uint32)
    cases = [(zero, zero, zero, zero), (ones, ones, ones, ones), (ones, ones, zero, zero), (zero, ones, ones, zero),
             (ones, zero, ones, ones), (zero, zero, zero, ones)]
    for trial in range(300):
        cases.append(tuple(_rand32(rng, W) for _ in range(4)))
        cases.append((_rand32(rng, W), _words(rng, W, 0.9), _words(rng, W, 0.05), _rand32(rng, W)))
    seen = 0
    for i, (ahi, alo, bhi, blo) in enumerate(cases):
        counts = _window_counts(L, ahi, alo, bhi, blo) if i % 4 == 0 or i < 6 else None
        for avg in _validities(rng):
            g, c = r(ahi, alo, avg, bhi, blo)
            assert (g == c).all(), (L, d, ahi, alo, bhi, blo, avg)
            if counts is not None:
                assert (c == _restated(L, d, counts, avg)).all(), (L, d, ahi, alo, bhi, blo, avg)
            seen += int(g.any())
    # identical planes: every window is a full match; bit row 31 of the words whose window reaches the extension words
    # sees the fiction's mismatches there, so only the windows before them are certain -- group 0's word 0 at least
    avg = np.full(NG, 0xFFFFFFFF, np.uint32)
    _, c = r(ones, zero, avg, ones, zero)
    assert (c & 0x7FFFFFFF == 0x7FFFFFFF).all()
    _, c = r(ones, ones, avg, zero, zero)
    assert d < L and not c.any()       # nothing matches: no window is within d mismatches
    assert seen > 10
