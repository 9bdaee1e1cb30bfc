"""window_group_any_crossings (gkm_bitslice.h) -- the counting loop of the shift-record kernels -- against
window_group_any_grouped, which the group-record kernels keep and tests/test_group_validity.py pins.

The crossings form never steps the top count plane: over a run of consecutive words the OR of the top planes is the top
plane of the run's first word ORed with the carries/borrows into it inside the run (b[w+1] = b[w] ^ t[w+1]: if a t fires,
b is set on one of its two sides).  That is a Boolean identity on arbitrary words, so the two functions must agree on ALL 32
bits of both groups, whatever the planes and whatever the validity words -- not only on bits a table-built validity lets
through.  Held here for every (L, d) whose threshold is the top plane, for both forms of the function: from the middle
(what the kernel runs: adder tree at word 5, one chain up, one down) and one direction (tree at word 0).

Planes: row and column planes whose per-base match density runs from iid (0.25) to dense (0.95) -- dense input makes the
top plane cross up and down inside one group and carries a set top plane over the group boundary --, independent random
planes, all-zero and all-one planes; validity words random, all ones, all zero and sparse."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.test_group_any import TOP_PLANE, TABLE, W, GRP

NG = W // GRP
PAIRS = sorted(TOP_PLANE)
DENSITIES = (0.25, 0.4, 0.55, 0.7, 0.8, 0.9, 0.95)


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any_crossings.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    return lib


class _Three:
    """One shift through the grouped entry and both forms of the crossings entry on the same planes."""

    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.out = np.zeros((3, NG), dtype=np.uint32)

    def __call__(self, ahi, alo, avg, bhi, blo):
        """five uint32 arrays (W, W, NG, W, W words) -> (grouped, from the middle, one direction)"""
        arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (ahi, alo, avg, bhi, blo)]
        assert [len(x) for x in arrs] == [W, W, NG, W, W]
        o = self.out.ctypes.data
        self.out[:] = 0xDEADBEEF
        rc = self.probe.bsprobe_group_any_crossings(self.L, self.d, *[x.ctypes.data for x in arrs], o, o + 4 * NG, o + 8 * NG)
        assert rc == 0, (self.L, self.d)
        return self.out[0].copy(), self.out[1].copy(), self.out[2].copy()


def _words(rng, n, density):
    """n words whose bits are set with the given probability"""
    bits = rng.random((n, 32)) < density
    return (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def _rand32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _pair_at_density(rng, p):
    """Row planes and column planes whose bases match with probability p: the column is the row with a mismatch (another
    of the three other bases, so one or both code bits flipped) at 1 - p of the positions."""
    ahi, alo = _rand32(rng, W), _rand32(rng, W)
    mm = _words(rng, W, 1.0 - p)
    kind = rng.integers(0, 3, (W, 32))       # 0: hi flips, 1: lo flips, 2: both
    sh = np.arange(32, dtype=np.uint64)
    fh = ((kind != 1).astype(np.uint64) << sh).sum(axis=1).astype(np.uint32) & mm
    fl = ((kind != 0).astype(np.uint64) << sh).sum(axis=1).astype(np.uint32) & mm
    return ahi, alo, ahi ^ fh, alo ^ fl


def _validities(rng):
    ones, zero = np.full(NG, 0xFFFFFFFF, np.uint32), np.zeros(NG, np.uint32)
    return [ones, zero, _rand32(rng, NG), _words(rng, NG, 0.1), np.array([0xFFFFFFFF, 0], np.uint32),
            np.array([0x3FFFFFFF, 0xC0000000], np.uint32)]


def test_the_crossings_entry_exists_for_the_top_plane_pairs_only(probe):
    z = np.zeros(W, dtype=np.uint32)
    out = np.zeros(3 * NG, dtype=np.uint32)
    a, o = z.ctypes.data, out.ctypes.data
    for L, d in TABLE:
        rc = probe.bsprobe_group_any_crossings(L, d, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG)
        assert rc == (0 if (L, d) in TOP_PLANE else 2), (L, d)
    assert probe.bsprobe_group_any_crossings(4, 1, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG) == 1
    assert len(PAIRS) == 15 and {(5, 1), (8, 0), (10, 3), (11, 3), (12, 4), (12, 5)} <= TOP_PLANE


@pytest.mark.parametrize("L,d", PAIRS)
def test_equal_on_every_bit_from_iid_to_dense(probe, L, d):
    rng = np.random.default_rng(4000 * L + d)
    r = _Three(probe, L, d)
    flagged = np.zeros(NG, dtype=np.int64)
    full = 0
    for p in DENSITIES:
        for trial in range(150):
            ahi, alo, bhi, blo = _pair_at_density(rng, p)
            for avg in _validities(rng):
                g, mid, one = r(ahi, alo, avg, bhi, blo)
                assert (g == mid).all() and (g == one).all(), (L, d, p, trial, avg, g, mid, one)
                flagged += (g != 0)
                full += int((g == avg).all() and avg.all())
    # the comparison saw hits in both groups, and shifts where every valid bit row of both groups is flagged
    assert (flagged > 100).all() and full > 0, (flagged, full)


@pytest.mark.parametrize("L,d", PAIRS)
def test_equal_on_arbitrary_planes(probe, L, d):
    """Independent random planes (no relation between row and column), and the constant ones: all bases equal on both
    sides (every window matches everywhere), all bases different (none does), and each plane constant on its own."""
    rng = np.random.default_rng(5000 * L + d)
    r = _Three(probe, L, d)
    ones, zero = np.full(W, 0xFFFFFFFF, np.uint32), np.zeros(W, np.uint32)
    cases = [(zero, zero, zero, zero), (ones, ones, ones, ones), (ones, ones, zero, zero), (zero, ones, ones, zero),
             (ones, zero, ones, ones), (zero, zero, zero, ones)]
    for trial in range(300):
        cases.append(tuple(_rand32(rng, W) for _ in range(4)))
        cases.append((_rand32(rng, W), _words(rng, W, 0.9), _words(rng, W, 0.05), _rand32(rng, W)))
    seen = 0
    for ahi, alo, bhi, blo in cases:
        for avg in _validities(rng):
            g, mid, one = r(ahi, alo, avg, bhi, blo)
            assert (g == mid).all() and (g == one).all(), (L, d, ahi, alo, bhi, blo, avg)
            seen += int(g.any())
    # identical planes: every window is a full match; bit row 31 of the words whose window reaches the extension words
    # sees the fiction's mismatches there, so only the windows before them are certain -- group 0's word 0 at least
    avg = np.full(NG, 0xFFFFFFFF, np.uint32)
    g, _, _ = r(ones, zero, avg, ones, zero)
    assert (g & 0x7FFFFFFF == 0x7FFFFFFF).all()
    g, _, _ = r(ones, ones, avg, zero, zero)
    assert d < L and not g.any()       # nothing matches: no window is within d mismatches
    assert seen > 10
