"""Row validity per GROUP of five words in the same-length variant of the hot kernel.

window_group_any_grouped (gkm_bitslice.h) applies the OR of a group's five validity words to the OR of the group's five
top planes, where window_group_any spends one op per word.  What it delivers is a superset: a (bit row, group) is flagged
when some window of the five is within d mismatches and some window of the five is owned.  The same-length kernel's trip
evaluates every window of a pushed group itself and reads the row weight by position from a table with L - 1 zero bytes
behind the row's last l-mer, so the extra flags are harmless exactly if every window they bring in lies at a lane
position i with nB <= i < nB + 4 (nB: the windows the lane owns) in a group of which the lane owns a part.

CPU part, through bitslice_cpu_probe.so, for every (L, d) whose threshold is the top plane: the entry equals
(OR of the top planes) & AVg bit for bit, contains window_group_any's result, and its extra bits stay inside that bound --
on random planes with table-built validity and on table-built planes over every shift of both strands.

GPU part: integer mismatch profiles of same-length problems bit for bit against the CPU oracle, at the lengths where the
last group of a row is partial, on sparse (four-letter) and dense (two-letter) input, weighted and unweighted."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.test_group_any import TOP_PLANE, TABLE, W, GRP

NG = W // GRP
PAIRS = sorted(TOP_PLANE)


@pytest.fixture(scope="module")
def probe(built):
    lib = ctypes.CDLL(os.path.join(helpers.ROOT, "gkmqc_amd", "csrc", "bitslice_cpu_probe.so"))
    lib.bsprobe_group_any.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    lib.bsprobe_group_any_grouped.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    lib.bsprobe_row_planes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.bsprobe_sb_words.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    lib.bsprobe_piece_valid.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return lib


class _Both:
    """One shift through window_group_any and window_group_any_grouped on the same planes."""

    def __init__(self, probe, L, d):
        self.probe, self.L, self.d = probe, L, d
        self.hit_or, self.any = np.zeros(NG, np.uint32), np.zeros(NG, np.uint32)
        self.grouped, self.top_or, self.avg = np.zeros(NG, np.uint32), np.zeros(NG, np.uint32), np.zeros(NG, np.uint32)
        self.top = ctypes.c_int(-1)

    def __call__(self, ahi, alo, av, bhi, blo):
        p = self.probe
        assert p.bsprobe_group_any(self.L, self.d, ahi, alo, av, bhi, blo, self.hit_or.ctypes.data, self.any.ctypes.data,
                                   ctypes.addressof(self.top)) == 0
        assert p.bsprobe_group_any_grouped(self.L, self.d, ahi, alo, av, bhi, blo, self.grouped.ctypes.data,
                                           self.top_or.ctypes.data, self.avg.ctypes.data) == 0
        return self.any, self.grouped, self.top_or, self.avg


def _check(any_, grouped, top_or, avg, owned, what):
    """The three properties for one shift; `owned` = number of windows the lane owns (positions 0 .. owned - 1).
    Returns the number of extra (bit row, group) flags."""
    assert (grouped == (top_or & avg)).all(), what
    assert ((any_ & ~grouped) == 0).all(), what
    extra = 0
    for g in range(NG):
        x = int(grouped[g] & ~any_[g])
        while x:
            b = (x & -x).bit_length() - 1
            x &= x - 1
            first = b * W + g * GRP             # the group's five windows: lane positions first .. first + 4
            # the lane owns a part of the group, and the windows it does not own are positions owned .. owned + 3 at most
            assert first < owned <= first + GRP - 1, (what, g, b, owned)
            assert owned <= first + GRP - 1 < owned + 4, (what, g, b, owned)
            extra += 1
    return extra


def test_the_grouped_entry_exists_for_the_top_plane_pairs_only(probe):
    z = np.zeros(W, dtype=np.uint32)
    out = np.zeros(3 * NG, dtype=np.uint32)
    a, o = z.ctypes.data, out.ctypes.data
    for L, d in TABLE:
        rc = probe.bsprobe_group_any_grouped(L, d, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG)
        assert rc == (0 if (L, d) in TOP_PLANE else 2), (L, d)
    assert probe.bsprobe_group_any_grouped(4, 1, a, a, a, a, a, o, o + 4 * NG, o + 8 * NG) == 1
    assert {(11, 3), (10, 3), (12, 4)} <= TOP_PLANE


def _validity_pool(probe, L):
    """Validity planes as the tables build them for a lane that starts at lane position 0, with the number of windows
    each owns: rows of one segment (row_plane_word) and pieces over all 32 bit rows (piece_bit) -- whole lanes of the
    same-length packing (the capacity rounded down to a multiple of five) and lanes that finish their row anywhere."""
    cap5 = (32 * W - (L - 1)) // GRP * GRP
    pool = []
    planes = np.zeros(3 * W, dtype=np.uint32)
    codes = np.zeros(400, dtype=np.uint8)
    for n in (L, L + 1, L + 3, L + 4, L + 5, 200, 300, 302, 303, 304):
        probe.bsprobe_row_planes(codes.ctypes.data, n, 0, W, L, planes.ctypes.data)
        pool.append((planes[2 * W:].copy(), n - L + 1))
    pv = np.zeros(W, dtype=np.uint32)
    for cnt in (cap5, cap5 - 1, cap5 - 4, cap5 - 5, 1, 2, 4, 5, 6, 151, 152, 153, 154, 155):
        probe.bsprobe_piece_valid(0, 32, cnt, W, pv.ctypes.data)
        pool.append((pv.copy(), cnt))
    for av, cnt in pool:
        assert sum(bin(int(x)).count("1") for x in av) == cnt
    return pool


@pytest.mark.parametrize("L,d", PAIRS)
def test_random_planes_with_table_built_validity(probe, L, d):
    rng = np.random.default_rng(1000 * L + d)
    r = _Both(probe, L, d)
    pool = _validity_pool(probe, L)
    flagged = extra = 0
    for trial in range(2000):
        p = rng.integers(0, 1 << 32, (5, W), dtype=np.uint64).astype(np.uint32)
        if trial % 2:           # near-identical planes: many windows at and around the threshold
            noise = rng.integers(0, 1 << 32, (3, 2, W), dtype=np.uint64).astype(np.uint32)
            p[3] = p[0] ^ (noise[0, 0] & noise[1, 0] & noise[2, 0])
            p[4] = p[1] ^ (noise[0, 1] & noise[1, 1] & noise[2, 1])
        av, owned = pool[trial % len(pool)]
        p[2] = av
        p = np.ascontiguousarray(p)
        a = p.ctypes.data
        any_, grouped, top_or, avg = r(a, a + 4 * W, a + 8 * W, a + 12 * W, a + 16 * W)
        want_avg = np.array([np.bitwise_or.reduce(av[g * GRP:(g + 1) * GRP]) for g in range(NG)], dtype=np.uint32)
        assert (avg == want_avg).all()
        extra += _check(any_, grouped, top_or, avg, owned, (trial, owned))
        flagged += int(grouped.any())
    assert flagged > 100 and extra > 0      # the comparison saw hits, and windows past the end among them


@pytest.mark.parametrize("L,d", PAIRS)
def test_planes_built_by_the_tables_over_all_shifts(probe, L, d):
    """Same-length pairs (row and column of length T) from a two-letter alphabet -- dense hits, so that the windows
    behind the row's last l-mer are flagged too -- and from all four letters, every shift of both strands."""
    rng = np.random.default_rng(77 * L + d)
    r = _Both(probe, L, d)
    planes = np.zeros(3 * W, dtype=np.uint32)
    flagged = extra = 0
    for T in (L, L + 1, L + 4, 300, 302, 303, 304):
        for letters in (2, 4):
            A = (rng.integers(0, letters, T) * (3 if letters == 2 else 1)).astype(np.uint8)      # A/T: closed under rc
            B = (rng.integers(0, letters, T) * (3 if letters == 2 else 1)).astype(np.uint8)
            if T >= 300:
                B[40:90] = A[60:110]                  # a shared stretch: dense hits along one diagonal
            probe.bsprobe_row_planes(A.ctypes.data, T, 0, W, L, planes.ctypes.data)
            pa = planes.ctypes.data
            for st in range(2):
                bh, bl = np.zeros(T + W, np.uint32), np.zeros(T + W, np.uint32)
                probe.bsprobe_sb_words(B.ctypes.data, T, st, W, L, T + W, bh.ctypes.data, bl.ctypes.data)
                for delta in range(T):
                    any_, grouped, top_or, avg = r(pa, pa + 4 * W, pa + 8 * W, bh.ctypes.data + 4 * delta, bl.ctypes.data + 4 * delta)
                    extra += _check(any_, grouped, top_or, avg, T - L + 1, (T, letters, st, delta))
                    flagged += int(grouped.any())
    assert flagged > 50 and extra > 0


# ---------------------------------------------------------------------------------------------- GPU
from tests.test_gpu_parity import dev  # noqa: E402,F401  (the module-scoped device fixture)


def _n_seq(T):
    """Two row tiles of the same-length variant, the second one partial: 70 rows of one lane each (64 + 6), or 40 rows of
    two lanes each at 604 bp (32 + 8)."""
    return 70 if T <= 310 else 40


# (L, d): the three bench workloads' pairs (top plane: beta 0, 1, 0) and one pair that keeps the per-word path
GPU_PAIRS = [(11, 3), (10, 3), (12, 4), (9, 3)]
# T - L in {0, 3}: fewer than five l-mers; 300: the headline (q by mod_small); 302 .. 304: nB % 5 != 0; 604: rows over two
# whole lanes, the second one's count not a multiple of five.  The packer lets rows share lanes at 200 bp and at 640 bp (a
# third lane with a few windows), so those two -- like the short ones -- take the several-pieces variants, which keep
# per-word validity: they show that path unchanged.
GPU_LENGTHS = ["L", "L+3", 200, 300, 302, 303, 304, 604, 640]
SAME_LENGTH_VARIANT = (300, 302, 303, 304, 604)
GPU_CASES = [(L, d, T, 2 if (i + j) % 2 else 4) for i, (L, d) in enumerate(GPU_PAIRS) for j, T in enumerate(GPU_LENGTHS)]


def _problem(L, T, letters, seed):
    rng = np.random.default_rng(seed)
    seqs = [(rng.integers(0, letters, T) * (3 if letters == 2 else 1)).astype(np.uint8) for _ in range(_n_seq(T))]
    seqs[5] = seqs[9].copy()
    seqs[17] = (3 - seqs[20][::-1]).astype(np.uint8)          # reverse complement of another sequence
    return seqs


@pytest.mark.gpu
@pytest.mark.parametrize("L,d,T,letters", GPU_CASES)
def test_same_length_profiles_against_the_oracle(dev, L, d, T, letters):
    """Weighted (type 4) and unweighted (type 2) on the same sequences; half of the cases from a two-letter alphabet,
    where 5-15 % of all windows are hits and the groups behind a row's end are visited as a matter of course."""
    assert ((L, d) in TOP_PLANE) == ((L, d) != (9, 3))
    T = {"L": L, "L+3": L + 3}.get(T, T)
    seqs = _problem(L, T, letters, 1000 * L + 10 * d + T)
    il = np.tril_indices(len(seqs))
    for t in (4, 2):
        want = helpers.oracle_problem(seqs, (t, L, L - d, d, 50, 50.0, 1.0))["P"]
        res = dev.gram_matrix(seqs, t, L, L - d, d, want_profiles=True, kernel=dev.KERNEL_BITSLICE)
        if T in SAME_LENGTH_VARIANT:    # rows that fill whole lanes: the variant this file is about
            assert res["kernel"] == "k_gram_bitslice<same length>", res["kernel"]
        else:
            assert res["kernel"].startswith("k_gram_bitslice<packed"), res["kernel"]
        got = res["P"].cpu().numpy()
        assert (got[il] == want[il]).all(), (t, L, d, T, letters, res["kernel"])
        assert want[il].any()
