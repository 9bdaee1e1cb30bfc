"""Regions of a scan on the GPU at product level (gkmpredict.scan_regions, scan_regions_with_panel and their command line;
DESIGN.md §5o).  The whole contract is one sentence: whatever the threshold, the gap, the chunking and what precedes a
record, the result is tests/regions_ref.py applied to `scan`'s own output, bit for bit.

The inputs are test_scan_gpu.py's locus (the golden positives and negatives back to back, 6 000 bases) and C-SVC tables
of types 0 and 4 trained on the golden files.  The thresholds come from `scan`'s output of the case: three quantile
thresholds ("low", "high" and "equal", the last an order statistic and so exactly some window's score), the minimum, the
maximum and the next double above the maximum.

Every case of the three quantile thresholds asserts on the reference side that it holds at least 10 regions and one of
more than one window.  The locus is bimodal -- its first half scores high, its second low -- so the median falls
between the two modes and leaves 1 to 7 regions; the quantiles are therefore chosen per gap (QUANTILES below).  At gaps
0 and 3 they are 0.3, 0.9 and 0.8 for every table and shape (11 to 56 regions).  A gap of 50 windows merges
neighbouring regions by design, so there the quantiles are chosen per table and shape from the region counts of the
grid 0.02, 0.03 .. 0.99 on `scan`'s scores: 10 to 15 regions on both stride-1 shapes (for type 0 at W = 600 only the
quantiles 0.22 .. 0.31 reach 10, so all three thresholds lie there).  At stride 7 and gap 50 the issue's own
parameters cannot give 10 regions: two regions lie at least 52 windows apart from first window to first window, the
locus has 843 windows, and its positives are 200 bases = 29 windows long, so neighbouring peaks always merge; over the
whole grid the most regions any threshold leaves is 5 (type 0) and 4 (type 4).  Those cases take the quantiles that
reach that and assert at least 4 regions.  The `min`, `max` and `above` cases cannot meet the condition by
construction -- everything in one region, only the windows that hold the maximum, nothing -- and assert exactly that."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import regions_ref as RR

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")
SHAPES = ((100, 1), (100, 7), (600, 1))
GAPS = (0, 3, 50)
THRESHOLDS = ("low", "high", "min", "max", "above", "equal")
# the quantiles of the low, high and equal thresholds per (gap, type, width, stride); None: every table and shape
QUANTILES = {(0, None): (0.3, 0.9, 0.8), (3, None): (0.3, 0.9, 0.8),
             (50, 0, 100, 1): (0.34, 0.83, 0.71), (50, 4, 100, 1): (0.23, 0.76, 0.77),
             (50, 0, 600, 1): (0.25, 0.27, 0.24), (50, 4, 600, 1): (0.28, 0.89, 0.27),
             (50, 0, 100, 7): (0.46, 0.95, 0.47), (50, 4, 100, 7): (0.45, 0.97, 0.44)}


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


@pytest.fixture(scope="module")
def locus(dv):
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    return np.concatenate([pos[i] for i in range(15)] + [neg[i] for i in range(15)])


@pytest.fixture(scope="module")
def tables(gp):
    return {t: gp.lmer_weights(gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3)) for t in (0, 4)}


@pytest.fixture(scope="module")
def scanned(gp, tables, locus):
    """`scan`'s scores of the locus per (type, width, stride): computed once, the yardstick's only input"""
    cache = {}

    def get(t, W, s):
        if (t, W, s) not in cache:
            cache[t, W, s] = gp.scan(tables[t], [locus], W, s)[0][2]
            cache[t, W, s].setflags(write=False)
        return cache[t, W, s]
    return get


def _threshold(kind, scores, quantiles=QUANTILES[0, None]):
    if kind == "low":
        return float(np.quantile(scores, quantiles[0]))
    if kind == "high":
        return float(np.quantile(scores, quantiles[1]))
    if kind == "min":
        return float(scores.min())
    if kind == "max":
        return float(scores.max())
    if kind == "above":
        return float(np.nextafter(scores.max(), np.inf))
    return float(np.sort(scores)[int(quantiles[2] * len(scores))])         # exactly some window's score


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("kind", THRESHOLDS)
@pytest.mark.parametrize("W,s", SHAPES)
@pytest.mark.parametrize("t", [0, 4])
def test_every_threshold_gap_and_chunk(gp, tables, locus, scanned, t, W, s, kind, gap):
    scores = scanned(t, W, s)
    thr = _threshold(kind, scores, QUANTILES.get((gap, None)) or QUANTILES[gap, t, W, s])
    want = RR.regions(scores, W, s, thr, gap)
    n = len(want["start"])
    if kind in ("low", "high", "equal"):
        assert (want["windows"] > 1).any() and n >= (4 if (s, gap) == (7, 50) else 10), n
    if kind == "equal":
        assert (scores == thr).any()
    if kind == "min":
        assert n == 1 and want["windows"].sum() == len(scores)
    if kind == "max":
        assert n >= 1 and (want["peak"] == thr).all() and want["windows"].sum() == (scores == thr).sum()
    if kind == "above":
        assert n == 0
    for chunk in (W, W + 1, 997, None):
        res = gp.scan_regions(tables[t], [locus], W, s, thr, gap, chunk=chunk)
        assert len(res) == 1 and res[0][0] == "seq0"
        assert RR.same(res[0][1], want), (chunk, res[0][1], want)


def test_invalid_characters_inside_a_region(gp, tables, locus, scanned):
    """an N inside a would-be region fails exactly the windows over it: the region splits, or is bridged by the gap"""
    W, s = 100, 1
    x = locus[:3000].copy()
    clean = gp.scan(tables[4], [x], W, s)[0][2]
    thr = float(np.quantile(clean, 0.25))
    before = RR.regions(clean, W, s, thr, 0)
    big = int(np.argmax(before["windows"]))
    assert before["windows"][big] >= W + 60 and before["windows"][big] == before["end"][big] - W - before["start"][big] + 1
    hole = int(before["start"][big] + 30 + W - 1)                          # the last base of the region's 31st window
    x[[hole, 2999]] = 4
    scores = gp.scan(tables[4], [x], W, s)[0][2]
    assert np.isnan(scores[hole - W + 1:hole + 1]).all() and np.isnan(scores).sum() == W + 1
    for gap in (0, 3, W - 1, W):
        want = RR.regions(scores, W, s, thr, gap)
        for chunk in (W, 997, None):
            got = gp.scan_regions(tables[4], [x], W, s, thr, gap, chunk=chunk)[0][1]
            assert RR.same(got, want), (gap, chunk)
        split = ((want["start"] <= before["end"][big] - W) & (want["end"] - W >= before["start"][big])).sum()
        assert split == (2 if gap < W else 1), (gap, split)                # W failing windows: a gap of W bridges them


def test_twin_windows_keep_the_first_summit(gp, tables, locus):
    """a record that is x + x at a stride that divides len(x): windows a and a + len(x) / s score identically"""
    W, s = 100, 5
    x = locus[:1500]
    rec = np.concatenate([x, x])
    scores = gp.scan(tables[4], [rec], W, s)[0][2]
    twin = len(x) // s
    head = (len(x) - W) // s + 1                                           # (the windows over the seam have no twin)
    assert head + twin == len(scores) and scores[:head].tobytes() == scores[twin:].tobytes()
    thr = float(scores.min())                                              # one region over everything: two maxima
    want = RR.regions(scores, W, s, thr, 0)
    assert len(want["start"]) == 1 and int((scores == scores.max()).sum()) >= 2
    assert want["summit"][0] == int(np.argmax(scores)) * s < len(x)
    for chunk in (W, 777, None):
        assert RR.same(gp.scan_regions(tables[4], [rec], W, s, thr, 0, chunk=chunk)[0][1], want), chunk


def test_several_records(gp, tables, locus, scanned):
    """records in order, one shorter than the width (empty arrays), and the same record alone and behind another"""
    W, s = 600, 1
    thr = _threshold("high", scanned(4, W, s))
    other = np.random.default_rng(8).integers(0, 4, size=1234, dtype=np.uint8)
    res = gp.scan_regions(tables[4], [other, locus[:50], locus, locus[:W - 1]], W, s, thr, 3, chunk=1500)
    assert [name for name, _ in res] == ["seq0", "seq1", "seq2", "seq3"]
    for i in (1, 3):
        assert all(len(res[i][1][k]) == 0 and res[i][1][k].dtype == (np.float64 if k == "peak" else np.int64)
                   for k in RR.FIELDS)
    assert RR.same(res[2][1], RR.regions(scanned(4, W, s), W, s, thr, 3))
    assert RR.same(res[0][1], RR.regions(gp.scan(tables[4], [other], W, s)[0][2], W, s, thr, 3))
    alone = gp.scan_regions(tables[4], [locus], W, s, thr, 3)[0][1]
    assert RR.same(res[2][1], alone)
    with pytest.raises(gp.ModelError, match="no record holds a window"):
        gp.scan_regions(tables[4], [locus[:50]], W, s, thr)


def test_only_the_regions_come_back(gp, tables, locus, scanned):
    W, s = 100, 1
    thr = _threshold("high", scanned(4, W, s))
    for chunk in (997, 2500, None):
        seen = []
        got = gp.scan_regions(tables[4], [locus], W, s, thr, 0, chunk=chunk, on_chunk=seen.append)[0][1]
        assert RR.same(got, RR.regions(scanned(4, W, s), W, s, thr, 0))
        assert sum(c["windows"] for c in seen) == len(scanned(4, W, s))
        assert sum(c["regions"] for c in seen) >= len(got["start"]) > 0    # (a region cut by a chunk counts twice)
        for c in seen:
            assert c["copied_bytes"] <= 64 + 40 * c["regions"], c
            assert c["copied_bytes"] < 8 * c["windows"] or c["windows"] < 16
            assert c["region_kernels_ms"] >= 0.0 and c["profile_kernel_ms"] >= 0.0 and c["score_kernel_ms"] >= 0.0
            assert c["kernel"] == "k_scan_profiles" and c["score_kernel"] == "k_scan_score" and c["wall_ms"] > 0.0


def test_panel_members_equal_the_single_table_calls(gp, tables, locus, scanned):
    """three members, a threshold each: member m's regions are scan_regions' for its own table, bit for bit"""
    rng = np.random.default_rng(11)
    base = tables[4]
    u = np.arange(4 ** base.L, dtype=np.uint32)
    third = rng.standard_normal(4 ** base.L) * np.abs(base.W).mean()
    third = gp.LmerTable(third + third[gp.lmer_rc(u, base.L)], base.kernel_type, base.L, base.k, base.d, base.M, base.H, 0.125)
    flipped = gp.LmerTable(-base.W, base.kernel_type, base.L, base.k, base.d, base.M, base.H, -base.rho)
    panel = gp.LmerPanel([base, flipped, third], ["a", "b", "c"])
    W, s = 100, 7
    thresholds = [_threshold("high", scanned(4, W, s)), -_threshold("low", scanned(4, W, s)), 0.125]
    singles = [gp.scan_regions(panel.table(m), [locus, locus[:300]], W, s, thresholds[m], 3) for m in range(3)]
    assert all(len(r[0][1]["start"]) >= 3 for r in singles)
    for chunk in (W, 997, None):
        seen = []
        res = gp.scan_regions_with_panel(panel, [locus, locus[:300]], W, s, thresholds, 3, chunk=chunk, on_chunk=seen.append)
        assert [name for name, _ in res] == ["seq0", "seq1"] and all(len(members) == 3 for _, members in res)
        for m in range(3):
            for rec in range(2):
                assert RR.same(res[rec][1][m], singles[m][rec][1]), (chunk, m, rec)
        assert all(c["models"] == 3 and len(c["regions"]) == 3 and c["score_kernel"] == "k_panel_scan_score" for c in seen)
    one = gp.scan_regions_with_panel(panel, [locus], W, s, 0.125, 0)       # one threshold for all members
    for m in range(3):
        assert RR.same(one[0][1][m], gp.scan_regions(panel.table(m), [locus], W, s, 0.125, 0)[0][1])


def test_command_line_from_train_to_regions(gp, locus, tmp_path):
    model, weights, pfile = (str(tmp_path / n) for n in ("m.txt", "w.txt", "p.npz"))
    fa, out, pout = str(tmp_path / "s.fa"), str(tmp_path / "o.bed"), str(tmp_path / "p.bed")
    text = gp.codes_to_text(locus[:3000])
    with open(fa, "w") as f:
        f.write(">chrT test locus\n%s\n>tiny\nACGT\n>again\n%s\n" % (text[:1400] + "N" + text[1401:], text[:900]))

    def spawn(*args, ok=True):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == (0 if ok else 1), (args, r.stderr)
        return r

    # (two processes of its own: the command that is the subject, and its refusal; the steps around it in this one)
    assert gp.main(["train", "-t", "4", "-L", "10", "-k", "6", "-d", "3", POS, NEG, model]) == 0
    assert gp.main(["weights", model, weights]) == 0
    r = spawn("scan-regions", "--width", "100", "--stride", "3", "--threshold", "0.25", "--gap", "2", "--chunk", "777",
              weights, fa, out)
    table = gp.load_lmer_table(weights)
    want = gp.scan_regions(table, fa, 100, 3, 0.25, 2)
    assert [name for name, _ in want] == ["chrT test locus", "tiny", "again"]
    for (name, got), (_, scores) in zip(want, [(n, v) for n, _, v in gp.scan(table, fa, 100, 3)]):
        assert RR.same(got, RR.regions(scores, 100, 3, 0.25, 2))
    rows = gp.read_regions(out)
    flat = [(name,) + row for name, r in want for row in zip(*(r[k].tolist() for k in RR.FIELDS))]
    assert len(rows) == len(flat) >= 2 and "%d regions" % len(flat) in r.stderr
    for got, exp in zip(rows, flat):
        assert got[:3] == exp[:3] and got[4:] == exp[4:] and np.float64(got[3]).tobytes() == np.float64(exp[3]).tobytes()
    # a panel of two: the member's name in front
    assert gp.main(["panel", "--names", "wgkm,gkm", pfile, weights, weights]) == 0
    assert gp.main(["scan-regions-panel", "--width", "100", "--stride", "3", "--threshold=0.25,-0.5", "--gap", "2", pfile, fa,
                    pout]) == 0
    prow = gp.read_panel_regions(pout)
    loose = gp.scan_regions(table, fa, 100, 3, -0.5, 2)
    pflat = [(m, name) + row for (name, a), (_, b) in zip(want, loose) for m, r in (("wgkm", a), ("gkm", b))
             for row in zip(*(r[k].tolist() for k in RR.FIELDS))]
    assert [r[:4] + r[5:] for r in prow] == [r[:4] + r[5:] for r in pflat]
    assert [np.float64(r[4]).tobytes() for r in prow] == [np.float64(r[4]).tobytes() for r in pflat]
    # a refusal exits 1 and leaves no file
    bad = str(tmp_path / "bad.bed")
    r = spawn("scan-regions", "--width", "100", "--gap", "-1", weights, fa, bad, ok=False)
    assert "gkmpredict: error:" in r.stderr and "gap" in r.stderr
    for args in (["scan-regions", "--width", "100", "--threshold", "nan", weights, fa, bad],
                 ["scan-regions", "--width", "3001", weights, fa, bad],
                 ["scan-regions-panel", "--width", "100", "--threshold", "1,2,3", pfile, fa, bad]):
        assert gp.main(args) == 1
    assert not os.path.exists(bad) and not os.path.exists(bad + ".tmp")
