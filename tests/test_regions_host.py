"""Regions of a scan without a GPU (gkmqc_amd/gkmpredict.py): the CPU reference (tests/regions_ref.py) on
hand-written cases and the batch builder against it (the two tests that check the yardstick itself, not the feature),
stitch_regions against the reference over every pass pattern, gap and way of cutting up to 12 windows, every refusal of
scan_regions and scan_regions_with_panel before a device is touched, the output files and the parser."""
import os

import numpy as np
import pytest

from tests import regions_ref as RR

NAN, INF = float("nan"), float("inf")
KEYS = ("first", "last", "summit", "windows", "peak")


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _table(gp, kernel_type=4, L=5, k=3, d=2, rho=0.125, seed=1):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal(4 ** L)
    u = np.arange(4 ** L, dtype=np.uint32)
    W = W + W[gp.lmer_rc(u, L)]
    return gp.LmerTable(W, kernel_type, L, k, d, 50, 50.0, rho)


def _rows(r):
    return list(zip(*(r[k].tolist() for k in RR.FIELDS)))


# ------------------------------------------------------------------ the reference itself
def test_reference_on_hand_written_cases():
    """(a check of the yardstick, tests/regions_ref.py, not of the feature: it runs no code of gkmqc_amd)"""
    s = [1.0, 2.0, 0.5, 3.0, 3.0, NAN, 4.0, 0.0, 0.0, 5.0]
    # threshold 1: windows 0 1 . 3 4 . 6 . . 9 pass
    assert _rows(RR.regions(s, 10, 1, 1.0, 0)) == [(0, 11, 2.0, 1, 2), (3, 14, 3.0, 3, 2), (6, 16, 4.0, 6, 1),
                                                    (9, 19, 5.0, 9, 1)]
    assert _rows(RR.regions(s, 10, 1, 1.0, 1)) == [(0, 16, 4.0, 6, 5), (9, 19, 5.0, 9, 1)]
    assert _rows(RR.regions(s, 10, 1, 1.0, 2)) == [(0, 19, 5.0, 9, 6)]
    # a stride and a width: starts are window * stride, the end is the last start + width
    assert _rows(RR.regions(s, 100, 7, 1.0, 0)) == [(0, 107, 2.0, 7, 2), (21, 128, 3.0, 21, 2), (42, 142, 4.0, 42, 1),
                                                     (63, 163, 5.0, 63, 1)]
    # a threshold equal to a score passes it; one above the maximum gives empty arrays of the right types
    assert _rows(RR.regions(s, 10, 1, 5.0, 0)) == [(9, 19, 5.0, 9, 1)]
    none = RR.regions(s, 10, 1, 5.5, 0)
    assert all(len(none[k]) == 0 for k in RR.FIELDS) and none["peak"].dtype == np.float64 and none["start"].dtype == np.int64
    # -inf passes every scored window, never a NaN; +inf is a score like any other
    assert _rows(RR.regions(s, 10, 1, -INF, 0)) == [(0, 14, 3.0, 3, 5), (6, 19, 5.0, 9, 4)]
    assert _rows(RR.regions([NAN, -INF, INF, INF, NAN], 3, 1, -INF, 0)) == [(1, 6, INF, 2, 3)]
    assert _rows(RR.regions([NAN, NAN], 3, 1, -INF, 5)) == []
    # all equal: the summit is the first window; -0.0 passes a threshold of 0.0 and ties with 0.0
    assert _rows(RR.regions([2.0] * 5, 4, 2, 2.0, 0)) == [(0, 12, 2.0, 0, 5)]
    r = RR.regions([-1.0, -0.0, 0.0, -1.0], 4, 1, 0.0, 0)
    assert _rows(r) == [(1, 6, 0.0, 1, 2)] and np.signbit(r["peak"][0])
    assert _rows(RR.regions([], 4, 1, 0.0, 0)) == []


# ------------------------------------------------------------------ stitching
def _cut_regions(scores, cuts, thr, gap):
    """every chunk on its own through the reference -> stitch_regions' input, in the record's window indices"""
    out, edges = [], [0] + list(cuts) + [len(scores)]
    for a, b in zip(edges[:-1], edges[1:]):
        r = RR.window_regions(scores[a:b], thr, gap)
        out.append(dict(first=r["first"] + a, last=r["last"] + a, summit=r["summit"] + a, windows=r["windows"],
                        peak=r["peak"]))
    return out


def test_stitch_on_hand_written_cases(gp):
    s = np.array([1.0, 2.0, 2.0, 0.0, 2.0, 1.0, 0.0, 0.0, 3.0])
    for gap in (0, 1, 2, 7):
        want = RR.window_regions(s, 1.0, gap)
        for cuts in ([], [1], [2], [3], [4], [1, 2, 3, 4, 5, 6, 7, 8], [2, 5], [4, 8]):
            got = gp.stitch_regions(_cut_regions(s, cuts, 1.0, gap), gap)
            assert RR.same(got, want, KEYS), (gap, cuts, got, want)
    # a tie across a boundary keeps the earlier chunk's summit; a cascade over one-window chunks
    got = gp.stitch_regions(_cut_regions(np.full(6, 2.0), [1, 2, 3, 4, 5], 2.0, 0), 0)
    assert [got[k].tolist() for k in KEYS] == [[0], [5], [0], [6], [2.0]]
    empty = gp.stitch_regions([], 3)
    assert RR.same(empty, RR.window_regions([], 0.0, 3), KEYS)
    assert RR.same(gp.stitch_regions(_cut_regions(np.zeros(4), [2], 1.0, 0), 0), empty, KEYS)


UNTIED = np.array([3.0, 9.0, 1.0, 12.0, 5.0, 11.0, 2.0, 8.0, 10.0, 4.0, 7.0, 6.0])
TIED = np.array([2.0, 1.0, 2.0, 2.0, 1.0, 2.0, 1.0, 1.0, 2.0, 2.0, 1.0, 2.0])   # the maximum recurs, across any cut


def test_stitch_case_by_case(gp):
    """n <= 6: every pass pattern, gap 0..3, every cut, one stitch_regions call per case with one dict per chunk"""
    for n in range(1, 7):
        for pattern in range(1 << n):
            for values in (UNTIED, TIED):
                s = np.where([(pattern >> i) & 1 for i in range(n)], values[:n], 0.0)
                for gap in range(4):
                    want = RR.window_regions(s, 1.0, gap)
                    for cut in range(1 << (n - 1)):
                        cuts = [i + 1 for i in range(n - 1) if (cut >> i) & 1]
                        got = gp.stitch_regions(_cut_regions(s, cuts, 1.0, gap), gap)
                        assert RR.same(got, want, KEYS), (s, gap, cuts)


def _batch_layout(bits, cutting):
    """Every (pattern, cut) pair of a batch as one case, pattern-major.  bits (patterns, n) bool: window i passes; cutting
    (cuts, n) bool: a chunk begins at window i (column 0 always).  -> (case, i, apart, severed) per passing window, case
    by case: how far back the passing window before it lies (n + 9 when there is none) and whether a cut separates the
    two."""
    pats, n = bits.shape
    idx = np.arange(n, dtype=np.int8)
    seen = np.maximum.accumulate(np.where(bits, idx, np.int8(-1)), axis=1)
    prev = np.concatenate((np.full((pats, 1), -1, dtype=np.int8), seen[:, :-1]), axis=1)     # the passing window before i
    chunk0 = np.maximum.accumulate(np.where(cutting, idx, np.int8(0)), axis=1)               # where i's chunk begins
    passing = np.broadcast_to(bits[:, None, :], (pats, len(cutting), n))
    severed = (prev[:, None, :] < chunk0[None, :, :])[passing]                               # (prev < 0 <= chunk0 too)
    apart = np.broadcast_to(np.where(prev < 0, np.int8(n + 9), idx - prev)[:, None, :], passing.shape)[passing]
    case, i = np.nonzero(passing.reshape(-1, n))
    return case, i, apart, severed


def _batch_regions(layout, values, gap, pitch):
    """_cut_regions for all cases of a layout at once: every chunk of every case on its own, case c at the window indices
    c * pitch + i -> one dict of the regions of all chunks of all cases, ascending."""
    case, i, apart, severed = layout
    begins = severed | (apart > gap + 1)
    g = case.astype(np.int64) * pitch + i
    v = values[i]
    at = np.flatnonzero(begins)
    group = np.cumsum(begins) - 1
    top = np.flatnonzero(v == np.maximum.reduceat(v, at)[group])
    top = top[np.concatenate(([True], group[top][1:] != group[top][:-1]))]
    return dict(first=g[at], last=g[np.append(at[1:], len(g)) - 1], summit=g[top],
                windows=np.diff(np.append(at, len(g))), peak=v[top])


def _all_cuts(n):
    """(2^(n-1), n) bool: every way of cutting n windows into consecutive chunks"""
    ncut = 1 << (n - 1)
    return np.concatenate((np.ones((ncut, 1), bool), ((np.arange(ncut)[:, None] >> np.arange(n - 1)) & 1).astype(bool)), axis=1)


def test_batch_builder_is_the_reference_per_chunk():
    """the vectorised builder the exhaustive test relies on, against _cut_regions case by case (n = 5, every case); a
    check of this file's own helper against the yardstick, not of the feature: it runs no code of gkmqc_amd"""
    n, pitch = 5, 20
    bits = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(bool)
    cutting = _all_cuts(n)
    layout = _batch_layout(bits, cutting)
    for values in (UNTIED, TIED):
        for gap in range(4):
            got = _batch_regions(layout, values, gap, pitch)
            want = {k: [np.empty(0, np.int64)] for k in KEYS}
            for c in range(len(bits) * len(cutting)):
                s = np.where(bits[c // len(cutting)], values[:n], 0.0)
                for part in _cut_regions(s, np.flatnonzero(cutting[c % len(cutting)])[1:].tolist(), 1.0, gap):
                    for k in KEYS:
                        want[k].append(part[k] + (c * pitch if k in KEYS[:3] else 0))
            assert all(np.array_equal(got[k], np.concatenate(want[k])) for k in KEYS), (gap,)


def test_stitch_exhaustively(gp):
    """Every pass pattern of n <= 12 windows, gap 0..3, every way of cutting them into consecutive chunks, untied and tied
    scores: the uncut reference comes out.  The cases of a batch stand side by side in one index space, far enough apart
    that none reaches its neighbour, and go through stitch_regions in one call (the per-chunk regions of all of them, in
    order, divided into a few dicts); test_stitch_case_by_case makes one call per case for n <= 6."""
    checked = 0
    for n in range(1, 13):
        cutting = _all_cuts(n)
        ncut, pitch = len(cutting), n + 5                                  # (pitch - n + 1 > gap + 1)
        offs = np.arange(ncut, dtype=np.int64) * pitch
        per = max(1, min(1 << n, (1 << 18) // ncut))                       # patterns per batch
        for p0 in range(0, 1 << n, per):
            pats = np.arange(p0, min(1 << n, p0 + per))
            bits = ((pats[:, None] >> np.arange(n)) & 1).astype(bool)
            layout = _batch_layout(bits, cutting)
            for values in (UNTIED, TIED):
                for gap in range(4):
                    built = _batch_regions(layout, values, gap, pitch)
                    third = len(built["first"]) // 3
                    pieces = [{k: a[lo:hi] for k, a in built.items()}
                              for lo, hi in ((0, third), (third, third), (third, len(built["first"])))]
                    got = gp.stitch_regions(pieces, gap)
                    want = {k: [] for k in KEYS}
                    for j, row in enumerate(bits):
                        r = RR.window_regions(np.where(row, values[:n], 0.0), 1.0, gap)
                        base = offs + j * ncut * pitch
                        for k in KEYS:
                            want[k].append((np.add.outer(base, r[k]) if k in KEYS[:3] else np.tile(r[k], (ncut, 1))).ravel())
                    for k in KEYS:
                        w = np.concatenate(want[k])
                        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (n, gap, p0, k)
                    checked += len(bits) * ncut
    assert checked == 8 * sum((1 << n) * (1 << (n - 1)) for n in range(1, 13))


# ------------------------------------------------------------------ refusals
def test_api_refusals_come_before_any_device_work(gp):
    """(no GPU here: anything that reached the device would fail otherwise)"""
    tab = _table(gp)
    x = [np.zeros(100, dtype=np.uint8)]
    for kw, msg in ((dict(width=4), "below L"), (dict(width=2048), "above 2047"), (dict(width=20, stride=0), "stride"),
                    (dict(width=20, chunk=19), "chunk"), (dict(width=101), "no record holds a window"),
                    (dict(width=20, gap=-1), "gap must be at least 0"), (dict(width=20, gap=1.0), "gap must be an integer"),
                    (dict(width=20, gap=(1 << 40) + 1), "gap must be at most 2.40 windows"),
                    (dict(width=20, gap=True), "gap must be an integer"), (dict(width=20, gap=None), "gap must be an integer"),
                    (dict(width=20, threshold=NAN), "threshold is NaN"),
                    (dict(width=20, threshold="high"), "threshold must be a number")):
        with pytest.raises(gp.ModelError, match=msg):
            gp.scan_regions(tab, x, **kw)
        if "no record" not in msg:
            with pytest.raises(gp.ModelError, match=msg):
                gp.check_scan_regions(tab, **dict(dict(stride=1), **kw))
    assert gp.check_scan_regions(tab, 20, 1, -INF, 0) == -INF             # (the checks hand back the thresholds as floats)
    assert gp.check_scan_regions(tab, 20, 3, np.float32(0.5), np.int64(5), 20) == 0.5
    assert gp.check_scan_regions(tab, 20, 1, 1, 1 << 40) == 1.0
    model = gp.Model(4, 5, 3, 2, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.0, 1, [1.0, 1.0], ["a", "b"],
                     [np.zeros(9, np.uint8), np.ones(9, np.uint8)])
    with pytest.raises(gp.ModelError, match="weight table"):
        gp.scan_regions(model, x, 20)
    panel = gp.LmerPanel([_table(gp, seed=s) for s in (1, 2, 3)], ["a", "b", "c"])
    with pytest.raises(gp.ModelError, match="weight table"):
        gp.scan_regions(panel, x, 20)
    with pytest.raises(gp.ModelError, match="weight panel"):
        gp.scan_regions_with_panel(tab, x, 20)
    for kw, msg in ((dict(width=4), "below L"), (dict(width=20, stride=0), "stride"), (dict(width=20, chunk=19), "chunk"),
                    (dict(width=101), "no record holds a window"), (dict(width=20, gap=-2), "gap must be at least 0"),
                    (dict(width=20, gap=1 << 41), "gap must be at most 2.40 windows"),
                    (dict(width=20, gap=0.5), "gap must be an integer"), (dict(width=20, threshold=NAN), "threshold is NaN"),
                    (dict(width=20, threshold=[0.0, NAN, 1.0]), "threshold is NaN"),
                    (dict(width=20, threshold=[0.0, 1.0]), "2 thresholds for the panel's 3 members"),
                    (dict(width=20, threshold=[0.0] * 4), "4 thresholds for the panel's 3 members"),
                    (dict(width=20, threshold=[]), "0 thresholds for the panel's 3 members")):
        with pytest.raises(gp.ModelError, match=msg):
            gp.scan_regions_with_panel(panel, x, **kw)
        if "no record" not in msg:
            with pytest.raises(gp.ModelError, match=msg):
                gp.check_panel_scan_regions(panel, **dict(dict(stride=1), **kw))
    assert gp.check_panel_scan_regions(panel, 20, 1, [0.0, -INF, 2.5], 3) == [0.0, -INF, 2.5]
    assert gp.check_panel_scan_regions(panel, 20, 1, np.array([0.0, 1.0, 2.0])) == [0.0, 1.0, 2.0]
    assert gp.check_panel_scan_regions(panel, 20, 1, 0.25) == [0.25, 0.25, 0.25]


def test_command_line_refusals_exit_1_and_write_nothing(gp, tmp_path, capsys):
    tab = _table(gp)
    weights, fa, out = str(tmp_path / "w.txt"), str(tmp_path / "s.fa"), str(tmp_path / "o.bed")
    pfile = str(tmp_path / "p.npz")
    tab.save(weights)
    gp.LmerPanel([tab, _table(gp, seed=2)], ["a", "b"]).save(pfile)
    with open(fa, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n")
    cases = [("scan-regions", ["--width", "4", weights, fa, out], "below L"),
             ("scan-regions", ["--width", "20", "--stride", "0", weights, fa, out], "stride"),
             ("scan-regions", ["--width", "20", "--chunk", "10", weights, fa, out], "chunk"),
             ("scan-regions", ["--width", "41", weights, fa, out], "no record holds a window"),
             ("scan-regions", ["--width", "20", "--gap", "-1", weights, fa, out], "gap must be at least 0"),
             ("scan-regions", ["--width", "20", "--threshold", "nan", weights, fa, out], "threshold is NaN"),
             ("scan-regions", ["--width", "20", "--threshold", "high", weights, fa, out], "no number"),
             ("scan-regions", ["--width", "20", "--threshold", "1,2", weights, fa, out], "no number"),
             ("scan-regions", ["--width", "20", weights, str(tmp_path / "missing.fa"), out], "cannot read"),
             ("scan-regions", ["--width", "20", str(tmp_path / "missing.txt"), fa, out], "missing.txt"),
             ("scan-regions-panel", ["--width", "20", weights, fa, out], "not a panel file"),
             ("scan-regions-panel", ["--width", "4", pfile, fa, out], "below L"),
             ("scan-regions-panel", ["--width", "20", "--gap", "-1", pfile, fa, out], "gap must be at least 0"),
             ("scan-regions-panel", ["--width", "20", "--threshold", "1,2,3", pfile, fa, out], "3 thresholds for the panel's 2"),
             ("scan-regions-panel", ["--width", "20", "--threshold", "1,nan", pfile, fa, out], "threshold is NaN"),
             ("scan-regions-panel", ["--width", "41", pfile, fa, out], "no record holds a window")]
    for cmd, args, msg in cases:
        assert gp.main([cmd] + args) == 1, (cmd, args)
        assert msg in capsys.readouterr().err, (cmd, args)
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    with pytest.raises(SystemExit):
        gp.main(["scan-regions", weights, fa, out])                        # --width is required
    with pytest.raises(SystemExit):
        gp.main(["scan-regions", "--width", "20", "--gap", "1.5", weights, fa, out])


# ------------------------------------------------------------------ files and the parser
def _regions(start, end, peak, summit, windows):
    return dict(start=np.array(start, np.int64), end=np.array(end, np.int64), peak=np.array(peak, np.float64),
                summit=np.array(summit, np.int64), windows=np.array(windows, np.int64))


def test_files_round_trip(gp, tmp_path):
    peaks = [0.1, 1.0 / 3.0, 2.0 ** -1074, 1.7976931348623157e308, -0.0, INF, -1.2345678901234567e-5, 0.30000000000000004]
    n = len(peaks)
    a = _regions(list(range(0, 10 * n, 10)), list(range(600, 600 + 10 * n, 10)), peaks, list(range(5, 5 + 10 * n, 10)),
                 list(range(1, n + 1)))
    none = _regions([], [], [], [], [])
    b = _regions([3 << 40], [(3 << 40) + 2047], [-2.5], [3 << 40], [1])
    results = [("chr1 with\ttab", a), ("empty", none), ("chrB", b)]
    path = str(tmp_path / "r.bed")
    assert gp.write_regions(path, results) == n + 1
    rows = gp.read_regions(path)
    assert len(rows) == n + 1 and [r[0] for r in rows] == ["chr1 with\ttab"] * n + ["chrB"]
    for row, want in zip(rows, _rows(a) + _rows(b)):
        assert row[1:3] == want[0:2] and row[4:] == want[3:]
        assert np.float64(row[3]).tobytes() == np.float64(want[2]).tobytes()       # the same double, -0.0's sign included
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "chr1 with\ttab\t0\t600\t%.17g\t5\t1" % 0.1
    # the panel variant: the member's name in front, records in file order, members in panel order
    ppath = str(tmp_path / "p.bed")
    assert gp.write_panel_regions(ppath, ["m0", "m1"], [("chr1 with\ttab", [a, none]), ("chrB", [b, b])]) == n + 2
    prow = gp.read_panel_regions(ppath)
    assert [(r[0], r[1]) for r in prow] == [("m0", "chr1 with\ttab")] * n + [("m0", "chrB"), ("m1", "chrB")]
    for row, want in zip(prow, _rows(a) + _rows(b) + _rows(b)):
        assert np.float64(row[4]).tobytes() == np.float64(want[2]).tobytes() and row[2:4] + row[5:] == want[:2] + want[3:]
    assert len(open(ppath).read().split("\n")[0].split("\t")) == 8          # (the record's name holds a tab of its own)
    # nothing to write: an empty file
    assert gp.write_regions(path, [("x", none)]) == 0 and open(path).read() == "" and gp.read_regions(path) == []


def test_parser(gp):
    p = gp.build_parser()
    a = p.parse_args(["scan-regions", "--width", "600", "w.txt", "s.fa", "o.bed"])
    assert (a.cmd, a.weights, a.seqs_fa, a.output) == ("scan-regions", "w.txt", "s.fa", "o.bed")
    assert (a.width, a.stride, a.threshold, a.gap, a.chunk, a.device) == (600, 1, "0", 0, None, 0)
    a = p.parse_args(["scan-regions", "--width", "600", "--stride", "10", "--threshold", "-1.5", "--gap", "3", "--chunk",
                      "5000", "--device", "1", "w.txt", "s.fa", "o.bed"])
    assert (a.width, a.stride, a.threshold, a.gap, a.chunk, a.device) == (600, 10, "-1.5", 3, 5000, 1)
    assert gp.region_thresholds(a.threshold) == -1.5
    a = p.parse_args(["scan-regions-panel", "--width", "64", "--threshold=-1,0.5,-inf", "p.npz", "s.fa", "o.bed"])
    assert (a.cmd, a.panel, a.seqs_fa, a.output, a.gap) == ("scan-regions-panel", "p.npz", "s.fa", "o.bed", 0)
    assert gp.region_thresholds(a.threshold, panel=True) == [-1.0, 0.5, -INF]
    assert gp.region_thresholds("2", panel=True) == 2.0 and gp.region_thresholds("-inf") == -INF
    with pytest.raises(gp.ModelError):
        gp.region_thresholds("1,,2", panel=True)
