"""Score distributions of a scan on the GPU at product level (gkmpredict.scan_quantiles, scan_tail_counts, their panel
forms and their command line).  Two sentences are the contract: scan_quantiles equals tests/dist_ref.py
applied to `scan`'s own output, bit for bit, whatever the chunk, the collect cap and the order of the requests; and
scan_tail_counts(t) equals the summed `windows` of scan_regions(threshold=t, gap=0) on the same input.

The inputs are test_regions_gpu.py's: the locus (the golden positives and negatives back to back, 6 000 bases) and
C-SVC tables of types 0 and 4 trained on the golden files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dist_ref as DR
from tests import helpers

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")
SHAPES = ((100, 1), (100, 7), (600, 1))
Q = (0.5, 0.0, 1.0, 0.99, 0.01, 0.5)
INF = float("inf")


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


def _pooled(gp, table, records, W, s):
    return np.concatenate([v for _, _, v in gp.scan(table, records, W, s)])


def _check_quantiles(got, scores, q=Q):
    n = int((~np.isnan(scores)).sum())
    ranks = DR.quantile_ranks(n, q)
    assert got["scored"] == n and got["unscored"] == len(scores) - n and got["q"] == list(q)
    assert got["ranks"].tolist() == ranks
    assert DR.same_bits(got["values"], DR.order_statistics(scores, ranks)), (got["values"], DR.order_statistics(scores, ranks))


@pytest.mark.parametrize("W,s", SHAPES)
@pytest.mark.parametrize("t", [0, 4])
def test_quantiles_at_every_chunk_and_cap(gp, tables, locus, scanned, t, W, s):
    scores = scanned(t, W, s)
    levels = len(gp.dist_level_bits())
    # A pass is a whole scan and the smallest chunks make the most launches: every cap at 997, every chunk at one cap,
    # and the chunks of one and two windows over the head of the locus only (1 501 windows at stride 1).
    head = locus[:W + 1500]
    head_scores = gp.scan(tables[t], [head], W, s)[0][2]
    for chunk, caps in ((W, (None,)), (W + 1, (50,)), (997, (1, 50, None)), (None, (1,))):
        for cap in caps:
            kw = {} if cap is None else dict(collect_cap=cap)
            small = chunk in (W, W + 1)
            got = gp.scan_quantiles(tables[t], [head if small else locus], W, s, q=Q, chunk=chunk, **kw)
            _check_quantiles(got, head_scores if small else scores)
            kinds = [p["kind"] for p in got["passes"]]
            assert [p["prefix_bits"] for p in got["passes"]] == ([0] + gp.dist_boundaries())[:len(kinds)]
            if cap == 1:                                                   # several ranks never fit a cap of 1: every level
                assert kinds == ["hist"] * levels
            elif cap is None:                                              # exactly one histogram pass, then the collect
                assert kinds == ["hist", "collect"]
            else:
                assert kinds[-1] == "collect" and 2 <= len(kinds) <= levels + 1
    got = gp.scan_quantiles(tables[t], [locus], W, s, ranks=[len(scores) - 1, 0, 7, 7], collect_cap=50)
    assert got["q"] is None and got["ranks"].tolist() == [len(scores) - 1, 0, 7, 7]
    assert DR.same_bits(got["values"], DR.order_statistics(scores, got["ranks"]))
    assert got["values"][0] == scores.max() and got["values"][1] == scores.min()


def test_twin_record_where_every_score_occurs_twice(gp, tables, locus):
    W, s = 100, 5
    x = locus[:1500]
    rec = np.concatenate([x, x])
    scores = gp.scan(tables[4], [rec], W, s)[0][2]
    twin = len(x) // s
    head = (len(x) - W) // s + 1
    assert head + twin == len(scores) and scores[:head].tobytes() == scores[twin:].tobytes()
    for cap, chunks in ((1, (W, None)), (2, (777,)), (50, (777,)), (1 << 20, (W, None))):
        for chunk in chunks:
            _check_quantiles(gp.scan_quantiles(tables[4], [rec], W, s, q=Q, chunk=chunk, collect_cap=cap), scores)
    n = len(scores)
    assert int((scores == scores.max()).sum()) >= 2                        # the maximum has a twin: the two top ranks tie
    got = gp.scan_quantiles(tables[4], [rec], W, s, ranks=[n - 1, n - 2], collect_cap=1)
    assert got["values"][0] == got["values"][1] == scores.max()
    assert [p["kind"] for p in got["passes"]] == ["hist"] * 5 and got["passes"][-1]["targets"] == 1


def test_invalid_characters_are_unscored(gp, tables, locus):
    W, s = 100, 1
    x = locus[:3000].copy()
    x[[1234, 2999]] = 4
    scores = gp.scan(tables[4], [x], W, s)[0][2]
    assert np.isnan(scores).sum() == W + 1
    for chunk in (W, 997, None):
        if chunk != W:                                                     # (several scans: not at one window per chunk)
            got = gp.scan_quantiles(tables[4], [x], W, s, q=Q, chunk=chunk, collect_cap=50)
            _check_quantiles(got, scores)
            assert got["unscored"] == W + 1
        tail = gp.scan_tail_counts(tables[4], [x], W, s, [-INF, 0.0], chunk=chunk)
        assert tail["unscored"] == W + 1 and tail["counts"][0] == tail["scored"] == len(scores) - W - 1
    everything = np.full(300, 4, dtype=np.uint8)
    with pytest.raises(gp.ModelError, match="no window has a score"):
        gp.scan_quantiles(tables[4], [everything], W, s, q=[0.5])
    tail = gp.scan_tail_counts(tables[4], [everything], W, s, [-INF])
    assert tail["scored"] == 0 and tail["unscored"] == 201 and tail["counts"].tolist() == [0]


def test_several_records_are_pooled(gp, tables, locus):
    W, s = 600, 1
    other = np.random.default_rng(8).integers(0, 4, size=1234, dtype=np.uint8)
    records = [other, locus[:50], locus, locus[:W - 1]]
    pooled = _pooled(gp, tables[4], records, W, s)
    assert len(pooled) == (1234 - W + 1) + (len(locus) - W + 1)
    for cap in (50, 1 << 20):
        _check_quantiles(gp.scan_quantiles(tables[4], records, W, s, q=Q, chunk=1500, collect_cap=cap), pooled)
    thr = [float(np.median(pooled)), -INF]
    got = gp.scan_tail_counts(tables[4], records, W, s, thr, chunk=1500)
    assert np.array_equal(got["counts"], DR.tail_counts(pooled, thr)) and got["scored"] == len(pooled)
    with pytest.raises(gp.ModelError, match="no record holds a window"):
        gp.scan_quantiles(tables[4], [locus[:50]], W, s, q=[0.5])
    with pytest.raises(gp.ModelError, match="0..n-1; %d windows" % len(pooled)):
        gp.scan_quantiles(tables[4], records, W, s, ranks=[len(pooled)])


@pytest.mark.parametrize("W,s", SHAPES)
@pytest.mark.parametrize("t", [0, 4])
def test_tail_counts(gp, tables, locus, scanned, t, W, s):
    scores = scanned(t, W, s)
    n = len(scores)
    stats = DR.order_statistics(scores, [n // 10, n // 2, (9 * n) // 10])
    thr = [float(scores.min()), float(scores.max()), float(np.nextafter(scores.max(), INF)), -INF, INF] + stats.tolist() + [0.0]
    want = DR.tail_counts(scores, thr)
    assert want[0] == want[3] == n and want[1] >= 1 and want[2] == want[4] == 0 and n > want[5] > want[6] > want[7] > 0
    for chunk in (W, W + 1, 997, None):
        seen = []
        got = gp.scan_tail_counts(tables[t], [locus], W, s, thr, chunk=chunk, on_chunk=seen.append)
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want), (chunk, got["counts"], want)
        assert got["scored"] == n == got["counts"][3] and got["unscored"] == 0 and DR.same_bits(got["thresholds"], thr)
        assert sum(c["windows"] for c in seen) == n
        assert all(c["copied_bytes"] == 0 and c["dist_kernels_ms"] >= 0.0 and c["kernel"] == "k_scan_profiles" for c in seen)
    regions = [int(gp.scan_regions(tables[t], [locus], W, s, x, 0)[0][1]["windows"].sum()) for x in thr]
    assert regions == want.tolist()
    many = np.random.default_rng(3).permutation(np.concatenate([scores[:2000], scores[:96]]))   # unsorted, duplicates
    assert np.array_equal(gp.scan_tail_counts(tables[t], [locus], W, s, many)["counts"], DR.tail_counts(scores, many))


def test_only_histograms_and_the_collected_values_come_back(gp, tables, locus, scanned):
    W, s = 100, 1
    scores = scanned(4, W, s)
    seen = []
    got = gp.scan_quantiles(tables[4], [locus], W, s, q=[0.99], chunk=997, collect_cap=50, on_pass=seen.append)
    _check_quantiles(got, scores, [0.99])
    assert len(seen) == len(got["passes"]) >= 2 and seen[-1]["kind"] == "collect" and seen[0]["targets"] == 0
    bits = gp.dist_level_bits()
    for i, p in enumerate(seen[:-1]):
        assert p["kind"] == "hist" and p["copied_bytes"] == 8 << bits[i] and p["dist_kernels_ms"] >= 0.0
    assert 8 < seen[-1]["copied_bytes"] <= 8 + 8 * 50


def test_panel_members_equal_the_single_table_calls(gp, tables, locus):
    rng = np.random.default_rng(11)
    base = tables[4]
    u = np.arange(4 ** base.L, dtype=np.uint32)
    third = rng.standard_normal(4 ** base.L) * np.abs(base.W).mean()
    third = gp.LmerTable(third + third[gp.lmer_rc(u, base.L)], base.kernel_type, base.L, base.k, base.d, base.M, base.H, 0.125)
    flipped = gp.LmerTable(-base.W, base.kernel_type, base.L, base.k, base.d, base.M, base.H, -base.rho)
    panel = gp.LmerPanel([base, flipped, third], ["a", "b", "c"])
    W, s = 100, 7
    records = [locus, locus[:300]]
    singles = [gp.scan_quantiles(panel.table(m), records, W, s, q=Q, collect_cap=50) for m in range(3)]
    thr = [0.125, -INF, float(singles[0]["values"][3]), -float(singles[0]["values"][3]), INF]
    tails = [gp.scan_tail_counts(panel.table(m), records, W, s, thr) for m in range(3)]
    assert len({x["values"].tobytes() for x in singles}) == 3
    for chunk in (W, 997, None):
        for cap in (50, 1 << 20):
            seen = []
            got = gp.scan_quantiles_with_panel(panel, records, W, s, q=Q, chunk=chunk, collect_cap=cap, on_pass=seen.append)
            assert got["values"].shape == got["ranks"].shape == (3, len(Q)) and got["q"] == list(Q)
            for m in range(3):
                assert DR.same_bits(got["values"][m], singles[m]["values"]), (chunk, cap, m)
                assert got["ranks"][m].tolist() == singles[m]["ranks"].tolist()
                assert got["scored"][m] == singles[m]["scored"] and got["unscored"][m] == singles[m]["unscored"]
            assert seen == got["passes"] and seen[0]["kind"] == ["hist"] * 3 and seen[0]["prefix_bits"] == [0] * 3
            if cap == 1 << 20:
                assert [p["kind"] for p in seen] == [["hist"] * 3, ["collect"] * 3]
        seen = []
        got = gp.scan_tail_counts_with_panel(panel, records, W, s, thr, chunk=chunk, on_chunk=seen.append)
        assert got["counts"].shape == (3, len(thr)) and got["counts"].dtype == np.int64
        for m in range(3):
            assert np.array_equal(got["counts"][m], tails[m]["counts"]) and got["scored"][m] == tails[m]["scored"]
        assert all(c["models"] == 3 and c["score_kernel"] == "k_panel_scan_score" for c in seen)


def test_command_line_from_train_to_quantiles_and_tail(gp, locus, tmp_path):
    model, weights = str(tmp_path / "m.txt"), str(tmp_path / "w.txt")
    fa, qout, tout = str(tmp_path / "s.fa"), str(tmp_path / "q.tsv"), str(tmp_path / "t.tsv")
    text = gp.codes_to_text(locus[:3000])
    with open(fa, "w") as f:
        f.write(">chrT test locus\n%s\n>tiny\nACGT\n>again\n%s\n" % (text[:1400] + "N" + text[1401:], text[:900]))

    def spawn(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)
        return r

    assert gp.main(["train", "-t", "4", "-L", "10", "-k", "6", "-d", "3", POS, NEG, model]) == 0
    assert gp.main(["weights", model, weights]) == 0
    table = gp.load_lmer_table(weights)
    r = spawn("scan-quantiles", "--width", "100", "--stride", "3", "--q", "0.99,0.5,0", "--chunk", "777", "--collect-cap", "40",
              weights, fa, qout)
    want = gp.scan_quantiles(table, fa, 100, 3, q=[0.99, 0.5, 0.0])
    _check_quantiles(want, _pooled(gp, table, fa, 100, 3), [0.99, 0.5, 0.0])
    got = gp.read_quantiles(qout)
    assert (got["scored"], got["unscored"], got["q"]) == (want["scored"], want["unscored"], want["q"]) and want["unscored"] > 0
    assert got["ranks"].tolist() == want["ranks"].tolist() and DR.same_bits(got["values"], want["values"])
    assert "3 order statistics" in r.stderr
    thr = "%.17g,-inf,0.25" % want["values"][0]
    spawn("scan-tail", "--width", "100", "--stride", "3", "--thresholds", thr, "--chunk", "777", weights, fa, tout)
    wtail = gp.scan_tail_counts(table, fa, 100, 3, [float(x) for x in thr.split(",")])
    gtail = gp.read_tail_counts(tout)
    assert (gtail["scored"], gtail["unscored"]) == (wtail["scored"], wtail["unscored"]) == (want["scored"], want["unscored"])
    assert np.array_equal(gtail["counts"], wtail["counts"]) and DR.same_bits(gtail["thresholds"], wtail["thresholds"])
    assert wtail["counts"][1] == wtail["scored"]
    assert np.array_equal(wtail["counts"], DR.tail_counts(_pooled(gp, table, fa, 100, 3), wtail["thresholds"]))
