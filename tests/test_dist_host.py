"""The host side of the score distributions of a scan, no GPU: the order-preserving key, the level
arithmetic, the refinement search driven by a numpy stand-in of its two callables, every refusal, the file formats and
the command line's refusals."""
import os

import numpy as np
import pytest

from tests import dist_ref as DR

NAN, INF = float("nan"), float("inf")
TINY, HUGE = 5e-324, np.finfo(np.float64).max


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


def test_key_order_and_round_trip(gp):
    up = np.nextafter
    ladder = np.array([-INF, -HUGE, up(-HUGE, 0.0), up(-1.0, -INF), -1.0, up(-1.0, 0.0), -2.2250738585072014e-308,
                       up(-TINY, -INF), -TINY, -0.0, 0.0, TINY, up(TINY, INF), 2.2250738585072014e-308, up(1.0, 0.0), 1.0,
                       up(1.0, INF), up(HUGE, 0.0), HUGE, INF])
    assert (np.diff(ladder[:9]) > 0).all() and (np.diff(ladder[10:]) > 0).all()
    for keys in (gp.score_keys(ladder), DR.key(ladder)):
        assert keys.dtype == np.uint64 and (keys[1:] > keys[:-1]).all()    # strictly: -0.0 below +0.0
    assert np.array_equal(gp.score_keys(ladder), DR.key(ladder))
    assert DR.same_bits(gp.keys_to_scores(gp.score_keys(ladder)), ladder) and DR.same_bits(DR.unkey(DR.key(ladder)), ladder)
    # the formula itself, and a bijection on arbitrary words (NaN payloads included)
    words = np.random.default_rng(0).integers(0, 1 << 64, size=5000, dtype=np.uint64)
    want = np.array([b ^ ((1 << 64) - 1 if b >> 63 else 1 << 63) for b in words.tolist()], dtype=np.uint64)
    assert np.array_equal(gp.score_keys(words.view(np.float64)), want)
    assert np.array_equal(gp.keys_to_scores(want).view(np.uint64), words)
    assert np.array_equal(gp.score_keys(gp.keys_to_scores(words)), words)
    rnd = np.random.default_rng(1).standard_normal(2000) * 10.0 ** np.random.default_rng(2).integers(-300, 300, 2000)
    assert np.array_equal(np.argsort(gp.score_keys(rnd), kind="stable"), np.argsort(rnd, kind="stable"))


@pytest.mark.parametrize("B", range(8, 17))
def test_level_arithmetic(gp, B):
    bits = gp.dist_level_bits(B)
    levels = -(-64 // B)
    assert len(bits) == levels and sum(bits) == 64 and bits[1:] == [B] * (levels - 1) and 1 <= bits[0] <= B
    assert bits[0] == 64 - B * (levels - 1)
    bounds = gp.dist_boundaries(B)
    assert bounds[-1] == 64 and bounds[0] == bits[0] and np.diff(bounds).tolist() == bits[1:]
    assert {8: 8, 9: 1, 10: 4, 11: 9, 12: 4, 13: 12, 14: 8, 15: 4, 16: 16}[B] == bits[0]


def test_the_build_resolves_13_bits_a_level(gp):
    assert gp.DIST_DIGIT_BITS == 13 and gp.dist_level_bits() == [12, 13, 13, 13, 13]
    assert gp.dist_boundaries() == [12, 25, 38, 51, 64]


def test_quantile_ranks(gp):
    assert gp.quantile_ranks(10, [0.0, 1.0, 0.5, 0.99, 0.1, 0.11, 0.12]) == [0, 9, 4, 8, 0, 0, 1]
    assert gp.quantile_ranks(1, [0.0, 0.3, 1.0]) == [0, 0, 0]
    for n in (2, 7, 1000, 123457):
        q = np.random.default_rng(n).random(50).tolist() + [0.0, 1.0]
        assert gp.quantile_ranks(n, q) == DR.quantile_ranks(n, q)
        assert all(0 <= r <= n - 1 for r in gp.quantile_ranks(n, q))


class StandIn:
    """the two callables of the search over an array the test holds; NaN: unscored"""

    def __init__(self, gp, scores, B):
        self.keys = np.sort(DR.key(DR.scored(scores)))
        self.bits = gp.dist_level_bits(B)
        self.bounds = gp.dist_boundaries(B)
        self.calls = []

    def hist(self, prefixes, prefix_bits):
        self.calls.append(("hist", prefix_bits, len(prefixes)))
        level = 0 if prefix_bits == 0 else self.bounds.index(prefix_bits) + 1
        bits = self.bits[level]
        digit = ((self.keys >> np.uint64(64 - prefix_bits - bits)) & np.uint64((1 << bits) - 1)).astype(np.int64)
        if prefix_bits == 0:
            assert len(prefixes) == 0
            return np.bincount(digit, minlength=1 << bits)[None, :]
        assert 1 <= len(prefixes) <= 64 and (np.diff(prefixes.astype(object)) > 0).all()
        top = self.keys >> np.uint64(64 - prefix_bits)
        return np.stack([np.bincount(digit[top == p], minlength=1 << bits) for p in prefixes])

    def collect(self, prefixes, prefix_bits, total):
        self.calls.append(("collect", prefix_bits, len(prefixes)))
        assert prefix_bits in self.bounds[:-1]
        got = self.keys[np.isin(self.keys >> np.uint64(64 - prefix_bits), prefixes)]
        assert len(got) == total
        return np.random.default_rng(3).permutation(DR.unkey(got))         # (the order is not part of the contract)


def _select(gp, scores, ranks, cap, B=13):
    s = StandIn(gp, scores, B)
    seen = []
    n, r, values, passes = gp.select_order_statistics(s.hist, s.collect, lambda n: ranks(n) if callable(ranks) else ranks,
                                                      collect_cap=cap, digit_bits=B, on_pass=seen.append)
    assert n == len(s.keys) and seen == passes
    assert [(p["kind"], p["prefix_bits"], p["targets"]) for p in passes] == s.calls
    assert len(passes) <= len(s.bits) + 1
    assert DR.same_bits(values, DR.order_statistics(scores, r)), (cap, B)
    return r, values, passes


@pytest.mark.parametrize("cap", [1, 7, 1 << 20])
def test_search_on_random_normals(gp, cap):
    x = np.random.default_rng(5).standard_normal(10000)
    x[::97] = NAN
    n = int((~np.isnan(x)).sum())
    ranks = [n // 2, 0, n - 1, 17, 17, n - 2, 5000, 1, n // 2]             # duplicates, unsorted, both ends
    for B in (13, 8, 11, 16):
        _, _, passes = _select(gp, x, ranks, cap, B)
        kinds = [p["kind"] for p in passes]
        if cap == 1 << 20:
            assert kinds == ["hist", "collect"]                            # everything fits after the first level
        elif cap == 7:                                                     # 7 distinct ranks: collected once each stands alone
            assert kinds[-1] == "collect" and kinds.count("collect") == 1 and len(kinds) >= 3
        else:                                                              # 7 targets never fit a cap of 1: every level
            assert kinds == ["hist"] * len(gp.dist_level_bits(B))
    q = [0.5, 0.0, 1.0, 0.99, 0.01, 0.5]
    r, values, _ = _select(gp, x, lambda n: gp.quantile_ranks(n, q), cap)
    assert r.tolist() == DR.quantile_ranks(n, q) and values[0] == values[5] and values[1] == np.nanmin(x)


@pytest.mark.parametrize("cap", [1, 7, 1 << 20])
def test_search_on_one_repeated_value(gp, cap):
    for value in (0.3, -0.0, -INF, 5e-324):
        x = np.full(1000, value)
        _, values, passes = _select(gp, x, [0, 999, 500, 500], cap)
        assert DR.same_bits(values, np.full(4, value))
        kinds = [p["kind"] for p in passes]
        if cap < 1000:
            assert kinds == ["hist"] * 5 and passes[-1]["prefix_bits"] == 51   # every level, then the prefix is the key
            assert all(p["targets"] == (1 if i else 0) for i, p in enumerate(passes))
        else:
            assert kinds == ["hist", "collect"]


@pytest.mark.parametrize("cap", [1, 7, 1 << 20])
def test_search_on_values_that_differ_in_the_last_bit(gp, cap):
    for base in (1.0, -1.0):
        x = np.where(np.random.default_rng(6).random(777) < 0.5, base, np.nextafter(base, 2 * base))
        lower = int((DR.key(x) == DR.key(x).min()).sum())
        assert 300 < lower < 477
        _, values, passes = _select(gp, x, [0, lower - 1, lower, 776, lower], cap)
        assert len(set(values.tolist())) == 2 and values[1] != values[2]
        if cap < 300:
            assert [p["kind"] for p in passes] == ["hist"] * 5 and passes[-1]["targets"] == 1
    # one value apart from the rest: the targets part ways at the first level and are refined in lockstep
    x = np.concatenate([np.full(50, -3.5), np.full(60, 2.25), [7.0]])
    _, values, passes = _select(gp, x, [110, 0, 49, 50, 109], 10)
    assert values.tolist() == [7.0, -3.5, -3.5, 2.25, 2.25] and passes[1]["targets"] == 3


def test_search_refusals(gp):
    s = StandIn(gp, np.arange(10.0), 13)
    _, want = gp.check_scan_quantiles(_table(gp), 20, 1, ranks=[0, 10])
    with pytest.raises(gp.ModelError, match="0..n-1; 10 windows"):
        gp.select_order_statistics(s.hist, s.collect, want)
    empty = StandIn(gp, np.full(5, NAN), 13)
    _, want = gp.check_scan_quantiles(_table(gp), 20, 1, q=[0.5])
    with pytest.raises(gp.ModelError, match="no window has a score"):
        gp.select_order_statistics(empty.hist, empty.collect, want)
    assert empty.calls == [("hist", 0, 0)]


def test_library_refusals(gp):
    tab = _table(gp)
    panel = gp.LmerPanel([tab, _table(gp, seed=2)], ["a", "b"])
    x = [np.zeros(40, dtype=np.uint8)]
    scan = [(dict(width=4), "below L"), (dict(width=2048), "above 2047"), (dict(width=20, stride=0), "stride"),
            (dict(width=20, chunk=10), "chunk")]
    tail = scan + [(dict(width=20), "1..4096 thresholds"), (dict(width=20, thresholds=[]), "1..4096 thresholds"),
                   (dict(width=20, thresholds=np.zeros(4097)), "1..4096 thresholds per call, not 4097"),
                   (dict(width=20, thresholds=[0.0, NAN]), "a threshold is NaN"),
                   (dict(width=20, thresholds=["high"]), "must be a number"),
                   (dict(width=41, thresholds=[0.0]), "no record holds a window")]
    quant = [(dict(kw, q=[0.5]), msg) for kw, msg in scan] + [
        (dict(width=20), "either q or ranks"), (dict(width=20, q=[0.5], ranks=[1]), "either q or ranks"),
        (dict(width=20, q=[]), "1..64 quantiles"), (dict(width=20, q=[0.5] * 65), "1..64 quantiles per call, not 65"),
        (dict(width=20, ranks=list(range(65))), "1..64 ranks"), (dict(width=20, q=[0.5, NAN]), "0..1"),
        (dict(width=20, q=[-0.01]), "0..1"), (dict(width=20, q=[1.0000001]), "0..1"), (dict(width=20, q=["x"]), "number"),
        (dict(width=20, ranks=[-1]), "0..n-1"), (dict(width=20, ranks=[1.5]), "integer"),
        (dict(width=20, ranks=[True]), "integer"), (dict(width=20, q=[0.5], collect_cap=0), "collect_cap"),
        (dict(width=20, q=[0.5], collect_cap=2.5), "collect_cap"), (dict(width=41, q=[0.5]), "no record holds a window")]
    for cases, single, multi, check, pcheck in (
            (tail, gp.scan_tail_counts, gp.scan_tail_counts_with_panel, gp.check_scan_tail_counts,
             gp.check_panel_scan_tail_counts),
            (quant, gp.scan_quantiles, gp.scan_quantiles_with_panel, gp.check_scan_quantiles, gp.check_panel_scan_quantiles)):
        for kw, msg in cases:
            with pytest.raises(gp.ModelError, match=msg):
                single(tab, x, **kw)
            with pytest.raises(gp.ModelError, match=msg):
                multi(panel, x, **kw)
            if "no record" not in msg:
                for fn, folded in ((check, tab), (pcheck, panel)):
                    with pytest.raises(gp.ModelError, match=msg):
                        fn(folded, **dict(dict(stride=1), **kw))
        with pytest.raises(gp.ModelError, match="not a model"):
            single(panel, x, width=20)
        with pytest.raises(gp.ModelError, match="panel"):
            multi(tab, x, width=20)
    got = gp.check_scan_tail_counts(tab, 20, 1, [1.0, -INF, INF, 1.0, -0.0])
    assert got.dtype == np.float64 and DR.same_bits(got, [1.0, -INF, INF, 1.0, -0.0])
    assert gp.check_scan_tail_counts(tab, 20, 1, 0.5).tolist() == [0.5]
    qs, want = gp.check_panel_scan_quantiles(panel, 20, 1, q=(1.0, 0.0, 0.5))
    assert qs == [1.0, 0.0, 0.5] and want(11) == [10, 0, 5]
    qs, want = gp.check_scan_quantiles(tab, 20, 1, ranks=np.array([3, 0, 3]))
    assert qs is None and want(4) == [3, 0, 3]


def test_files_round_trip_bit_for_bit(gp, tmp_path):
    path = str(tmp_path / "o.tsv")
    values = np.array([0.1, -0.0, 1 / 3, -INF, INF, 5e-324, -HUGE, np.nextafter(1.0, 2.0)])
    tail = dict(scored=12345678901, unscored=7, thresholds=values, counts=np.arange(8, dtype=np.int64) * 3000000000)
    gp.write_tail_counts(path, tail)
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "#scored\t12345678901\tunscored\t7" and lines[1] == "%.17g\t0" % 0.1 and len(lines) == 10
    back = gp.read_tail_counts(path)
    assert (back["scored"], back["unscored"]) == (12345678901, 7) and DR.same_bits(back["thresholds"], values)
    assert back["counts"].dtype == np.int64 and np.array_equal(back["counts"], tail["counts"])
    for q in ([0.5, 0.0, 1.0, 0.99, 0.01, 0.5, 1 / 3, 0.1], None):
        quant = dict(scored=9, unscored=0, q=q, ranks=np.arange(8, dtype=np.int64), values=values, passes=[])
        gp.write_quantiles(path, quant)
        back = gp.read_quantiles(path)
        assert (back["scored"], back["unscored"], back["q"]) == (9, 0, q)
        assert np.array_equal(back["ranks"], quant["ranks"]) and DR.same_bits(back["values"], values)
    with open(path) as f:
        assert f.read().split("\n")[1] == "-\t0\t%.17g" % 0.1
    # panels: the member's name in front
    names = ["wgkm", "gkm"]
    ptail = dict(scored=np.array([5, 4]), unscored=np.array([0, 1]), thresholds=values[:3],
                 counts=np.array([[5, 3, 1], [4, 4, 0]]))
    gp.write_panel_tail_counts(path, names, ptail)
    heads, rows = gp.read_panel_tail_counts(path)
    assert heads == [("wgkm", 5, 0), ("gkm", 4, 1)]
    assert [r[0] for r in rows] == ["wgkm"] * 3 + ["gkm"] * 3 and [r[2] for r in rows] == [5, 3, 1, 4, 4, 0]
    assert DR.same_bits([r[1] for r in rows], np.tile(values[:3], 2))
    pquant = dict(scored=np.array([5, 4]), unscored=np.array([0, 1]), q=[0.5, 1.0], ranks=np.array([[2, 4], [1, 3]]),
                  values=np.stack([values[:2], values[2:4]]))
    gp.write_panel_quantiles(path, names, pquant)
    heads, rows = gp.read_panel_quantiles(path)
    assert heads == [("wgkm", 5, 0), ("gkm", 4, 1)]
    assert [r[:3] for r in rows] == [("wgkm", 0.5, 2), ("wgkm", 1.0, 4), ("gkm", 0.5, 1), ("gkm", 1.0, 3)]
    assert DR.same_bits([r[3] for r in rows], values[:4])


def test_command_line_refusals_exit_1_and_write_nothing(gp, tmp_path, capsys):
    tab = _table(gp)
    weights, fa, out = str(tmp_path / "w.txt"), str(tmp_path / "s.fa"), str(tmp_path / "o.tsv")
    pfile = str(tmp_path / "p.npz")
    tab.save(weights)
    gp.LmerPanel([tab, _table(gp, seed=2)], ["a", "b"]).save(pfile)
    with open(fa, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n")
    cases = []
    for suffix, folded in (("", weights), ("-panel", pfile)):
        t, q = "scan-tail" + suffix, "scan-quantiles" + suffix
        cases += [(t, ["--width", "4", "--thresholds", "0", folded, fa, out], "below L"),
                  (t, ["--width", "20", "--stride", "0", "--thresholds", "0", folded, fa, out], "stride"),
                  (t, ["--width", "20", "--chunk", "10", "--thresholds", "0", folded, fa, out], "chunk"),
                  (t, ["--width", "20", folded, fa, out], "1..4096 thresholds"),
                  (t, ["--width", "20", "--thresholds", ",".join(["1"] * 4097), folded, fa, out], "not 4097"),
                  (t, ["--width", "20", "--thresholds", "1,nan", folded, fa, out], "a threshold is NaN"),
                  (t, ["--width", "20", "--thresholds", "1,high", folded, fa, out], "no comma-separated list of numbers"),
                  (t, ["--width", "41", "--thresholds", "0", folded, fa, out], "no record holds a window"),
                  (t, ["--width", "20", "--thresholds", "0", folded, str(tmp_path / "missing.fa"), out], "cannot read"),
                  (t, ["--width", "20", "--thresholds", "0", str(tmp_path / "missing.txt"), fa, out], "missing.txt"),
                  (q, ["--width", "4", "--q", "0.5", folded, fa, out], "below L"),
                  (q, ["--width", "20", folded, fa, out], "either q or ranks"),
                  (q, ["--width", "20", "--q", "0.5", "--ranks", "1", folded, fa, out], "either q or ranks"),
                  (q, ["--width", "20", "--q", "", folded, fa, out], "1..64 quantiles"),
                  (q, ["--width", "20", "--q", ",".join(["0.5"] * 65), folded, fa, out], "not 65"),
                  (q, ["--width", "20", "--q", "0.5,nan", folded, fa, out], "0..1"),
                  (q, ["--width", "20", "--q", "1.5", folded, fa, out], "0..1"),
                  (q, ["--width", "20", "--q", "half", folded, fa, out], "no comma-separated list of numbers"),
                  (q, ["--width", "20", "--ranks", "-1", folded, fa, out], "0..n-1"),
                  (q, ["--width", "20", "--ranks", "1.5", folded, fa, out], "no comma-separated list of integers"),
                  (q, ["--width", "20", "--q", "0.5", "--collect-cap", "0", folded, fa, out], "collect_cap"),
                  (q, ["--width", "41", "--q", "0.5", folded, fa, out], "no record holds a window"),
                  (q, ["--width", "20", "--q", "0.5", folded, str(tmp_path / "missing.fa"), out], "cannot read")]
    cases += [("scan-tail-panel", ["--width", "20", "--thresholds", "0", weights, fa, out], "not a panel file"),
              ("scan-quantiles-panel", ["--width", "20", "--q", "0.5", weights, fa, out], "not a panel file")]
    for cmd, args, msg in cases:
        assert gp.main([cmd] + args) == 1, (cmd, args)
        err = capsys.readouterr().err
        assert err.startswith("gkmpredict: error:") and msg in err, (cmd, args, err)
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    with pytest.raises(SystemExit):
        gp.main(["scan-tail", "--thresholds", "0", weights, fa, out])      # --width is required
    with pytest.raises(SystemExit):
        gp.main(["scan-quantiles", "--width", "20", "--q", "0.5", "--collect-cap", "many", weights, fa, out])
