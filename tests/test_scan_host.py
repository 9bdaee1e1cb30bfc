"""Scanning without a GPU: the CPU reference (tests/scan_ref.py), the stretch formulation against the oracle's self
profiles, window enumeration, the long-sequence reader, the window validity mask, the chunk plan, the output file, and
every refusal of gkmpredict.scan and its command line (gkmqc_amd/gkmpredict.py)."""
import os

import numpy as np
import pytest

from tests import scan_ref as SR


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _table(gp, kernel_type=4, L=5, k=3, d=2, rho=0.125, seed=1):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal(4 ** L)
    u = np.arange(4 ** L, dtype=np.uint32)
    W = W + W[gp.lmer_rc(u, L)]                       # W[u] == W[rc(u)], as a model's table
    return gp.LmerTable(W, kernel_type, L, k, d, 50, 50.0, rho)


@pytest.mark.parametrize("T,W,s,want", [(20, 20, 3, [0]), (22, 20, 3, [0]), (23, 20, 3, [0, 3]), (19, 20, 3, []),
                                        (20, 20, 1, [0]), (25, 20, 1, [0, 1, 2, 3, 4, 5]), (100, 10, 45, [0, 45, 90]),
                                        (0, 5, 1, [])])
def test_window_enumeration_at_the_edges(gp, T, W, s, want):
    """T = W, T = W + s - 1 (one window), T = W + s (two), T < W (none)"""
    assert SR.starts(T, W, s) == want
    assert gp.scan_window_count(T, W, s) == len(want)
    assert [a for a, _ in SR.windows(np.zeros(T, np.uint8), W, s)] == want
    assert all(len(w) == W for _, w in SR.windows(np.zeros(T, np.uint8), W, s))


def test_reader_keeps_long_records_whole_and_marks_invalid_bases(gp, tmp_path):
    rng = np.random.default_rng(4)
    long_codes = rng.integers(0, 4, size=10000, dtype=np.uint8)
    text = gp.codes_to_text(long_codes)
    path = str(tmp_path / "x.fa")
    with open(path, "w") as f:
        f.write("not a record\n")
        f.write(">chrA some description\nACGTacgt\nNNNNac\n\nRYgt\n")
        f.write(">long\n" + "\n".join(text[i:i + 70] for i in range(0, len(text), 70)) + "\n")
        f.write(">crlf\r\nAC\r\nGT\r\n")
        f.write(">empty\n")
        f.write(">last no newline\nTTTT")
    recs = gp.read_long_fasta(path)
    assert [r[0] for r in recs] == ["chrA some description", "long", "crlf", "empty", "last no newline"]
    name, codes, valid = recs[0]
    assert codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 0, 0, 0, 0, 1, 0, 0, 2, 3]
    assert valid.tolist() == [True] * 8 + [False] * 4 + [True, True, False, False, True, True]
    assert codes.dtype == np.uint8 and valid.dtype == np.bool_
    assert len(recs[1][1]) == 10000 and np.array_equal(recs[1][1], long_codes) and recs[1][2].all()
    assert recs[2][1].tolist() == [0, 1, 2, 3] and recs[2][2].all()
    assert len(recs[3][1]) == 0
    assert recs[4][1].tolist() == [3, 3, 3, 3]


def test_code_arrays_take_values_from_four_up_as_invalid(gp):
    from gkmqc_amd import gkmscan
    recs = gkmscan._as_scan_records([np.array([0, 3, 4, 255, 2], dtype=np.uint8), [1, 1]])
    assert [r[0] for r in recs] == ["seq0", "seq1"]
    assert recs[0][1].tolist() == [0, 3, 0, 0, 2] and recs[0][2].tolist() == [True, True, False, False, True]
    assert recs[1][2].all()


@pytest.mark.parametrize("W,s", [(5, 1), (5, 3), (12, 7), (40, 40), (40, 43), (200, 1)])
def test_window_validity_against_a_plain_loop(gp, W, s):
    rng = np.random.default_rng(W + s)
    x = rng.integers(0, 4, size=300, dtype=np.uint8)
    x[[0, 17, 18, 19, 150, 299]] = 4
    x[60:75] = 9
    got = gp.window_validity(x < 4, W, s)
    assert got.tolist() == SR.valid_windows(x, W, s)
    assert got.dtype == np.bool_
    assert gp.window_validity(np.ones(W - 1, bool), W, s).shape == (0,)


@pytest.mark.parametrize("T,W,s", [(1000, 60, 1), (1000, 60, 7), (1000, 60, 60), (1000, 60, 63), (61, 60, 1), (60, 60, 5),
                                   (5000, 600, 10)])
@pytest.mark.parametrize("chunk", [1, 64, 100, 601, 999, 10 ** 6])
def test_chunk_plan_covers_every_window_exactly_once(gp, T, W, s, chunk):
    plan = gp.scan_chunk_plan(T, W, s, chunk)
    nw = gp.scan_window_count(T, W, s)
    seen = np.zeros(nw, dtype=np.int64)
    for w0, w1, b0, b1 in plan:
        assert 0 <= w0 < w1 <= nw
        seen[w0:w1] += 1
        assert b0 == w0 * s and b1 == (w1 - 1) * s + W and b1 <= T      # the chunk's bases hold exactly its windows
        assert b1 - b0 <= max(chunk, W)
    assert (seen == 1).all()
    assert [p[0] for p in plan] == sorted(p[0] for p in plan)
    if chunk >= T:
        assert len(plan) == 1
    if s == 1 and len(plan) > 1:
        assert plan[0][3] - plan[1][2] == W - 1                           # consecutive chunks overlap by W - 1 bases
    assert gp.scan_chunk_plan(W - 1, W, s, chunk) == []


def test_default_chunk_fits_the_device_budget(gp):
    for d in (0, 3, 12):
        b = gp.default_scan_chunk(d)
        assert b >= 1 << 20 and b * (8 * (d + 1) + 64) <= gp.BLOCK_BYTES


@pytest.mark.parametrize("t,L,k,d", [(0, 5, 3, 2), (4, 5, 3, 2), (4, 6, 3, 3), (2, 6, 4, 1)])
@pytest.mark.parametrize("W,s,g", [(5, 1, 4), (6, 1, 64), (20, 1, 5), (20, 3, 4), (20, 3, 1), (20, 20, 3), (20, 23, 2),
                                   (33, 2, 16)])
def test_stretch_formulation_equals_the_oracle_self_profiles(built, t, L, k, d, W, s, g):
    """every l-mer pair of a stretch compared once per strand and credited to the windows that hold it = the oracle's
    P_m(w, w) of every window cut out; with one window per stretch it compares n^2 + n pairs, half of window by window"""
    W = max(W, L)
    rng = np.random.default_rng(W + s + L)
    x = rng.integers(0, 4, size=90, dtype=np.uint8)
    x[30:48] = 0                                                           # a homopolymer stretch: dense hits
    x[60:70] = np.tile([0, 3], 5)                                          # (AT)n: reverse-complement hits
    got, comparisons = SR.stretch_profiles(x, W, s, g, t, L, d)
    want = SR.profiles(x, W, s, t, L, k, d)
    assert got.shape == want.shape and len(want) == len(SR.starts(90, W, s))
    assert np.array_equal(got, want)
    n = W - L + 1
    if g == 1:
        assert comparisons == (n * n + n) * len(want)


def test_reference_scores_follow_the_definition(gp):
    from tests import explain_ref as R
    from tests import lmer_ref as LR
    tab = _table(gp)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 4, size=60, dtype=np.uint8)
    x[25] = 4
    res = SR.scores(tab, x, 12, 5)
    assert [a for a, _ in res] == list(range(0, 49, 5))
    for a, v in res:
        if a <= 25 < a + 12:
            assert np.isnan(v)
        else:
            w = x[a:a + 12]
            assert v == LR.table_score(tab, tab.W, w) / R.self_norm(w, 4, 5, 3, 2) + tab.rho


def test_output_file_round_trip(gp, tmp_path):
    rng = np.random.default_rng(9)
    s0 = rng.standard_normal(7) * 10.0 ** rng.integers(-8, 8, size=7)
    s0[[2, 3]] = np.nan
    s1 = np.array([np.pi, -0.0, 5e-324])
    results = [("chr1 with\ttab", np.arange(7, dtype=np.int64) * 10, s0), ("none", np.zeros(0, np.int64), np.zeros(0)),
               ("chr2", np.arange(3, dtype=np.int64), s1)]
    path = str(tmp_path / "o.bedgraph")
    assert gp.write_scan(path, results, 600) == 2
    back = gp.read_scan(path)
    want = [("chr1 with\ttab", 10 * i, 10 * i + 600, s0[i]) for i in (0, 1, 4, 5, 6)]
    want += [("chr2", i, i + 600, s1[i]) for i in range(3)]
    assert len(back) == len(want)
    for b, w in zip(back, want):
        assert b[:3] == w[:3] and np.float64(b[3]).tobytes() == np.float64(w[3]).tobytes()
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "chr1 with\ttab\t0\t600\t%.17g" % s0[0]


def test_api_refusals_come_before_any_device_work(gp):
    """(no GPU here: anything that reached the device would fail otherwise)"""
    tab = _table(gp)
    x = [np.zeros(100, dtype=np.uint8)]
    for kw, msg in ((dict(width=4), "below L"), (dict(width=2048), "above 2047"), (dict(width=20, stride=0), "stride"),
                    (dict(width=20, stride=-3), "stride"), (dict(width=20, chunk=19), "chunk"),
                    (dict(width=101), "no record holds a window")):
        with pytest.raises(gp.ModelError, match=msg):
            gp.scan(tab, x, **kw)
    with pytest.raises(gp.ModelError, match="no record holds a window"):
        gp.scan(tab, [], 20)
    rbf = _table(gp)
    rbf.kernel_type = 5
    with pytest.raises(gp.ModelError, match="RBF"):
        gp.scan(rbf, x, 20)
    with pytest.raises(gp.ModelError, match="RBF"):
        gp.LmerTable(tab.W, 3, 5, 3, 2, 50, 50.0, 0.0)
    model = gp.Model(4, 5, 3, 2, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.0, 1, [1.0, 1.0], ["a", "b"],
                     [np.zeros(9, np.uint8), np.ones(9, np.uint8)])
    with pytest.raises(gp.ModelError, match="weight table"):
        gp.scan(model, x, 20)


def test_command_line_refusals_exit_1_and_write_nothing(gp, tmp_path, capsys):
    tab = _table(gp)
    weights, fa, out = str(tmp_path / "w.txt"), str(tmp_path / "s.fa"), str(tmp_path / "o.bedgraph")
    tab.save(weights)
    with open(fa, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n")
    bad_weights = str(tmp_path / "bad.txt")
    with open(bad_weights, "w") as f:
        f.write(open(weights).read().replace("kernel_type 4", "kernel_type 5"))
    cases = [(["--width", "4", fa, weights, out], "below L"),
             (["--width", "2048", fa, weights, out], "above 2047"),
             (["--width", "20", "--stride", "0", fa, weights, out], "stride"),
             (["--width", "20", "--chunk", "10", fa, weights, out], "chunk"),
             (["--width", "41", fa, weights, out], "no record holds a window"),
             (["--width", "20", str(tmp_path / "missing.fa"), weights, out], "cannot read"),
             (["--width", "20", fa, str(tmp_path / "missing.txt"), out], "missing.txt"),
             (["--width", "20", fa, bad_weights, out], "RBF")]
    for args, msg in cases:
        assert gp.main(["scan"] + args) == 1, args
        assert msg in capsys.readouterr().err, args
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    with pytest.raises(SystemExit):
        gp.main(["scan", fa, weights, out])                                # --width is required
