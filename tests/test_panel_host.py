"""L-mer weight panels without a GPU (gkmqc_amd/gkmpredict.py): construction and every refusal of
LmerPanel, the device image, the panel file and each malformed-file refusal, the refusals of the panel functions and of
the four subcommands, and the scan chunk formula."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


PARAMS = dict(kernel_type=4, L=5, k=3, d=2, M=50, H=50.0)


def _table(gp, seed=1, rho=None, **over):
    p = dict(PARAMS, **over)
    L = p["L"]
    W = np.random.default_rng(seed).standard_normal(4 ** L)
    W = W + W[gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)]
    return gp.LmerTable(W, p["kernel_type"], L, p["k"], p["d"], p["M"], p["H"], 0.125 * seed if rho is None else rho)


def _tables(gp, n):
    return [_table(gp, seed=s + 1) for s in range(n)]


def test_construction(gp):
    tables = _tables(gp, 3)
    panel = gp.LmerPanel(tables)
    assert panel.n_models == 3 and panel.names == ["table0", "table1", "table2"]
    assert panel.W.shape == (4 ** 5, 3) and panel.W.dtype == np.float64 and panel.W.flags["C_CONTIGUOUS"]
    assert panel.rho.shape == (3,) and panel.rho.tolist() == [0.125, 0.25, 0.375]
    for m, t in enumerate(tables):
        assert panel.W[:, m].tobytes() == t.W.tobytes()
        assert panel.table(m).W.tobytes() == t.W.tobytes() and panel.table(m).rho == t.rho
    assert (panel.kernel_type, panel.L, panel.k, panel.d, panel.M, panel.H) == (4, 5, 3, 2, 50, 50.0)
    assert panel.kernel_params() == tables[0].kernel_params()
    rc = gp.lmer_rc(np.arange(4 ** 5, dtype=np.uint32), 5)
    assert panel.W[rc].tobytes() == panel.W.tobytes()
    named = gp.LmerPanel(tables, names=["a", "b c", "d.txt"])
    assert named.names == ["a", "b c", "d.txt"]
    assert gp.LmerPanel(_tables(gp, 64)).n_models == 64


@pytest.mark.parametrize("key,value", [("kernel_type", 2), ("L", 6), ("k", 4), ("d", 1), ("M", 40), ("H", 25.0)])
def test_members_must_share_every_parameter(gp, key, value):
    over = {key: value}
    if key == "L":
        over.update(k=4)                                                   # (k = L - d stays a valid combination)
    if key == "k":
        over.update(d=1)
    odd = _table(gp, seed=9, **over)
    with pytest.raises(gp.ModelError) as e:
        gp.LmerPanel([_table(gp), _table(gp, seed=2), odd], names=["x", "y", "odd"])
    assert "member 2 (odd) has %s = %r" % (key, value) in str(e.value)


def test_first_differing_key_is_named(gp):
    """k and d both differ: k comes first in (kernel_type, L, k, d, M, H)"""
    with pytest.raises(gp.ModelError, match=r"member 1 \(table1\) has k = 4"):
        gp.LmerPanel([_table(gp), _table(gp, k=4, d=1)])


def test_member_count_and_name_refusals(gp):
    with pytest.raises(gp.ModelError, match="0 members"):
        gp.LmerPanel([])
    with pytest.raises(gp.ModelError, match="65 members"):
        gp.LmerPanel([_table(gp)] * 65)
    two = _tables(gp, 2)
    with pytest.raises(gp.ModelError, match="given to members 0 and 1"):
        gp.LmerPanel(two, names=["a", "a"])
    for bad in ("", "a\tb", "a\nb", 7, None):
        with pytest.raises(gp.ModelError, match="name of member 1"):
            gp.LmerPanel(two, names=["a", bad])
    with pytest.raises(gp.ModelError, match="1 names for 2 members"):
        gp.LmerPanel(two, names=["a"])
    with pytest.raises(gp.ModelError, match="member 1 is no l-mer weight table"):
        gp.LmerPanel([two[0], object()])


def test_an_rbf_table_is_refused(gp):
    with pytest.raises(gp.ModelError, match="RBF"):
        _table(gp, kernel_type=3)
    rbf = _table(gp, kernel_type=2)
    rbf.kernel_type = 3                                                    # (no constructor hands one out)
    with pytest.raises(gp.ModelError, match="RBF"):
        gp.LmerPanel([rbf])
    with pytest.raises(gp.ModelError, match="RBF"):
        gp.LmerPanel([_table(gp, kernel_type=2), rbf])


def test_size_limit_is_checked_before_any_allocation(gp, monkeypatch):
    tables = _tables(gp, 9)
    assert gp.PANEL_MAX_BYTES >= 4 ** 12 * 64 * 8
    from gkmqc_amd import gkmtables
    monkeypatch.setattr(gkmtables, "PANEL_MAX_BYTES", 4 ** 5 * 16 * 8)
    assert gp.LmerPanel(tables).n_models == 9                              # ms = 16: exactly the limit
    monkeypatch.setattr(gkmtables, "PANEL_MAX_BYTES", 4 ** 5 * 16 * 8 - 1)
    stacked = []
    monkeypatch.setattr(gp.np, "stack", lambda *a, **k: stacked.append(1))
    with pytest.raises(gp.ModelError, match="PANEL_MAX_BYTES"):
        gp.LmerPanel(tables)
    assert not stacked


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64])
def test_device_rows(gp, n):
    panel = gp.LmerPanel(_tables(gp, n))
    P = panel.device_rows()
    ms = (n + 7) // 8 * 8
    assert gp.panel_row_stride(n) == ms and ms % 8 == 0 and ms >= n
    assert P.shape == (4 ** 5, ms) and P.dtype == np.float64 and P.flags["C_CONTIGUOUS"]
    assert P[:, :n].tobytes() == panel.W.tobytes()
    assert not P[:, n:].any() and not np.signbit(P[:, n:]).any()


def test_save_and_load_round_trip(gp, tmp_path):
    path = str(tmp_path / "p.npz")
    panel = gp.LmerPanel(_tables(gp, 9), names=["m%d" % i for i in range(9)])
    panel.save(path)
    assert not os.path.exists(path + ".tmp")
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["format", "kernel_type", "L", "k", "d", "M", "H", "names", "rho", "W"])
        assert str(z["format"]) == "gkmqc-lmer-panel-1" == gp.PANEL_FORMAT
        assert z["W"].shape == (len(gp.canonical_codes(5)), 9)
        assert z["W"].tobytes() == panel.W[gp.canonical_codes(5)].tobytes()
    back = gp.load_lmer_panel(path)
    assert back.names == panel.names and back.n_models == 9
    assert back.W.tobytes() == panel.W.tobytes() and back.rho.tobytes() == panel.rho.tobytes()
    assert back.W.flags["C_CONTIGUOUS"] and back.kernel_params() == panel.kernel_params()


def _saved(gp, tmp_path, **change):
    """a good panel file with some members replaced or removed (value None)"""
    panel = gp.LmerPanel(_tables(gp, 3), names=["a", "b", "c"])
    good = str(tmp_path / "good.npz")
    panel.save(good)
    with np.load(good, allow_pickle=False) as z:
        got = {key: z[key] for key in z.files}
    for key, value in change.items():
        if value is None:
            del got[key]
        else:
            got[key] = value
    path = str(tmp_path / "bad.npz")
    with open(path, "wb") as f:
        np.savez(f, **got)
    return path


MALFORMED = [
    (dict(format=np.array("gkmqc-lmer-panel-2")), "format"),
    (dict(format=np.array("gkmqc-lmer-importance-1")), "format"),
    (dict(rho=None), "missing key"),
    (dict(names=None), "missing key"),
    (dict(W=None), "missing key"),
    (dict(H=None), "missing key"),
    (dict(extra=np.zeros(1)), "do not belong"),
    (dict(W=np.zeros((10, 3))), "W is"),
    (dict(W=np.zeros((512, 2))), "W is"),
    (dict(W=np.zeros((512, 3), dtype=np.float32)), "W is"),
    (dict(rho=np.zeros(2)), "rho is"),
    (dict(rho=np.array([0.0, np.nan, 0.0])), "rho of member 1 is not finite"),
    (dict(rho=np.array([0.0, 0.0, np.inf])), "rho of member 2 is not finite"),
    (dict(names=np.array(["a", "b", "a"])), "given to members 0 and 2"),
    (dict(names=np.array(["a", "", "c"])), "name of member 1"),
    (dict(names=np.array([1, 2, 3])), "names is"),
    (dict(L=np.float64(5.0)), "L must be one integer"),
    (dict(kernel_type=np.int64(3)), "RBF"),
    (dict(kernel_type=np.int64(9)), "rejected"),
]


@pytest.mark.parametrize("change,reason", MALFORMED, ids=[r + str(i) for i, (_, r) in enumerate(MALFORMED)])
def test_malformed_panel_files(gp, tmp_path, change, reason):
    assert len(gp.canonical_codes(5)) == 512
    path = _saved(gp, tmp_path, **change)
    with pytest.raises(gp.ModelError) as e:
        gp.load_lmer_panel(path)
    assert reason in str(e.value) and path in str(e.value)


def test_files_that_are_no_panel(gp, tmp_path):
    text = str(tmp_path / "w.txt")
    _table(gp).save(text)
    with pytest.raises(gp.ModelError, match="not a panel file"):
        gp.load_lmer_panel(text)
    pickled = str(tmp_path / "o.npz")
    with open(pickled, "wb") as f:
        np.savez(f, format=np.array([{"a": 1}], dtype=object))
    with pytest.raises(gp.ModelError, match="not a panel file"):
        gp.load_lmer_panel(pickled)
    many = _saved(gp, tmp_path, names=np.array(["n%d" % i for i in range(65)]), rho=np.zeros(65), W=np.zeros((512, 65)))
    with pytest.raises(gp.ModelError, match="65 members"):
        gp.load_lmer_panel(many)


def test_default_panel_scan_chunk(gp):
    seen = []
    for d in (0, 3, 12):
        for n in (1, 8, 20, 64):
            want = gp.BLOCK_BYTES // (8 * (d + 1) + 64 + 8 * n)
            assert gp.default_panel_scan_chunk(d, n) == want
            assert gp.default_panel_scan_chunk(d, n, budget=1 << 20) == (1 << 20) // (8 * (d + 1) + 64 + 8 * n)
            assert gp.default_panel_scan_chunk(d, n) < gp.default_scan_chunk(d)
            seen.append(want)
        assert seen[-4] > seen[-3] > seen[-2] > seen[-1]


def test_api_refuses_before_it_touches_the_device(gp):
    """a table or a model where a panel is needed, and the single-table functions' own refusals, without a GPU"""
    table = _table(gp)
    panel = gp.LmerPanel(_tables(gp, 2))
    x = np.array([0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3], dtype=np.uint8)           # ACGTTGCAACGT
    for what in (table, object()):
        with pytest.raises(gp.ModelError, match="needs an l-mer weight panel"):
            gp.score_with_panel(what, [x])
        with pytest.raises(gp.ModelError, match="needs an l-mer weight panel"):
            gp.scan_with_panel(what, [x], 8)
        with pytest.raises(gp.ModelError, match="needs an l-mer weight panel"):
            gp.delta_with_panel(what, [x], [(0, 0, "A", "C")])
        with pytest.raises(gp.ModelError, match="needs an l-mer weight panel"):
            gp.delta_saturation_with_panel(what, [x])
    with pytest.raises(gp.ModelError, match="no query sequences"):
        gp.score_with_panel(panel, [])
    with pytest.raises(gp.ModelError, match="shorter than L"):
        gp.score_with_panel(panel, [x, x[:4]])
    with pytest.raises(gp.ModelError, match="below L"):
        gp.scan_with_panel(panel, [x], 4)
    with pytest.raises(gp.ModelError, match="above 2047"):
        gp.scan_with_panel(panel, [x], 2048)
    with pytest.raises(gp.ModelError, match="stride"):
        gp.scan_with_panel(panel, [x], 8, stride=0)
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.scan_with_panel(panel, [x], 8, chunk=7)
    with pytest.raises(gp.ModelError, match="no record holds a window"):
        gp.scan_with_panel(panel, [x], 13)
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.delta_with_panel(panel, [x], [(0, 0, "A", "C")], chunk=100)
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.delta_saturation_with_panel(panel, [x], chunk=100)
    with pytest.raises(gp.ModelError, match="does not match"):
        gp.delta_with_panel(panel, [x], [(0, 0, "C", "A")])
    with pytest.raises(gp.ModelError, match="no such record"):
        gp.delta_with_panel(panel, [x], [("seq1", 0, "A", "C")])
    with pytest.raises(gp.ModelError, match="fewer than L"):
        gp.delta_saturation_with_panel(panel, [x, x[:4]])
    assert gp.delta_with_panel(panel, [x], []).shape == (0, 2)
    with pytest.raises(gp.ModelError, match="needs an l-mer weight table"):
        gp.delta(panel, [x], [(0, 0, "A", "C")])                                  # (and a panel is no table)
    with pytest.raises(gp.ModelError, match="needs an l-mer weight table"):
        gp.scan(panel, [x], 8)


def _refusal(gp, call):
    with pytest.raises(gp.ModelError) as e:
        call()
    return str(e.value)


def test_panel_checks_refuse_what_the_table_checks_refuse(gp):
    """check_panel_scan / check_panel_delta share their bodies with check_scan / check_delta: the same bad argument gives
    the same message behind the prefix.  The texts are written out here, not taken from the code under test."""
    table, panel = _table(gp), gp.LmerPanel(_tables(gp, 2))
    rbf_table, rbf_panel = _table(gp, kernel_type=2), gp.LmerPanel(_tables(gp, 2))
    rbf_table.kernel_type = rbf_panel.kernel_type = 3                      # (no constructor hands one out)
    rbf = "RBF kernels (types 3 and 5) have no l-mer weight table (their score is not linear in the query's l-mers)"
    scans = [((4, 1, None), "the width 4 is below L = 5"),
             ((2048, 1, None), "the width 2048 is above 2047, the longest sequence a score is defined for"),
             ((8, 0, None), "the stride must be at least 1"),
             ((8, 1, 7), "a chunk must hold at least one window (8 bases)")]
    for args, text in scans:
        assert _refusal(gp, lambda: gp.check_scan(table, *args)) == "scan: " + text
        assert _refusal(gp, lambda: gp.check_panel_scan(panel, *args)) == "scan-panel: " + text
    assert _refusal(gp, lambda: gp.check_scan(rbf_table, 8, 1)) == "scan: " + rbf
    assert _refusal(gp, lambda: gp.check_panel_scan(rbf_panel, 8, 1)) == "scan-panel: " + rbf
    assert gp.delta_min_chunk(5) == 264
    chunk = "a chunk must hold a variant's context (at least 264 bases for L = 5)"
    assert _refusal(gp, lambda: gp.check_delta(table, chunk=263)) == "delta: " + chunk
    assert _refusal(gp, lambda: gp.check_panel_delta(panel, chunk=263)) == "delta-panel: " + chunk
    assert _refusal(gp, lambda: gp.check_delta(rbf_table)) == "delta: " + rbf
    assert _refusal(gp, lambda: gp.check_panel_delta(rbf_panel)) == "delta-panel: " + rbf
    # a bad variant is `delta:`'s on either side
    allele = "delta: variant 0 (0, 0, 'A', 'N'): an allele holds a character other than A, C, G, T"
    assert _refusal(gp, lambda: gp.check_delta(table, variants=[(0, 0, "A", "N")])) == allele
    assert _refusal(gp, lambda: gp.check_panel_delta(panel, variants=[(0, 0, "A", "N")])) == allele
    # the wrong object: each side names what it needs
    for wrong in (object(), panel):
        assert _refusal(gp, lambda: gp.check_scan(wrong, 8, 1)) == \
            "scan: needs an l-mer weight table (gkmpredict weights), not a model"
        assert _refusal(gp, lambda: gp.check_delta(wrong)) == \
            "delta: needs an l-mer weight table (gkmpredict weights), not a model"
    for wrong in (object(), table):
        assert _refusal(gp, lambda: gp.check_panel_scan(wrong, 8, 1)) == \
            "scan-panel: needs an l-mer weight panel (gkmpredict panel), not a table or a model"
        assert _refusal(gp, lambda: gp.check_panel_delta(wrong)) == \
            "delta-panel: needs an l-mer weight panel (gkmpredict panel), not a table or a model"
    # and nothing is refused that was not
    assert gp.check_scan(table, 8, 1, 8) is None and gp.check_panel_scan(panel, 8, 1, 8) is None
    assert gp.check_delta(table, chunk=264) is None and gp.check_panel_delta(panel, chunk=264) is None


def test_panel_output_files_round_trip(gp, tmp_path):
    path = str(tmp_path / "o.tsv")
    names = ["a.txt", "b"]
    v = np.array([[0.1, -2.5e-300], [np.pi, 1e300], [np.nan, np.nan]])
    gp.write_panel_scores(path, names, ["q0", "q 1", "q2"], v)
    assert open(path).read().split("\n")[0] == "#name\ta.txt\tb"
    got = gp.read_panel_output(path, 1)
    assert got[0] == names and got[1] == [("q0",), ("q 1",), ("q2",)]
    assert got[2][:2].tobytes() == v[:2].tobytes() and np.isnan(got[2][2]).all()
    starts = np.array([0, 10, 20], dtype=np.int64)
    assert gp.write_panel_scan(path, names, [("chr", starts, v)], 600) == 1
    assert open(path).read().split("\n")[0] == "#name\tstart\tend\ta.txt\tb"
    got = gp.read_panel_output(path, 3)
    assert got[1] == [("chr", "0", "600"), ("chr", "10", "610")] and got[2].tobytes() == v[:2].tobytes()
    variants = [("chr", 4, "A", "C", "rs1"), ("chr", 9, "", "GG", "rs2"), ("chr", 0, "T", "", "rs3")]
    gp.write_panel_delta(path, names, variants, v)
    assert open(path).read().split("\n")[0] == "#name\tpos\tref\talt\tid\ta.txt\tb"
    got = gp.read_panel_output(path, 5)
    assert got[1] == [("chr", "5", "A", "C", "rs1"), ("chr", "10", ".", "GG", "rs2"), ("chr", "1", "T", ".", "rs3")]
    assert got[2][:2].tobytes() == v[:2].tobytes() and np.isnan(got[2][2]).all()
    gp.write_panel_delta(path, names, [t[:4] for t in variants], v)
    assert open(path).read().split("\n")[0] == "#name\tpos\tref\talt\ta.txt\tb"


def test_command_line_refusals(gp, tmp_path, capsys):
    w1, w2, w6, fa, var, out, pan = (str(tmp_path / n) for n in ("w1.txt", "w2.txt", "w6.txt", "x.fa", "v.tsv", "o.tsv",
                                                                 "p.npz"))
    _table(gp, seed=1).save(w1)
    _table(gp, seed=2).save(w2)
    _table(gp, seed=3, L=6, k=4).save(w6)
    with open(fa, "w") as f:
        f.write(">a\nACGTTGCAACGT\n")
    with open(var, "w") as f:
        f.write("a\t1\tC\tA\n")
    parser = gp.build_parser()
    for argv in (["panel"], ["panel", pan], ["predict-panel", fa, pan], ["scan-panel", fa, pan, out],
                 ["scan-panel", "--width", "x", fa, pan, out], ["delta-panel", fa, var, pan],
                 ["predict-panel", "--block", "x", fa, pan, out], ["delta-panel", "--chunk", "x", fa, var, pan, out]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
    capsys.readouterr()
    a = parser.parse_args(["panel", "--names", "a,b", pan, w1, w2])
    assert (a.output, a.weights, a.names) == (pan, [w1, w2], "a,b")
    assert gp.panel_member_names([w1, "/x/y/z.w"]) == ["w1.txt", "z.w"]
    # panel
    assert gp.main(["panel", pan, w1, w6]) == 1
    assert "member 1 (w6.txt) has L = 6" in capsys.readouterr().err
    assert gp.main(["panel", pan, w1, w1]) == 1                               # the same basename twice
    assert "given to members 0 and 1" in capsys.readouterr().err
    assert gp.main(["panel", "--names", "a", pan, w1, w2]) == 1
    assert gp.main(["panel", "--names", "a,a", pan, w1, w2]) == 1
    assert gp.main(["panel", pan, w1, str(tmp_path / "none.txt")]) == 1
    assert gp.main(["panel", pan] + [w1] * 65) == 1
    assert gp.main(["panel", pan, fa]) == 1                                   # not a weights file
    assert not os.path.exists(pan) and not os.path.exists(pan + ".tmp")
    capsys.readouterr()
    assert gp.main(["panel", pan, w1, w2]) == 0
    panel = gp.load_lmer_panel(pan)
    assert panel.names == ["w1.txt", "w2.txt"] and panel.W[:, 1].tobytes() == gp.load_lmer_table(w2).W.tobytes()
    assert gp.main(["panel", "--names", "x,y z", pan, w1, w2]) == 0 and gp.load_lmer_panel(pan).names == ["x", "y z"]
    # the three that read a panel
    none = str(tmp_path / "none.fa")
    assert gp.main(["predict-panel", none, pan, out]) == 1
    assert gp.main(["predict-panel", "--block", "0", fa, pan, out]) == 1
    assert gp.main(["predict-panel", fa, w1, out]) == 1                       # a weights file is no panel
    assert "not a panel file" in capsys.readouterr().err
    assert gp.main(["predict-panel", fa, str(tmp_path / "none.npz"), out]) == 1
    assert gp.main(["scan-panel", "--width", "8", none, pan, out]) == 1
    assert gp.main(["scan-panel", "--width", "4", fa, pan, out]) == 1
    assert "below L" in capsys.readouterr().err
    assert gp.main(["scan-panel", "--width", "2048", fa, pan, out]) == 1
    assert gp.main(["scan-panel", "--width", "8", "--stride", "0", fa, pan, out]) == 1
    assert gp.main(["scan-panel", "--width", "8", "--chunk", "7", fa, pan, out]) == 1
    assert gp.main(["scan-panel", "--width", "13", fa, pan, out]) == 1
    assert "no record holds a window" in capsys.readouterr().err
    assert gp.main(["scan-panel", "--width", "8", fa, w1, out]) == 1
    assert gp.main(["delta-panel", none, var, pan, out]) == 1
    assert gp.main(["delta-panel", fa, str(tmp_path / "none.tsv"), pan, out]) == 1
    assert gp.main(["delta-panel", "--chunk", "10", fa, var, pan, out]) == 1
    assert gp.main(["delta-panel", fa, var, pan, out]) == 1                   # the reference allele does not match
    assert "does not match" in capsys.readouterr().err
    assert gp.main(["delta-panel", fa, var, w1, out]) == 1
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
