"""PWM motifs against a table or panel without a GPU (gkmqc_amd/gkmmotifs.py): the MEME reader on good and
malformed files, the windows of a motif, row normalisation and its refusals, the peak's tie rule, the host restatement of
the contraction against tests/motif_ref.py, the files, the command line's shape and the refusals of the check functions."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import motif_ref as R


@pytest.fixture(scope="module")
def gm(built):
    from gkmqc_amd import gkmmotifs
    return gkmmotifs


@pytest.fixture(scope="module")
def gt(built):
    from gkmqc_amd import gkmtables
    return gkmtables


def _table(gt, L=5, seed=1):
    W = R.symmetric_table(np.random.default_rng(seed), L)
    return gt.LmerTable(W, 2, L, L - 1, 1, 50, 50.0, 0.25)


GOOD = """MEME version 4

ALPHABET= ACGT

strands: + -

Background letter frequencies
A 0.25 C 0.25 G 0.25 T 0.25

MOTIF one first_alt
letter-probability matrix: alength= 4 w= 3 nsites= 20 E= 0
0.100000 0.200000 0.300000 0.400000
 1.000000  0.000000  0.000000  0.000000
0.250000\t0.250000\t0.250000\t0.250001
URL http://example.invalid/one

MOTIF two
letter-probability matrix: w= 1
0 0 1 0
"""


def _write(tmp_path, text, name="m.meme"):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_reader_on_a_good_file(gm, tmp_path):
    got = gm.read_motifs(_write(tmp_path, GOOD))
    assert [n for n, _ in got] == ["one", "two"]
    one, two = got[0][1], got[1][1]
    assert one.shape == (3, 4) and one.dtype == np.float64 and two.tolist() == [[0.0, 0.0, 1.0, 0.0]]
    raw = np.array([[0.1, 0.2, 0.3, 0.4], [1, 0, 0, 0], [0.25, 0.25, 0.25, 0.250001]])
    assert one.tobytes() == R.normalise(raw).tobytes()
    assert one[1].tolist() == [1.0, 0.0, 0.0, 0.0]
    # a file that ends inside the last matrix's last row, without a final newline
    assert len(gm.read_motifs(_write(tmp_path, GOOD.rstrip("\n"), "n.meme"))) == 2


@pytest.mark.parametrize("edit,line,text", [
    (lambda s: s.replace("ALPHABET= ACGT", "ALPHABET= ACDEFGHIKLMNPQRSTVWY"), 3, "alphabet must be ACGT"),
    (lambda s: s.replace("MOTIF two", "MOTIF one"), 17, "given twice"),
    (lambda s: s.replace("w= 3", "w= 4"), 15, "3 rows where w= announces 4"),
    (lambda s: s.replace("w= 3", "w= 2"), 14, "a row beyond the 2"),
    (lambda s: s.replace("w= 1", "w= 0"), 18, "outside 1..64"),
    (lambda s: s.replace("w= 1", "w= 65"), 18, "outside 1..64"),
    (lambda s: s.replace("w= 1", "nsites= 3"), 18, "no integer w="),
    (lambda s: s.replace("alength= 4", "alength= 20"), 11, "alength= 20"),
    (lambda s: s.replace(" 1.000000  0.000000  0.000000  0.000000", "1.0 0.0 0.0"), 13, "row 1 is not four numbers"),
    (lambda s: s.replace(" 1.000000  0.000000  0.000000  0.000000", "1.0 0.0 x 0.0"), 13, "row 1 is not four numbers"),
    (lambda s: s.replace("0.100000 0.200000", "0.100000 0.300000"), 12, "motif one: row 0 sums to"),
    (lambda s: s.replace("0 0 1 0", "0 0 1.5 -0.5"), 19, "motif two: row 0 holds a value"),
    (lambda s: s.replace("0 0 1 0", "0 0 nan 1"), 19, "motif two: row 0 holds a value"),
    (lambda s: s.replace("letter-probability matrix: w= 1\n0 0 1 0\n", ""), 17, "has no letter-probability matrix"),
    (lambda s: s.replace("MOTIF one first_alt\n", ""), 10, "without a MOTIF line"),
    (lambda s: s.replace("MOTIF two", "MOTIF"), 17, "MOTIF without a name"),
])
def test_reader_refuses_malformed_files_with_path_and_line(gm, tmp_path, edit, line, text):
    path = _write(tmp_path, edit(GOOD))
    with pytest.raises(gm.MotifError) as e:
        gm.read_motifs(path)
    assert str(e.value).startswith("%s:%d: " % (path, line)) and text in str(e.value), str(e.value)


def test_reader_refuses_a_file_without_motifs(gm, tmp_path):
    path = _write(tmp_path, "MEME version 4\n\nALPHABET= ACGT\n")
    with pytest.raises(gm.MotifError, match="holds no motif"):
        gm.read_motifs(path)


@pytest.mark.parametrize("m", [2, 5, 9])          # m < L, m = L, m > L at L = 5
def test_windows_shapes_and_padding(gm, m):
    L, bg = 5, np.array([0.1, 0.2, 0.3, 0.4])
    M = R.dirichlet_motif(np.random.default_rng(m), m)
    P = gm.motif_windows(M, L, bg)
    assert P.shape == (m + L - 1, L, 4) and P.dtype == np.float64 and P.flags["C_CONTIGUOUS"]
    assert P.tobytes() == R.windows(M, L, bg).tobytes()
    for o in range(m + L - 1):
        for i in range(L):
            c = o + i - (L - 1)                   # the motif column under position i of window o
            assert P[o, i].tolist() == (M[c].tolist() if 0 <= c < m else bg.tolist())
    assert P[0, L - 1].tolist() == M[0].tolist() and P[-1, 0].tolist() == M[-1].tolist()
    assert gm.motif_windows(M, L).tobytes() == R.windows(M, L, np.full(4, 0.25)).tobytes()


def test_row_normalisation_and_its_refusals(gm):
    M = np.array([[0.1, 0.2, 0.3, 0.4009], [0.25, 0.25, 0.25, 0.2401], [2 ** -60, 0.0, 1.0, 0.0]])
    got = gm.normalise_motif("x", M)
    assert got.tobytes() == R.normalise(M).tobytes() and np.abs(got.sum(axis=1) - 1).max() < 1e-15
    assert gm.normalise_motif("x", [[0, 1, 0, 0]]).tolist() == [[0.0, 1.0, 0.0, 0.0]]
    for bad, text in (([[0.1, 0.2, 0.3, 0.411]], "row 0 sums to"), ([[0.25] * 4, [0.25, 0.25, 0.25, 0.2399]], "row 1 sums to"),
                      ([[0.5, 0.6, -0.1, 0.0]], "row 0 holds a value"), ([[0.25] * 4, [np.inf, 0, 0, 0]], "row 1 holds a value"),
                      ([[np.nan, 0.5, 0.5, 0]], "row 0 holds a value"), ([[0.5, 0.5, 0.0]], "shape"), ([], "shape"),
                      (np.full((65, 4), 0.25), "shape"), ([["a", 0, 0, 1]], "not an array of numbers")):
        with pytest.raises(gm.MotifError) as e:
            gm.normalise_motif("name7", bad)
        assert "motif name7" in str(e.value) and text in str(e.value), str(e.value)
    assert gm.normalise_motif("w", np.full((64, 4), 0.25)).shape == (64, 4)
    for bad in ([0.25, 0.25, 0.25], [0.5, 0.5, 0.5, 0.5], [1.0, 0.0, np.nan, 0.0], [1.1, -0.1, 0.0, 0.0], "acgt"):
        with pytest.raises(gm.MotifError, match="background"):
            gm.check_background(bad)
    assert gm.check_background(None).tolist() == [0.25] * 4
    assert gm.check_background([0.3, 0.2, 0.2, 0.3001]).tobytes() == R.normalise([[0.3, 0.2, 0.2, 0.3001]])[0].tobytes()


def test_summary_follows_the_stated_arithmetic_and_the_peak_takes_the_lowest_offset(gm):
    rng = np.random.default_rng(5)
    L, m = 4, 6
    prof = rng.standard_normal(m + L - 1)
    prof[2] = prof[7] = prof.max() + 1.0                # a tie: the lower window wins
    b0 = 0.03125 + rng.random()
    aff, enr, peak, off = gm.summarise_profile(prof, m, L, b0)
    want = R.summary(prof, m, L, b0)
    assert (np.float64(aff).tobytes(), np.float64(enr).tobytes(), np.float64(peak).tobytes(), int(off)) == \
        (want[0].tobytes(), want[1].tobytes(), want[2].tobytes(), want[3])
    assert int(off) == 2 - (L - 1) and peak == prof[2]
    # a panel's profile: every column on its own
    prof2 = np.stack([prof, prof[::-1].copy(), rng.standard_normal(m + L - 1)], axis=1)
    b2 = np.array([b0, -b0, 0.5])
    aff2, enr2, peak2, off2 = gm.summarise_profile(prof2, m, L, b2)
    for c in range(3):
        want = R.summary(prof2[:, c], m, L, b2[c])
        assert (aff2[c].tobytes(), enr2[c].tobytes(), peak2[c].tobytes(), int(off2[c])) == \
            (want[0].tobytes(), want[1].tobytes(), want[2].tobytes(), want[3])
    assert off2[:2].tolist() == [2 - (L - 1), 1 - (L - 1)]


def test_host_restatement_equals_the_reference_and_a_one_hot_window_returns_its_weight(gm):
    rng = np.random.default_rng(11)
    for L in (2, 3, 5):
        W = R.symmetric_table(rng, L)
        for M in (R.dirichlet_motif(rng, 1), R.dirichlet_motif(rng, L + 2)):
            for P in gm.motif_windows(M, L, [0.2, 0.3, 0.3, 0.2]):
                assert np.float64(gm.contract_reference(W, P)).tobytes() == R.contract(W, P).tobytes()
        u = int(rng.integers(0, 4 ** L))
        digits = [(u >> (2 * (L - 1 - i))) & 3 for i in range(L)]
        assert gm.contract_reference(W, np.eye(4)[digits]) == W[u] == R.contract(W, np.eye(4)[digits])
    assert gm.reverse_complement_motif([[0.1, 0.2, 0.3, 0.4], [1, 0, 0, 0]]).tolist() == [[0, 0, 0, 1], [0.4, 0.3, 0.2, 0.1]]
    P = gm.marginal_windows(3)
    assert P.shape == (3, 4, 3, 4) and P[1, 2].tolist() == [[0.25] * 4, [0, 0, 1, 0], [0.25] * 4]


def _result(rng, n, cols=()):
    return dict(names=["m%d" % i for i in range(n)], width=rng.integers(1, 20, size=n),
                affinity=rng.standard_normal((n,) + cols), enrichment=rng.standard_normal((n,) + cols) * 1e-7,
                peak=rng.standard_normal((n,) + cols), peak_offset=rng.integers(-9, 9, size=(n,) + cols),
                background=rng.standard_normal(cols) if cols else 0.1 + 0.2,
                profiles=[rng.standard_normal((int(w) + 4,) + cols) for w in rng.integers(1, 5, size=n)])


def test_files_round_trip(gm, tmp_path):
    rng = np.random.default_rng(3)
    r = _result(rng, 5)
    path = str(tmp_path / "s.tsv")
    gm.write_motif_scores(path, r)
    assert not os.path.exists(path + ".tmp")
    back = gm.read_motif_scores(path)
    assert back["names"] == r["names"] and back["background"] == r["background"]
    for key in ("width", "affinity", "enrichment", "peak", "peak_offset"):
        assert back[key].tobytes() == np.asarray(r[key]).tobytes(), key
    with open(path) as f:
        assert f.readline() == "#name\twidth\taffinity\tbackground\tenrichment\tpeak\tpeak_offset\n"
    gm.write_motif_profiles(path, r, 5)
    names, offs, vals = gm.read_motif_profiles(path)
    assert names == r["names"] and all(o.tolist() == list(range(-4, len(p) - 4)) for o, p in zip(offs, r["profiles"]))
    assert all(v.tobytes() == p.tobytes() for v, p in zip(vals, r["profiles"]))
    with pytest.raises(gm.MotifError, match="no motif score header"):
        gm.read_motif_scores(path)
    # a panel: one field, one column per member
    rp = _result(rng, 4, (3,))
    members = ["a", "b c", "d"]
    gm.write_panel_motif_scores(path, members, rp)
    got = gm.read_panel_motif_scores(path)
    assert got[0] == members and got[1] == rp["names"] and got[2].tobytes() == rp["enrichment"].tobytes()
    gm.write_panel_motif_scores(path, members, rp, "peak")
    assert gm.read_panel_motif_scores(path)[2].tobytes() == rp["peak"].tobytes()
    with pytest.raises(gm.MotifError, match="field"):
        gm.write_panel_motif_scores(path, members, rp, "background")
    gm.write_motif_profiles(path, rp, 5)
    names, offs, vals = gm.read_motif_profiles(path)
    assert names == rp["names"] and all(v.tobytes() == p.tobytes() for v, p in zip(vals, rp["profiles"]))
    marg = rng.standard_normal((7, 4))
    gm.write_marginals(path, marg)
    assert gm.read_marginals(path).tobytes() == marg.tobytes() and not os.path.exists(path + ".tmp")
    with pytest.raises(gm.MotifError, match="no marginals header"):
        gm.read_marginals(_write(tmp_path, "x\n", "bad.tsv"))


def test_check_functions_refuse_without_a_device(gm, gt):
    table = _table(gt)
    panel = gt.LmerPanel([_table(gt, seed=s) for s in (1, 2, 3)])
    motifs = [("a", [[0.25] * 4]), ("b", [[1, 0, 0, 0], [0, 0.5, 0.5, 0]])]
    names, mats, bg = gm.check_motif_scores(table, motifs)
    assert names == ["a", "b"] and bg.tolist() == [0.25] * 4 and [M.shape for M in mats] == [(1, 4), (2, 4)]
    assert gm.check_panel_motif_scores(panel, motifs, [0.3, 0.2, 0.2, 0.3], 7)[2].tobytes() == R.normalise([[0.3, 0.2, 0.2, 0.3]])[0].tobytes()

    class NoTable:
        kernel_type, L = 2, 5
    for check, good, others in ((gm.check_motif_scores, table, (panel, NoTable())),
                                (gm.check_panel_motif_scores, panel, (table, NoTable()))):
        for other in others:
            with pytest.raises(gt.ModelError, match="needs an l-mer weight"):
                check(other, motifs)
        with pytest.raises(gm.MotifError, match="background"):
            check(good, motifs, background=[0.5, 0.5, 0.5, 0.5])
        for block in (0, -1, 65537):
            with pytest.raises(gm.MotifError, match="a block holds 1..65536 windows"):
                check(good, motifs, block=block)
        with pytest.raises(gm.MotifError, match="no motifs"):
            check(good, [])
        with pytest.raises(gm.MotifError, match="given twice"):
            check(good, motifs + [("a", [[0.25] * 4])])
        with pytest.raises(gm.MotifError, match="motif b: row 1 sums to"):
            check(good, [("a", [[0.25] * 4]), ("b", [[1, 0, 0, 0], [0, 0.5, 0.6, 0]])])
        with pytest.raises(gm.MotifError, match="name of motif 0"):
            check(good, [("", [[0.25] * 4])])
        with pytest.raises(gm.MotifError, match="no \\(name, matrix\\) pair"):
            check(good, [5])
    assert gm.default_motif_block(5) == 65536 and gm.default_motif_block(12, 64) == (2 << 30) // (32 * 12 + 8 * 64 + (8 * 64 << 12))
    assert gm.default_motif_block(10, 0, budget=1 << 20) == (1 << 20) // (320 + 8 + 2048)


def test_command_line_shape(gm):
    p = gm.build_parser()
    a = p.parse_args(["score", "--background", "0.3,0.2,0.2,0.3", "--profiles", "p.tsv", "--block", "9", "--device", "1", "w", "m", "o"])
    assert (a.cmd, a.source, a.motifs, a.output, a.background, a.profiles, a.block, a.device) == \
        ("score", "w", "m", "o", "0.3,0.2,0.2,0.3", "p.tsv", 9, 1)
    a = p.parse_args(["score-panel", "--field", "peak", "pn", "m", "o"])
    assert (a.cmd, a.source, a.motifs, a.output, a.field, a.block, a.background) == ("score-panel", "pn", "m", "o", "peak", None, None)
    assert p.parse_args(["score-panel", "pn", "m", "o"]).field == "enrichment"
    a = p.parse_args(["marginals", "w", "o"])
    assert (a.cmd, a.source, a.output, a.device) == ("marginals", "w", "o", 0) and not hasattr(a, "motifs")
    for bad in (["score", "w", "m"], ["marginals", "w", "m", "o"], ["marginals", "--block", "3", "w", "o"], ["best", "w", "m", "o"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert gm.parse_background("0.1,0.2,0.3,0.4") == [0.1, 0.2, 0.3, 0.4]
    with pytest.raises(gm.MotifError):
        gm.parse_background("0.1,x")


def test_a_missing_input_is_refused_by_name(gm, gt, tmp_path, capsys):
    wpath, mpath, out = str(tmp_path / "w.txt"), _write(tmp_path, GOOD), str(tmp_path / "o.tsv")
    _table(gt).save(wpath)
    gone = str(tmp_path / "gone")
    for argv in (["score", gone, mpath, out], ["score", wpath, gone, out], ["score-panel", gone, mpath, out],
                 ["marginals", gone, out]):
        assert gm.main(argv) == 1
        assert "gkmmotifs: error: cannot read %s" % gone in capsys.readouterr().err
    # refusals that need no device either: a bad field, a bad background, a malformed motif file; nothing is written
    assert gm.main(["score-panel", "--field", "background", wpath, mpath, out]) == 1 and "field" in capsys.readouterr().err
    assert gm.main(["score", "--background", "1,1,1,1", wpath, mpath, out]) == 1 and "background" in capsys.readouterr().err
    assert gm.main(["score", wpath, wpath, out]) == 1 and "holds no motif" in capsys.readouterr().err
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmmotifs", "score", gone, mpath, out], cwd=helpers.ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read %s" % gone in r.stderr
