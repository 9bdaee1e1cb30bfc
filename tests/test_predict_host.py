"""Training / prediction without a GPU: the model file, the one-file FASTA reader, the command line's checks
(gkmqc_amd/gkmpredict.py, gkm_problem_read_one)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _model(gp, n_sv=7, n0=3, L=10, **kw):
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 4, size=int(rng.integers(L, 80)), dtype=np.uint8) for _ in range(n_sv)]
    names = ["chr1:%d-%d_p%d" % (i, i + 100, i) for i in range(n_sv)]
    names[1] = "name with spaces\tand a tab"
    args = dict(kernel_type=4, L=L, k=6, d=3, M=50, H=50.0, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
                rho=-0.1 - 0.2, n0=n0, alpha=1.0 / np.arange(3, 3 + n_sv), names=names, seqs=seqs)
    args.update(kw)
    return gp.Model(**args)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


def test_model_file_round_trips_exactly(gp, tmp_path):
    m = _model(gp, H=37.25, gamma=1 / 3, C=0.1 + 0.7, tol=2.0 ** -11, shrinking=True)
    m.alpha[2] = 5e-324                       # the smallest subnormal survives too
    path = str(tmp_path / "m.txt")
    m.save(path)
    r = gp.load(path)
    for key in ("kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "rho", "n0", "n_sv"):
        assert getattr(r, key) == getattr(m, key), key
    assert r.alpha.tobytes() == m.alpha.tobytes()
    assert r.names == m.names
    assert all(np.array_equal(a, b) for a, b in zip(r.seqs, m.seqs))
    r.save(str(tmp_path / "again.txt"))
    assert open(path).read() == open(str(tmp_path / "again.txt")).read()


def _lines(gp, tmp_path):
    path = str(tmp_path / "good.txt")
    _model(gp).save(path)
    return open(path).read().split("\n")


@pytest.mark.parametrize("case", ["missing_key", "count_too_big", "count_too_small", "bad_params", "non_acgt",
                                  "bad_format", "alpha_zero", "n0_too_big", "no_sv_line", "bad_number", "short_sv",
                                  "unknown_key"])
def test_malformed_models_are_refused(gp, tmp_path, case):
    lines = _lines(gp, tmp_path)
    head = {ln.split(" ")[0]: i for i, ln in enumerate(lines[:lines.index("SV")])}
    sv0 = lines.index("SV") + 1
    if case == "missing_key":
        del lines[head["rho"]]
    elif case == "count_too_big":
        lines[head["n_sv"]] = "n_sv 8"
    elif case == "count_too_small":
        lines[head["n_sv"]] = "n_sv 6"
    elif case == "bad_params":
        lines[head["d"]] = "d 5"              # d > L - k: gkm_check_parameter_values refuses it
    elif case == "non_acgt":
        a, name, seq = lines[sv0].split("\t")
        lines[sv0] = "\t".join((a, name, seq[:4] + "N" + seq[5:]))
    elif case == "bad_format":
        lines[head["format"]] = "format lsgkm"
    elif case == "alpha_zero":
        lines[sv0] = "0.0" + lines[sv0][lines[sv0].index("\t"):]
    elif case == "n0_too_big":
        lines[head["n0"]] = "n0 9"
    elif case == "no_sv_line":
        lines = lines[:sv0 - 1]
    elif case == "bad_number":
        lines[head["C"]] = "C one"
    elif case == "short_sv":
        a, name, seq = lines[sv0].split("\t")
        lines[sv0] = "\t".join((a, name, seq[:9]))
    elif case == "unknown_key":
        lines.insert(1, "colour blue")
    path = str(tmp_path / "bad.txt")
    open(path, "w").write("\n".join(lines))
    with pytest.raises(gp.ModelError):
        gp.load(path)


def test_one_file_reader_keeps_names_and_matches_the_pair_reader(built):
    from gkmqc_amd import device as dv
    for path, other in ((helpers.QUIRK_POS, helpers.QUIRK_NEG), (helpers.QUIRK_NEG, helpers.QUIRK_POS)):
        seqs, names, invalid, truncated = dv.read_fasta(path)
        pair, npos, _, _ = dv.read_problem(path, other)
        assert len(seqs) == npos
        assert np.array_equal(seqs.off, pair.off[:npos + 1])
        assert np.array_equal(seqs.codes, pair.codes[:pair.off[npos]])
        raw = open(path, "rb").read().decode()
        expect = [ln[1:].split("\r")[0] for ln in raw.split("\n") if ln.startswith(">")]
        assert names == expect
    # the quirks file holds lowercase letters, invalid characters and an over-long record
    seqs, names, invalid, truncated = dv.read_fasta(helpers.QUIRK_POS)
    assert invalid > 0 and truncated > 0 and max(np.diff(seqs.off)) == 2047


def test_one_file_reader_edge_cases(built, tmp_path):
    from gkmqc_amd import device as dv
    p = tmp_path / "e.fa"
    p.write_bytes(b"junk before\n>first one\r\nacgtN\n\n>\nTTTT\n>last")
    seqs, names, invalid, truncated = dv.read_fasta(str(p))
    assert names == ["first one", "", "last"]
    assert [list(s) for s in seqs] == [[0, 1, 2, 3, 0], [3, 3, 3, 3], []]
    assert invalid == 1 and truncated == 0
    (tmp_path / "empty.fa").write_bytes(b"")
    seqs, names, _, _ = dv.read_fasta(str(tmp_path / "empty.fa"))
    assert len(seqs) == 0 and names == []
    with pytest.raises(dv.GkmError):
        dv.read_fasta(str(tmp_path / "missing.fa"))


def test_cli_argument_checks(built, tmp_path):
    assert _run().returncode == 2
    assert _run("train", helpers.QUIRK_POS).returncode == 2
    assert _run("predict", helpers.QUIRK_POS, "m.txt").returncode == 2
    assert _run("train", "-u", "2", helpers.QUIRK_POS, helpers.QUIRK_NEG, tmp_path / "m").returncode == 2
    for bad in (["-d", "5"], ["-t", "7"], ["-L", "13"], ["-M", "300"], ["-C", "0"], ["-e", "-1"]):
        model = tmp_path / "m.txt"
        r = _run("train", *bad, helpers.QUIRK_POS, helpers.QUIRK_NEG, model)
        assert r.returncode == 1 and "error" in r.stderr and not model.exists(), bad
    r = _run("train", tmp_path / "missing.fa", helpers.QUIRK_NEG, tmp_path / "m.txt")
    assert r.returncode == 1 and not (tmp_path / "m.txt").exists()


def test_predict_rejects_before_writing(gp, tmp_path):
    """An empty query file, a query shorter than L, a model whose parameters fail the check, a bad block size: non-zero
    exit, no output file -- all decided before the device is touched."""
    good = str(tmp_path / "good.txt")
    _model(gp, L=10).save(good)
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write(open(good).read().replace("\nd 3\n", "\nd 9\n"))
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    short = tmp_path / "short.fa"
    short.write_text(">a\nACGTACGTACGTAC\n>b\nACGTACGTA\n")
    ok = tmp_path / "ok.fa"
    ok.write_text(">a\nACGTACGTACGTAC\n")
    out = tmp_path / "out.txt"
    for args, why in (((empty, good), "no query"), ((short, good), "shorter than L"), ((ok, bad), "rejected"),
                      ((tmp_path / "missing.fa", good), "cannot read"), ((ok, tmp_path / "nomodel.txt"), "")):
        r = _run("predict", *args, out)
        assert r.returncode == 1 and why in r.stderr and not out.exists(), (args, r.stderr)
    r = _run("predict", "--block", "0", ok, good, out)
    assert r.returncode == 1 and not out.exists()


def test_default_block_is_bounded(gp):
    for s in (1, 100, 5000, 60000):
        qb = gp.default_block(s)
        assert 1 <= qb and 16 * max(s, 64) * qb <= gp.BLOCK_BYTES
    assert gp.default_block(5000) > 10000
