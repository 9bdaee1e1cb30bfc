"""epsilon-SVR without a GPU (gkmqc_amd/gkmpredict.py): the targets file, the `gkmqc-svr-1` model file next to the
C-SVC one, and the argument checks of `train-svr`."""
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _svr_model(gp, n_sv=6, L=10, **kw):
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, 4, size=int(rng.integers(L, 70)), dtype=np.uint8) for _ in range(n_sv)]
    names = ["peak_%d" % i for i in range(n_sv)]
    names[2] = "a name\twith a tab"
    coef = np.array([0.5, -1.0, 1.0 / 3, -2.0 ** -30, 5e-324, -0.1 - 0.2])[:n_sv]
    args = dict(kernel_type=4, L=L, k=6, d=3, M=50, H=50.0, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
                rho=0.1 + 0.2, n0=0, alpha=coef, names=names, seqs=seqs, svm_type=gp.EPSILON_SVR, epsilon=0.1)
    args.update(kw)
    return gp.Model(**args)


def _fasta(path, names, length=30):
    rng = np.random.default_rng(len(names))
    with open(path, "w") as f:
        for n in names:
            f.write(">%s\n%s\n" % (n, "".join("ACGT"[b] for b in rng.integers(0, 4, length))))
    return str(path)


def _targets(path, rows):
    with open(path, "w") as f:
        f.write("".join("%s\t%s\n" % tuple(r) for r in rows))
    return str(path)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


# ------------------------------------------------------------------ targets file
def test_targets_file_is_read_in_fasta_order(gp, tmp_path):
    from gkmqc_amd import device as dv
    names = ["chr1:100-700", "peak two", "chr2:5-605\tsignal\tx", "last"]
    fa = _fasta(tmp_path / "s.fa", names)
    _, got_names, _, _ = dv.read_fasta(fa)
    assert got_names == names                          # the reader keeps tabs and spaces of the header
    vals = ["1.5", "-0.25", "1e-300", "  3  "]
    z = gp.read_targets(_targets(tmp_path / "t.txt", zip(names, vals)), got_names)
    assert z.dtype == np.float64 and z.tolist() == [1.5, -0.25, 1e-300, 3.0]
    # no final newline is fine too
    p = tmp_path / "t2.txt"
    p.write_text("\n".join("%s\t%s" % r for r in zip(names, vals)))
    assert gp.read_targets(str(p), got_names).tolist() == z.tolist()


@pytest.mark.parametrize("case,line", [
    ("too_few", 3), ("too_many", 4), ("name_mismatch", 2), ("nan", 2), ("inf", 3), ("minus_inf", 1),
    ("garbage", 2), ("no_tab", 1), ("empty_value", 3), ("order", 1)])
def test_bad_targets_are_refused_with_the_line(gp, tmp_path, case, line):
    names = ["a", "b\tc", "d"]
    rows = [["a", "1.0"], ["b\tc", "2.0"], ["d", "3.0"]]
    if case == "too_few":
        rows = rows[:2]
    elif case == "too_many":
        rows.append(["e", "4.0"])
    elif case == "name_mismatch":
        rows[1][0] = "b"
    elif case == "nan":
        rows[1][1] = "nan"
    elif case == "inf":
        rows[2][1] = "inf"
    elif case == "minus_inf":
        rows[0][1] = "-Infinity"
    elif case == "garbage":
        rows[1][1] = "1.0x"
    elif case == "empty_value":
        rows[2][1] = ""
    elif case == "order":
        rows[0], rows[2] = rows[2], rows[0]
    path = tmp_path / "t.txt"
    if case == "no_tab":
        path.write_text("a 1.0\nb\tc\t2.0\nd\t3.0\n")
    else:
        _targets(path, rows)
    with pytest.raises(gp.ModelError) as e:
        gp.read_targets(str(path), names)
    assert ("t.txt:%d:" % line) in str(e.value), str(e.value)


# ------------------------------------------------------------------ model file
def test_svr_model_file_round_trips_exactly(gp, tmp_path):
    m = _svr_model(gp, H=37.25, gamma=1 / 3, C=0.1 + 0.7, tol=2.0 ** -11, shrinking=True, epsilon=0.1 + 0.2)
    path = str(tmp_path / "m.txt")
    m.save(path)
    text = open(path).read()
    assert text.startswith("format gkmqc-svr-1\n") and "\nepsilon " in text and "\nn0 " not in text
    r = gp.load(path)
    assert r.is_svr and r.svm_type == gp.EPSILON_SVR and r.n0 == 0
    for key in ("kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "epsilon", "rho", "n_sv"):
        assert getattr(r, key) == getattr(m, key), key
    assert r.alpha.tobytes() == m.alpha.tobytes()
    assert r.dual_coef().tobytes() == m.alpha.tobytes()      # signed coefficients as stored, training order
    assert r.names == m.names
    assert all(np.array_equal(a, b) for a, b in zip(r.seqs, m.seqs))
    r.save(str(tmp_path / "again.txt"))
    assert open(path).read() == open(str(tmp_path / "again.txt")).read()


def _svr_lines(gp, tmp_path):
    path = str(tmp_path / "good.txt")
    _svr_model(gp).save(path)
    return open(path).read().split("\n")


@pytest.mark.parametrize("case", ["missing_epsilon", "negative_epsilon", "nan_epsilon", "coef_zero", "coef_nan",
                                  "coef_inf", "unknown_format", "n0_key", "bad_coef"])
def test_malformed_svr_models_are_refused(gp, tmp_path, case):
    lines = _svr_lines(gp, tmp_path)
    sv = lines.index("SV")

    def head(key):
        return [i for i, ln in enumerate(lines) if ln.startswith(key + " ")][0]

    def set_coef(v):
        parts = lines[sv + 2].split("\t", 1)
        lines[sv + 2] = v + "\t" + parts[1]
    if case == "missing_epsilon":
        del lines[head("epsilon")]
    elif case == "negative_epsilon":
        lines[head("epsilon")] = "epsilon -0.5"
    elif case == "nan_epsilon":
        lines[head("epsilon")] = "epsilon nan"
    elif case == "coef_zero":
        set_coef("0.0")
    elif case == "coef_nan":
        set_coef("nan")
    elif case == "coef_inf":
        set_coef("-inf")
    elif case == "unknown_format":
        lines[0] = "format gkmqc-svr-2"
    elif case == "n0_key":
        lines.insert(head("rho"), "n0 0")
    elif case == "bad_coef":
        set_coef("0.5.1")
    path = str(tmp_path / "bad.txt")
    open(path, "w").write("\n".join(lines))
    with pytest.raises(gp.ModelError):
        gp.load(path)


def test_svr_model_invariants(gp):
    with pytest.raises(gp.ModelError):
        _svr_model(gp, epsilon=None)
    with pytest.raises(gp.ModelError):
        _svr_model(gp, n0=2)
    with pytest.raises(gp.ModelError):
        _svr_model(gp, svm_type="nu_svr")
    # negative coefficients are what an SVR model holds; for a C-SVC model they stay refused
    m = _svr_model(gp)
    with pytest.raises(gp.ModelError):
        gp.Model(m.kernel_type, m.L, m.k, m.d, m.M, m.H, m.gamma, m.C, m.tol, m.shrinking, m.rho, 0, m.alpha, m.names,
                 m.seqs)
    with pytest.raises(gp.ModelError):
        gp.Model(m.kernel_type, m.L, m.k, m.d, m.M, m.H, m.gamma, m.C, m.tol, m.shrinking, m.rho, 0, np.abs(m.alpha),
                 m.names, m.seqs, epsilon=0.1)


def test_csvc_model_file_still_loads_the_same(gp, tmp_path):
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 4, size=40, dtype=np.uint8) for _ in range(5)]
    m = gp.Model(4, 10, 6, 3, 50, 50.0, 1.0, 1.0, 1e-3, False, -0.3, 2, 1.0 / np.arange(3, 8), ["n%d" % i for i in range(5)],
                 seqs)
    path = str(tmp_path / "c.txt")
    m.save(path)
    text = open(path).read()
    assert text.startswith("format gkmqc-model-1\n") and "\nn0 2\n" in text and "epsilon" not in text
    r = gp.load(path)
    assert not r.is_svr and r.svm_type == gp.C_SVC and r.epsilon is None and r.n0 == 2
    assert r.dual_coef().tobytes() == np.where(np.arange(5) < 2, -m.alpha, m.alpha).tobytes()
    assert r.rho == m.rho and r.alpha.tobytes() == m.alpha.tobytes()
    # an epsilon line does not belong to a C-SVC file
    lines = text.split("\n")
    lines.insert(1, "epsilon 0.1")
    open(path, "w").write("\n".join(lines))
    with pytest.raises(gp.ModelError):
        gp.load(path)


# ------------------------------------------------------------------ command line
@pytest.mark.parametrize("args", [
    ["-p", "-0.5"], ["-p", "nan"], ["-p", "inf"], ["-C", "0"], ["-e", "0"], ["-t", "9"], ["-M", "300"],
    ["-L", "10", "-k", "11"]])
def test_train_svr_argument_checks(built, tmp_path, args):
    out = tmp_path / "m.txt"
    r = _run("train-svr", *args, tmp_path / "missing.fa", tmp_path / "missing.txt", out)
    assert r.returncode == 1, r.stderr
    assert "gkmpredict: error:" in r.stderr
    assert "cannot read" not in r.stderr            # the argument checks come before anything is read
    assert not out.exists()


def test_train_svr_refuses_before_writing(gp, tmp_path):
    names = ["a", "b", "c"]
    fa = _fasta(tmp_path / "s.fa", names)
    out = tmp_path / "m.txt"
    r = _run("train-svr", fa, tmp_path / "missing.txt", out)
    assert r.returncode == 1 and "cannot read" in r.stderr and not out.exists()
    bad = _targets(tmp_path / "t.txt", [("a", "1"), ("b", "nan"), ("c", "2")])
    r = _run("train-svr", fa, bad, out)
    assert r.returncode == 1 and "t.txt:2:" in r.stderr and not out.exists()


def test_train_svr_refuses_too_many_sequences_before_the_gram_matrix(gp, tmp_path, monkeypatch):
    names = ["s%d" % i for i in range(5)]
    fa = _fasta(tmp_path / "s.fa", names)
    from gkmqc_amd import gkmmodel
    monkeypatch.setattr(gkmmodel, "MAX_SVR_SAMPLES", 4)

    def no_gram(*a, **k):
        raise AssertionError("the Gram matrix must not be built")
    monkeypatch.setattr(gp.dv, "gram_matrix", no_gram)
    with pytest.raises(gp.ModelError) as e:
        gp.train_svr(fa, np.zeros(5))
    assert "at most 4" in str(e.value)
    assert gp.MAX_SVR_SAMPLES * 2 <= 60000
    with pytest.raises(gp.ModelError):
        gp.train_svr(fa, np.zeros(4))           # wrong count
    with pytest.raises(gp.ModelError):
        gp.train_svr(fa, [0.0, 1.0, np.inf, 2.0, 3.0])


def test_svr_solver_refuses_a_host_matrix(built):
    import torch
    from gkmqc_amd import svmcv
    with pytest.raises(svmcv.SvmError):
        svmcv.train_svr_folds(torch.eye(3, dtype=torch.float64), [np.arange(3)], np.zeros(3))
