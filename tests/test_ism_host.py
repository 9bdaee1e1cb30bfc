"""In-silico mutagenesis without a GPU: the CPU reference (tests/ism_ref.py) against the oracle's mismatch profiles of
explicit mutants, and the `ism` API's and command line's refusals and output format (gkmqc_amd/gkmpredict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as E
from tests import helpers
from tests import ism_ref as R


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _check_profile_change(x, s, t, L, k, d, M=50, H=50.0):
    """dP_m(t, b) of the reference's tallies == gkmo_profile(y, s) - gkmo_profile(x, s), exactly, for every t, b"""
    U, B = R.tallies(x, s, t, L, d, M, H)
    dP = R.profile_change(x, U, B, d)
    P0 = E.profile(x, s, t, L, k, d, M, H).astype(np.int64)
    for tt in range(len(x)):
        for b in range(4):
            want = E.profile(R.mutant(x, tt, b), s, t, L, k, d, M, H).astype(np.int64) - P0
            assert np.array_equal(dP[tt, b], want), (t, L, k, d, tt, b, dP[tt, b], want)
    return U, B


# (type, L, k, d): d = L - k at several L, d = L - 1, and k = 0 with d = L (the only models where d = L is allowed)
CASES = [(0, 10, 6, 3), (4, 10, 6, 3), (2, 8, 4, 4), (1, 6, 2, 4), (0, 5, 1, 4), (4, 4, 1, 3), (2, 3, 0, 3),
         (0, 6, 0, 6), (4, 12, 4, 8), (0, 2, 1, 1), (2, 1, 0, 1)]


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_profile_change_equals_the_oracle_on_explicit_mutants(built, t, L, k, d):
    rng = np.random.default_rng(10 * L + d + t)
    for lx, ls in ((L, L), (L + 1, 2 * L + 3), (37, 29)):
        x, s = _rand(rng, lx), _rand(rng, ls)
        if lx >= 12 and ls >= 12:
            s[3:11] = (3 - x[2:10])[::-1]               # a reverse-strand copy: pairs at every mismatch count
        _check_profile_change(x, s, t, L, k, d)


@pytest.mark.parametrize("M,H", [(50, 50.0), (17, 9.5)])
def test_profile_change_with_positional_weights(built, M, H):
    rng = np.random.default_rng(M)
    x = _rand(rng, 61)
    s = np.concatenate((_rand(rng, 12), x[20:45], _rand(rng, 9)))
    U, B = _check_profile_change(x, s, 4, 10, 6, 3, M, H)
    assert U[:, 0].sum() > 0 and B[:, 1].sum() > 0 and B[:, 4].sum() > 0


def test_tallies_of_one_pair(built):
    """L = 4, d = 1, one l-mer each: ACGT against AGGT (one mismatch at base 1, where s has G) and its reverse complement
    ACCT (one mismatch at base 2, where it has C)"""
    x = np.array([0, 1, 2, 3], np.uint8)
    s = np.array([0, 2, 2, 3], np.uint8)
    U, B = R.tallies(x, s, 0, 4, 1)
    assert U[:, 0].tolist() == [0, 0, 0, 0]
    assert U[:, 1].tolist() == [2, 1, 1, 2]
    assert B[:, 1].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert B[:, 0].sum() == 0 and B[:, 2].sum() == 0


@pytest.mark.parametrize("t,L,k,d", [(0, 6, 3, 3), (4, 10, 6, 3), (2, 5, 0, 5), (1, 4, 1, 3)])
def test_self_profiles_equal_the_oracle(built, t, L, k, d):
    rng = np.random.default_rng(L + d)
    x = np.concatenate((_rand(rng, 20), np.tile(np.array([0, 3], np.uint8), 6), _rand(rng, 9)))
    x[30:36] = (3 - x[3:9])[::-1]                          # its own reverse complement inside
    P = R.self_profiles(x, t, L, d)
    for tt in range(len(x)):
        for b in range(4):
            y = R.mutant(x, tt, b)
            assert np.array_equal(P[tt, b], E.profile(y, y, t, L, k, d).astype(np.int64)), (tt, b)


def test_coefficients_take_c_as_zero_beyond_d(gp):
    from gkmqc_amd import device as dv
    for t, L, k, d in ((0, 10, 6, 3), (2, 8, 4, 4), (0, 6, 0, 6), (4, 12, 4, 2)):
        fu, fb, c = gp.ism_coefficients(_model(gp, t, L, k, d))
        want = dv.mismatch_weights(t, L, k)[:d + 1]
        assert c.tolist() == want.tolist() and len(fu) == len(fb) == d + 1
        ce = list(want) + [0.0]
        assert fu.tolist() == [ce[m + 1] - ce[m] for m in range(d + 1)]
        assert fb.tolist() == [ce[m - 1] - ce[m] for m in range(1, d + 2)]


# ------------------------------------------------------------------ command line
def _model(gp, kernel_type=4, L=10, k=6, d=3):
    rng = np.random.default_rng(3)
    seqs = [_rand(rng, rng.integers(L, 60)) for _ in range(5)]
    return gp.Model(kernel_type, L, k, d, 50, 50.0, 1.0, 1.0, 1e-3, False, -0.25, 2, 1.0 / np.arange(2, 7),
                    ["sv%d" % i for i in range(5)], seqs)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


@pytest.mark.parametrize("case", ["rbf3", "rbf5", "short_query", "empty_file", "bad_block", "bad_model", "missing_query"])
def test_ism_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    model, query, out = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    kw = dict(rbf3=dict(kernel_type=3), rbf5=dict(kernel_type=5)).get(case, {})
    _model(gp, **kw).save(model)
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGTA" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    args = ["ism"] + (["--block", "0"] if case == "bad_block" else [])
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), model, out]))
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    if case.startswith("rbf"):
        assert "RBF" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_ism_api_refuses_rbf_before_touching_a_device(gp):
    for kw in (dict(kernel_type=3), dict(kernel_type=5)):
        with pytest.raises(gp.ModelError):
            gp.ism(_model(gp, **kw), [np.zeros(20, np.uint8)], device=12345)


def test_ism_api_accepts_k0_models(gp):
    """k = 0 (d = L) passes the check that RBF fails: it is served"""
    gp.check_ism(_model(gp, 0, 6, 0, 6))
    gp.check_ism(_model(gp, 4, 10, 6, 3))


def test_ism_file_round_trips(gp, tmp_path):
    rng = np.random.default_rng(9)
    values = [rng.standard_normal((n, 4)) * 10.0 ** rng.integers(-300, 300, size=(n, 4)) for n in (1, 7, 600)]
    values[1][2, 1] = -0.0
    values[1][3, 3] = 5e-324
    values[1][4, 0] = 0.0
    names = ["chr1:1-2", "name with spaces\tand a tab", "x"]
    path = str(tmp_path / "i.txt")
    gp.write_ism(path, names, values)
    got_names, got = gp.read_ism(path)
    assert got_names == names
    assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, values))
    lines = open(path).read().split("\n")
    assert len(lines) == 4 and lines[-1] == ""
    assert lines[0].split("\t") == ["chr1:1-2", ",".join(repr(float(e)) for e in values[0][0])]
    assert len(lines[2].split("\t")[1].split(",")) == 4 * 600
