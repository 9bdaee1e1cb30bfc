"""Per-base importance without a GPU: the CPU reference (tests/explain_ref.py) against the oracle's mismatch profiles, and
the `explain` command line's refusals and output format (gkmqc_amd/gkmpredict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as R
from tests import helpers


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _check_completeness(x, s, t, L, k, d, M=50, H=50.0):
    """sum_t H[t][m] == (L - m) P_m(x, s), exactly, for every m <= d"""
    Ht = R.tallies(x, s, t, L, d, M, H)
    P = R.profile(x, s, t, L, k, d, M, H).astype(np.int64)
    want = (L - np.arange(d + 1)) * P
    assert np.array_equal(Ht.sum(axis=0), want), (t, L, k, d, Ht.sum(axis=0), want)
    return Ht


@pytest.mark.parametrize("t,M,H", [(0, 50, 50.0), (1, 50, 50.0), (2, 50, 50.0), (4, 50, 50.0), (4, 17, 9.5)])
def test_tallies_sum_to_the_oracle_profile(built, t, M, H):
    rng = np.random.default_rng(100 + t + M)
    for L in range(2, 13):
        for k in sorted({L, max(1, L - 4), 1}):
            for d in sorted({0, L - k}):
                for lx, ls in ((L, L + 3), (int(rng.integers(L, 90)), int(rng.integers(L, 90))), (57, L)):
                    _check_completeness(_rand(rng, lx), _rand(rng, ls), t, L, k, d, M, H)


def test_tallies_of_a_long_ragged_pair_with_repeats(built):
    rng = np.random.default_rng(7)
    x = np.concatenate((_rand(rng, 150), np.tile(np.array([0, 1], np.uint8), 40), _rand(rng, 211)))
    s = np.concatenate((_rand(rng, 33), (3 - x[120:260])[::-1], _rand(rng, 64)))     # x's reverse complement inside s
    Ht = _check_completeness(x, s, 4, 10, 6, 3)
    assert Ht[:, 0].sum() > 0                      # the reverse-strand copy is found with no mismatch


def test_tallies_of_non_acgt_input_read_as_the_reader_encodes_it(built, tmp_path):
    from gkmqc_amd import device as dv
    path = str(tmp_path / "q.fa")
    with open(path, "w") as f:
        f.write(">a\nACGTNNacgtRYKMACGGGTTTACCA\nNNNNACGTAC\n>b\nTTGACnnnnGTCAGGGAAACTTACAGTAGGA\n")
    seqs, names, invalid, _ = dv.read_fasta(path)
    assert invalid > 0 and names == ["a", "b"]
    x, s = seqs[0], seqs[1]
    for t, L, k, d in ((0, 6, 3, 3), (2, 8, 5, 3), (4, 10, 6, 3)):
        _check_completeness(x, s, t, L, k, d)
        _check_completeness(s, x, t, L, k, d)


def test_tallies_credit_only_matched_bases(built):
    """one l-mer each, L = 4: the pair ACGT / AGGT has one mismatch at base 1; the reverse complement of AGGT is ACCT,
    which has one mismatch at base 2"""
    x = np.array([0, 1, 2, 3], np.uint8)
    s = np.array([0, 2, 2, 3], np.uint8)
    Ht = R.tallies(x, s, 0, 4, 1)
    assert Ht[:, 0].tolist() == [0, 0, 0, 0]
    assert Ht[:, 1].tolist() == [2, 1, 1, 2]


# ------------------------------------------------------------------ command line
def _model(gp, kernel_type=4, L=10, k=6, d=3):
    rng = np.random.default_rng(3)
    seqs = [_rand(rng, rng.integers(L, 60)) for _ in range(5)]
    return gp.Model(kernel_type, L, k, d, 50, 50.0, 1.0, 1.0, 1e-3, False, -0.25, 2, 1.0 / np.arange(2, 7),
                    ["sv%d" % i for i in range(5)], seqs)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


@pytest.mark.parametrize("case", ["rbf3", "rbf5", "k0", "short_query", "empty_file", "bad_block", "bad_model",
                                  "missing_query"])
def test_explain_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    model, query, out = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    kw = dict(rbf3=dict(kernel_type=3), rbf5=dict(kernel_type=5), k0=dict(k=0, d=10)).get(case, {})
    _model(gp, **kw).save(model)
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGTA" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    args = ["explain"] + (["--block", "0"] if case == "bad_block" else [])
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), model, out]))
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_explain_api_refuses_rbf_and_k0_before_touching_a_device(gp):
    for kw in (dict(kernel_type=3), dict(kernel_type=5), dict(k=0, d=10)):
        with pytest.raises(gp.ModelError):
            gp.explain(_model(gp, **kw), [np.zeros(20, np.uint8)], device=12345)


def test_shares_are_gkmexplain_split_for_type_0(gp):
    """type 0: c_m = C(L - m, k), so c_m / (L - m) = C(L - m - 1, k - 1) / k"""
    from math import comb
    for L, k, d in ((10, 6, 4), (12, 3, 9), (5, 5, 0), (2, 1, 1)):
        sh = gp.explain_shares(_model(gp, 0, L, k, d))
        assert sh.tolist() == [comb(L - m - 1, k - 1) / k for m in range(d + 1)]


def test_explanation_file_round_trips(gp, tmp_path):
    rng = np.random.default_rng(9)
    values = [rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, size=n) for n in (1, 7, 600)]
    values[1][2] = -0.0
    values[1][3] = 5e-324
    names = ["chr1:1-2", "name with spaces\tand a tab", "x"]
    path = str(tmp_path / "e.txt")
    gp.write_explanation(path, names, values)
    got_names, got = gp.read_explanation(path)
    assert got_names == names
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, values))
    lines = open(path).read().split("\n")
    assert len(lines) == 4 and lines[-1] == ""
    assert lines[0].split("\t") == ["chr1:1-2", repr(float(values[0][0]))]
