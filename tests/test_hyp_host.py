"""Hypothetical importance without a GPU: the decomposition of tests/hyp_ref.py (explain's tally of a mutant is ism's
mismatched tally of the query, one mismatch count up) against explicit mutants, the reference against brute force, and the
`hypothetical` API's and command line's refusals (gkmqc_amd/gkmpredict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as E
from tests import helpers
from tests import hyp_ref as HR
from tests import ism_ref as R


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


# (type, L, k, d): types 0, 2 and 4; d = L - k at several L, and d < L - k
CASES = [(0, 10, 6, 3), (4, 10, 6, 4), (2, 8, 4, 4), (0, 5, 1, 4), (4, 12, 4, 8), (2, 3, 1, 2), (0, 2, 1, 1),
         (4, 6, 3, 2), (2, 10, 6, 3)]


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_mutant_tally_is_the_shifted_mismatched_tally(built, t, L, k, d):
    """H_y[t, m] == B_x[t, m + 1, b] for every t, b != x[t], m = 0..d, and H_x[t, m] == U_x[t, m]: exactly"""
    rng = np.random.default_rng(100 * t + 10 * L + d)
    for lx, ls in ((L, L), (L + 1, 2 * L + 3), (37, 29)):
        x, s = _rand(rng, lx), _rand(rng, ls)
        if lx >= 12 and ls >= 12:
            s[3:11] = (3 - x[2:10])[::-1]               # a reverse-strand copy: pairs at every mismatch count
            if lx >= 30 and ls >= 25:
                s[15:25] = x[20:30]                     # and a forward one
        U, B = R.tallies(x, s, t, L, d)
        assert np.array_equal(E.tallies(x, s, t, L, d), U), (t, L, k, d, lx)
        for tt in range(len(x)):
            for b in range(4):
                if b != x[tt]:
                    Hy = E.tallies(R.mutant(x, tt, b), s, t, L, d)
                    assert np.array_equal(Hy[tt], B[tt, 1:d + 2, b]), (t, L, k, d, lx, tt, b, Hy[tt], B[tt, :, b])
    assert B[:, 1:d + 2].sum() > 0


@pytest.mark.parametrize("t,L,k,d", [(0, 6, 3, 3), (4, 10, 6, 3), (2, 5, 1, 4)])
def test_reference_equals_brute_force_explain_of_every_mutant(gp, t, L, k, d):
    rng = np.random.default_rng(L + d)
    x = _rand(rng, 31)
    seqs = [np.concatenate((_rand(rng, 7), x[4:20], _rand(rng, 5))), (3 - x[10:30])[::-1].copy(), _rand(rng, 40)]
    model = gp.Model(t, L, k, d, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.5, 1, np.array([0.75, 1.5, 0.25]),
                     ["a", "b", "c"], seqs)
    norms = E.sv_norms(model)
    got, bound = HR.hypothetical(model, x, norms)
    want = HR.brute_force(model, x, norms=norms)
    assert np.all(np.abs(got - want) <= 1e-13 * bound + 1e-300), np.max(np.abs(got - want) - 1e-13 * bound)
    assert np.abs(want).max() > 1e-6
    own, _ = E.explanation(model, x, norms)
    assert np.allclose(got[np.arange(len(x)), x], own, rtol=1e-13, atol=0)


# ------------------------------------------------------------------ API and command line
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
def test_hypothetical_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    model, query, out = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    kw = dict(rbf3=dict(kernel_type=3), rbf5=dict(kernel_type=5), k0=dict(kernel_type=0, L=6, k=0, d=6)).get(case, {})
    _model(gp, **kw).save(model)
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGTA" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    args = ["hypothetical"] + (["--block", "0"] if case == "bad_block" else [])
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), model, out]))
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    if case.startswith("rbf"):
        assert "RBF" in r.stderr
    if case == "k0":
        assert "k = 0" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_hypothetical_api_refuses_before_touching_a_device(gp):
    for kw in (dict(kernel_type=3), dict(kernel_type=5), dict(kernel_type=0, L=6, k=0, d=6)):
        with pytest.raises(gp.ModelError, match="hypothetical"):
            gp.hypothetical(_model(gp, **kw), [np.zeros(20, np.uint8)], device=12345)


def test_default_block_fits_the_budget(gp):
    for max_len, d in ((10, 3), (600, 3), (2047, 12)):
        qb = gp.default_hyp_block(max_len, d)
        assert qb >= 1 and qb * max(max_len, 64) * 8 * (4 * gp.ISM_CHUNKS + 4 * (d + 1)) <= gp.BLOCK_BYTES
    assert gp.default_hyp_block(600, 3, budget=1) == 1
