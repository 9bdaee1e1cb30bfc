"""Mutant scores without a GPU: the `mutant_scores` API's and command line's refusals, its block size and its output
format (gkmqc_amd/gkmpredict.py)."""
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


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _model(gp, kernel_type=5, L=10, k=6, d=3):
    rng = np.random.default_rng(3)
    seqs = [_rand(rng, rng.integers(L, 60)) for _ in range(5)]
    return gp.Model(kernel_type, L, k, d, 50, 50.0, 2.0, 1.0, 1e-3, False, -0.25, 2, 1.0 / np.arange(2, 7),
                    ["sv%d" % i for i in range(5)], seqs)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


@pytest.mark.parametrize("kernel_type", [5, 4])
@pytest.mark.parametrize("case", ["short_query", "empty_file", "bad_block", "bad_model", "missing_query"])
def test_mutant_scores_refusals_exit_1_and_write_nothing(gp, tmp_path, case, kernel_type):
    model, query, out = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    _model(gp, kernel_type).save(model)
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGTA" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    args = ["mutant-scores"] + (["--block", "0"] if case == "bad_block" else []) + ["--device", "12345"]
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), model, out]))
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_api_raises_on_bad_queries_before_touching_a_device(gp):
    for t in (0, 3, 4, 5):
        model = _model(gp, t)
        with pytest.raises(gp.ModelError):
            gp.mutant_scores(model, [np.zeros(9, np.uint8)], device=12345)                          # shorter than L
        with pytest.raises(gp.ModelError):
            gp.mutant_scores(model, [np.zeros(20, np.uint8), np.zeros(3, np.uint8)], device=12345)
        with pytest.raises(gp.ModelError):
            gp.mutant_scores(model, [], device=12345)


def test_rbf_models_are_served_where_ism_refuses_them(gp):
    """the refusal stays `ism`'s own: nothing named check_mutant_scores is needed, since nothing `score` serves is refused"""
    for t in (3, 5):
        with pytest.raises(gp.ModelError):
            gp.check_ism(_model(gp, t))
    cmds = gp.build_parser().parse_args(["mutant-scores", "--block", "3", "--device", "1", "q.fa", "m.txt", "o.txt"])
    assert (cmds.cmd, cmds.block, cmds.device, cmds.query_fa, cmds.model, cmds.output) == \
        ("mutant-scores", 3, 1, "q.fa", "m.txt", "o.txt")
    assert gp._QUERY_COMMANDS["mutant-scores"] == (gp.mutant_scores, gp.write_ism)


def test_default_block_is_positive_and_shrinks_with_support_vectors_and_length(gp):
    f = gp.default_mutscores_block
    for d in (3, 8):
        assert f(600, d, 7467) >= 1 and f(2047, d, 10 ** 7) >= 1 and f(10, d, 0) >= 1
        assert f(600, d, 100) > f(600, d, 10 ** 5) > f(600, d, 10 ** 6)
        assert f(100, d, 7467) > f(600, d, 7467) > f(2047, d, 7467)
        assert f(600, d, 7467) <= gp.default_ism_block(600, d)          # the Gram block and the norms come on top
    assert f(600, 8, 7467) < f(600, 3, 7467)
    assert f(600, 3, 7467, budget=1000) == 1                               # never below one query
    # what a block holds stays within the budget: per query, ism's buffers, 32 more bytes per base, 16 per support vector
    qb = f(600, 3, 7467)
    assert qb * (600 * 8 * (3 * gp.ISM_CHUNKS + 4 * 4 + 28) + 16 * 7467) <= gp.BLOCK_BYTES


def test_file_round_trips(gp, tmp_path):
    """the output is the ism file format: scores with an offset, the own-base column included, read back bit for bit"""
    rng = np.random.default_rng(11)
    values = [rng.standard_normal((n, 4)) - 0.731 for n in (10, 37, 600)]
    for v in values:
        x = rng.integers(0, 4, size=len(v))
        v[np.arange(len(v)), x] = v[0, x[0]]                              # one double down the own-base column
    names = ["chr2:5-15", "a name\twith a tab", "y"]
    path = str(tmp_path / "ms.txt")
    gp.write_ism(path, names, values)
    got_names, got = gp.read_ism(path)
    assert got_names == names
    assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, values))
