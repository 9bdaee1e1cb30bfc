"""L-mer weight tables without a GPU: the CPU reference (tests/lmer_ref.py) against the oracle's mismatch profiles and
scores, gkmpredict's host aggregation of the support vectors' l-mers, the weights file format, and the `weights` and
`predict-table` command lines' refusals (gkmqc_amd/gkmpredict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as R
from tests import helpers
from tests import lmer_ref as LR


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _model(gp, kernel_type=4, L=6, k=3, d=2, M=50, H=50.0, n_sv=5, seed=3, rho=-0.25):
    """a trained-looking model: random support vectors of ragged lengths, one of them with a palindromic stretch"""
    rng = np.random.default_rng(seed)
    seqs = [_rand(rng, rng.integers(L, 60)) for _ in range(n_sv)]
    half = _rand(rng, 8)
    seqs[0] = np.concatenate((seqs[0], half, (3 - half)[::-1]))
    alpha = 1.0 / np.arange(2, 2 + n_sv)
    return gp.Model(kernel_type, L, k, d, M, H, 1.0, 1.0, 1e-3, False, rho, n_sv // 2, alpha,
                    ["sv%d" % i for i in range(n_sv)], seqs)


CASES = [(0, 5, 2, 2), (1, 6, 3, 2), (2, 6, 4, 1), (4, 6, 3, 3), (4, 5, 1, 4), (0, 6, 0, 6)]


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_reference_table_matches_the_oracle_profiles(gp, t, L, k, d):
    """W(u) = sum_s coef_s sum_m c_m P_m(u, s) / w_u, P_m the oracle's profile of the L-base sequence u against s and
    w_u = position_weights(type, 1) (50 for type 4 with M = 50)"""
    from oracle import oracle as O
    model = _model(gp, t, L, k, d)
    norms = R.sv_norms(model)
    c = O.mismatch_weights(t, L, k)[:d + 1]
    w_u = float(R.weights(t, 1, model.M, model.H)[0])
    assert w_u == (50.0 if t == 4 else 1.0)
    rng = np.random.default_rng(L + d)
    u = np.concatenate(([0, 4 ** L - 1], rng.integers(0, 4 ** L, size=60)))
    W, bound = LR.table(model, u, norms)
    for code, got, b in zip(u, W, bound):
        x = np.array([(int(code) >> (2 * (L - 1 - i))) & 3 for i in range(L)], dtype=np.uint8)
        want = 0.0
        for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
            P = R.profile(x, s, t, L, k, d, model.M, model.H).astype(np.float64)
            want += coef / sqs * float(np.dot(c, P)) / w_u
        assert abs(got - want) <= 1e-13 * max(b, 1e-300), (t, L, d, int(code), got, want)
    rc = LR.rc_codes(u, L)
    W_rc, _ = LR.table(model, rc, norms)
    assert np.allclose(W, W_rc, rtol=1e-14, atol=1e-300)


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_decomposition_reproduces_the_oracle_score(gp, t, L, k, d):
    """T(x) / sq_x + rho from the reference table equals the oracle's score, ragged x down to length L"""
    model = _model(gp, t, L, k, d)
    norms = R.sv_norms(model)
    W, _ = LR.table(model, np.arange(4 ** L), norms)
    rng = np.random.default_rng(5 * L + t)
    queries = [_rand(rng, n) for n in (L, L + 1, 9, 37, 120)]
    queries.append(np.concatenate((model.seqs[1][:20], (3 - model.seqs[2])[::-1])))
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    for x in queries:
        sqx = R.self_norm(x, t, L, k, d, model.M, model.H)
        got = LR.table_score(model, W, x) / sqx + model.rho
        want = LR.oracle_score(model, x, norms)
        assert abs(got - want) <= tol, (t, L, d, len(x), got, want)


@pytest.mark.parametrize("t", [0, 4])
def test_host_classes_match_a_plain_loop(gp, t):
    model = _model(gp, t, 6, 3, 2, n_sv=7, seed=11)
    norms = R.sv_norms(model)
    v, cv = gp.lmer_classes(model, norms)
    want = LR.classes(model, norms)
    assert v.dtype == np.uint32 and (np.diff(v.astype(np.int64)) > 0).all()
    assert sorted(want) == v.tolist()
    assert (v.astype(np.int64) <= LR.rc_codes(v, 6)).all()
    got = dict(zip(v.tolist(), cv.tolist()))
    for key, val in want.items():
        assert abs(got[key] - val) <= 1e-15 * max(abs(val), 1e-300) * 8, key
    # the classes' (v, cv) give the reference table through the same count
    from oracle import oracle as O
    c = O.mismatch_weights(t, 6, 3)[:3]
    u = np.arange(4 ** 6)
    W, bound = LR.table(model, u, norms)
    assert (np.abs(LR.count(u, v, cv, 6, 2, c) - W) <= 1e-13 * np.maximum(bound, 1e-300)).all()


def test_reverse_complement_and_canonical_codes(gp):
    for L in range(1, 10):
        u = np.arange(4 ** L, dtype=np.uint32)
        assert gp.lmer_rc(u, L).astype(np.int64).tolist() == LR.rc_codes(u, L).tolist()
        can = gp.canonical_codes(L)
        assert len(can) == (4 ** L + (4 ** (L // 2) if L % 2 == 0 else 0)) // 2
        text = gp.lmer_text(can, L)
        assert text == sorted(text) and len(set(text)) == len(text)
    assert gp.lmer_text(np.array([0, 27, 4 ** 3 - 1], np.uint32), 3) == ["AAA", "CGT", "TTT"]


# ------------------------------------------------------------------ weights file
def _table(gp, L=5, t=4, seed=2):
    rng = np.random.default_rng(seed)
    u = np.arange(4 ** L, dtype=np.uint32)
    W = rng.standard_normal(4 ** L) * 10.0 ** rng.integers(-300, 300, size=4 ** L)
    can = np.minimum(u, gp.lmer_rc(u, L))
    W = W[can]                                     # W[u] == W[rc(u)]
    W[0] = W[4 ** L - 1] = -0.0
    W[1] = W[gp.lmer_rc(np.array([1], np.uint32), L)[0]] = 5e-324
    k, d = (1, 1) if L < 4 else (3, 2)
    return gp.LmerTable(W, t, L, k, d, 50, 50.0, -1.5e-7)


@pytest.mark.parametrize("L", [2, 3, 5, 6])
def test_weights_file_round_trips_bit_for_bit(gp, tmp_path, L):
    tab = _table(gp, L, 0)
    path = str(tmp_path / "w.txt")
    tab.save(path)
    got = gp.load_lmer_table(path)
    assert got.W.tobytes() == tab.W.tobytes()
    assert (got.kernel_type, got.L, got.k, got.d, got.M, got.H, got.rho) == (0, L, tab.k, tab.d, 50, 50.0, -1.5e-7)
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = [x for x in lines[:-1] if x.startswith("#")]
    body = lines[len(head):-1]
    assert head[0] == "# format gkmqc-lmer-weights-1"
    assert sorted(x.split(" ")[1] for x in head) == sorted(("format", "kernel_type", "L", "k", "d", "M", "H", "rho"))
    assert len(body) == (4 ** L + (4 ** (L // 2) if L % 2 == 0 else 0)) // 2
    names = [x.split("\t")[0] for x in body]
    assert names == sorted(names) and names[0] == "A" * L
    for x in body:
        name, w = x.split("\t")
        code = 0
        for ch in name:
            code = 4 * code + "ACGT".index(ch)
        assert code <= LR.rc_codes([code], L)[0]
        assert w == repr(float(tab.W[code]))
    assert not os.path.exists(path + ".tmp")


def _edit(path, fn):
    lines = open(path).read().split("\n")[:-1]
    lines = fn(lines)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _swap_first_body_lmer(lines, new):
    i = next(j for j, x in enumerate(lines) if not x.startswith("#"))
    lines[i] = new + "\t" + lines[i].split("\t")[1]
    return lines


REFUSALS = {
    "drop_line": (lambda ls: ls[:-1], "l-mer lines"),
    "extra_line": (lambda ls: ls + ["TTTTT\t1.0"], "l-mer lines"),
    "non_canonical": (lambda ls: _swap_first_body_lmer(ls, "TTTTT"), "not canonical"),
    "repeated": (lambda ls: _swap_first_body_lmer(ls, "AAAAC"), "given twice"),
    "bad_char": (lambda ls: _swap_first_body_lmer(ls, "AANAA"), "other than A, C, G, T"),
    "lower_case": (lambda ls: _swap_first_body_lmer(ls, "aaaaa"), "other than A, C, G, T"),
    "short_lmer": (lambda ls: _swap_first_body_lmer(ls, "AAAA"), "l-mer of 5 bases"),
    "bad_weight": (lambda ls: [x if i != 9 else x.split("\t")[0] + "\tone" for i, x in enumerate(ls)], "one"),
    "missing_key": (lambda ls: [x for x in ls if not x.startswith("# rho ")], "missing key"),
    "repeated_key": (lambda ls: ls[:1] + ls[:1] + ls[1:], "given twice"),
    "unknown_key": (lambda ls: ["# gamma 1.0"] + ls, "header"),
    "bad_format": (lambda ls: ["# format gkmqc-lmer-weights-0"] + ls[1:], "format"),
    "rbf": (lambda ls: [("# kernel_type 5" if x.startswith("# kernel_type") else x) for x in ls], "RBF"),
    "bad_params": (lambda ls: [("# d 9" if x.startswith("# d ") else x) for x in ls], "rejected"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_weights_file_refusals(gp, tmp_path, case):
    path = str(tmp_path / "w.txt")
    _table(gp, 5).save(path)
    fn, reason = REFUSALS[case]
    _edit(path, fn)
    with pytest.raises(gp.ModelError, match=reason):
        gp.load_lmer_table(path)


def test_table_refuses_rbf_and_a_wrong_size(gp):
    with pytest.raises(gp.ModelError):
        gp.LmerTable(np.zeros(4 ** 5), 3, 5, 3, 2, 50, 50.0, 0.0)
    with pytest.raises(gp.ModelError):
        gp.LmerTable(np.zeros(4 ** 5 - 1), 4, 5, 3, 2, 50, 50.0, 0.0)


def test_api_refuses_rbf_before_touching_a_device(gp):
    for t in (3, 5):
        with pytest.raises(gp.ModelError, match="RBF"):
            gp.lmer_weights(_model(gp, kernel_type=t), device=12345)


# ------------------------------------------------------------------ command line
def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


@pytest.mark.parametrize("case", ["rbf3", "rbf5", "bad_model", "missing_model"])
def test_weights_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    model, out = str(tmp_path / "m.txt"), str(tmp_path / "w.txt")
    kw = dict(rbf3=dict(kernel_type=3), rbf5=dict(kernel_type=5)).get(case, {})
    _model(gp, **kw).save(model)
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    r = _run("weights", "--device", "12345", model + ("x" if case == "missing_model" else ""), out)
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    if case.startswith("rbf"):
        assert "RBF" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


@pytest.mark.parametrize("case", ["short_query", "empty_file", "bad_block", "bad_table", "missing_table",
                                  "missing_query", "model_not_table"])
def test_predict_table_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    table, query, out = str(tmp_path / "w.txt"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    _table(gp, 5).save(table)
    if case == "model_not_table":
        _model(gp, L=5).save(table)
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGT" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    if case == "bad_table":
        _edit(table, lambda ls: ls[:-1])
    args = ["predict-table", "--device", "12345"] + (["--block", "0"] if case == "bad_block" else [])
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), table + ("x" if case == "missing_table" else ""),
                       out]))
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
