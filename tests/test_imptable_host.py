"""Per-base importance tables without a GPU: the CPU reference (tests/imp_ref.py) against the explanation reference and the
weight-table reference, explanations gathered from the reference table, the table file format, and the refusals of
`lmer_importance` and of the `importance-table`, `explain-table` and `hypothetical-table` command lines
(gkmqc_amd/gkmpredict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as R
from tests import helpers
from tests import imp_ref as IR
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


def _bases(code, L):
    return np.array([(int(code) >> (2 * (L - 1 - i))) & 3 for i in range(L)], dtype=np.uint8)


CASES = [(0, 5, 2, 2), (1, 6, 3, 2), (2, 6, 4, 1), (4, 6, 3, 3), (4, 5, 1, 4), (2, 7, 4, 3)]


@pytest.fixture(scope="module")
def refs(gp):
    """per case: the model, its support vectors' norms and the reference table over every code, computed once"""
    out = {}
    for t, L, k, d in CASES:
        model = _model(gp, t, L, k, d)
        norms = R.sv_norms(model)
        V, bound = IR.table(model, np.arange(4 ** L), norms)
        out[(t, L, k, d)] = (model, norms, V, bound)
    return out


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_reference_table_is_the_explanation_of_one_lmer(refs, t, L, k, d):
    """explain_ref.explanation of the L-base sequence u, times sq_u / w_u, is V(u, .): the check §5g makes for W"""
    model, norms, V, bound = refs[(t, L, k, d)]
    w_u = float(R.weights(t, 1, model.M, model.H)[0])
    rng = np.random.default_rng(L + d)
    lm = R.pack(model.seqs[1], L).astype(np.int64)
    for code in np.concatenate(([0, 4 ** L - 1], rng.integers(0, 4 ** L, size=40), lm[:6], LR.rc_codes(lm[6:10], L))):
        x = _bases(code, L)
        E, _ = R.explanation(model, x, norms)
        want = E * R.self_norm(x, t, L, k, d, model.M, model.H) / w_u
        assert (np.abs(V[code] - want) <= 1e-13 * np.maximum(bound[code], 1e-300)).all(), (t, L, d, int(code))
    assert (bound[lm[:6]].sum(1) > 0).all()


@pytest.mark.parametrize("t,L,k,d", CASES[:4])
def test_reference_by_support_vector_agrees_with_the_classes(refs, t, L, k, d):
    model, norms, V, bound = refs[(t, L, k, d)]
    u = np.random.default_rng(t).integers(0, 4 ** L, size=300)
    V2, bound2 = IR.table_by_sv(model, u, norms)
    assert (np.abs(V2 - V[u]) <= 1e-13 * np.maximum(bound[u], 1e-300)).all()
    assert (np.abs(bound2 - bound[u]) <= 1e-12 * np.maximum(bound[u], 1e-300)).all()


def test_exact_count_agrees_with_the_float_count():
    rng = np.random.default_rng(4)
    L, d = 4, 2
    v = np.unique(rng.integers(0, 4 ** L, size=30))
    cv = rng.integers(-5, 6, size=len(v)).astype(np.float64)
    u = np.arange(4 ** L)
    exact = IR.count_exact(u, v, cv, L, d)
    for m in range(d + 1):
        assert np.array_equal(exact[m], IR.count(u, v, cv, L, d, np.eye(d + 1)[m]))
    assert np.abs(exact).sum(axis=(1, 2)).min() > 0


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_reference_rows_sum_to_the_weight_table(refs, t, L, k, d):
    model, norms, V, bound = refs[(t, L, k, d)]
    u = np.arange(4 ** L)
    W, wbound = LR.table(model, u, norms)
    assert (np.abs(V.sum(1) - W) <= 1e-13 * np.maximum(wbound, 1e-300)).all()
    assert (np.abs(bound.sum(1) - wbound) <= 1e-12 * np.maximum(wbound, 1e-300)).all()
    assert (np.abs(W) > 0).mean() > 0.5


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_reference_table_is_symmetric_under_reverse_complement(refs, t, L, k, d):
    """V(rc u, L-1-i) == V(u, i): the two strands swap roles, and their terms meet in one commutative add"""
    _, _, V, _ = refs[(t, L, k, d)]
    rc = LR.rc_codes(np.arange(4 ** L), L)
    assert np.array_equal(V[rc][:, ::-1], V)


@pytest.mark.parametrize("t,L,k,d", CASES)
def test_explanations_gathered_from_the_reference_table(refs, t, L, k, d):
    """types 0, 1, 2 and 4, even and odd L, ragged queries down to length L"""
    model, norms, V, _ = refs[(t, L, k, d)]
    rng = np.random.default_rng(7 * L + t)
    queries = [_rand(rng, n) for n in (L, L + 1, 2 * L - 1, 37, 120)]
    queries.append(np.concatenate((model.seqs[1][:20], (3 - model.seqs[2])[::-1])))
    for x in queries:
        got = IR.explain_from_table(model, lambda u: V[u], x)
        want, bound = R.explanation(model, x, norms)
        assert got.shape == want.shape
        assert (np.abs(got - want) <= 1e-13 * np.maximum(bound, 1e-300)).all(), (t, L, d, len(x))
    assert np.abs(want).max() > 0


# ------------------------------------------------------------------ table file
def _table(gp, L=5, t=4, seed=2, k=None, d=None):
    """a table with the symmetry a real one has, values over the whole double range, -0.0 and a denormal"""
    rng = np.random.default_rng(seed)
    u = np.arange(4 ** L, dtype=np.uint32)
    rc = gp.lmer_rc(u, L).astype(np.int64)
    V = rng.standard_normal((4 ** L, L)) * 10.0 ** rng.integers(-300, 300, size=(4 ** L, L))
    V[0, 0] = -0.0
    V[1, 2 % L] = 5e-324
    low = u <= rc
    V[rc[low]] = V[low][:, ::-1]
    pal = u == rc
    V[pal] = np.where(np.arange(L) < L // 2, V[pal], V[pal][:, ::-1])
    kk, dd = (1, 1) if L < 4 else (3, 2)
    return gp.LmerImportanceTable(V, t, L, kk if k is None else k, dd if d is None else d, 50, 50.0, -1.5e-7)


@pytest.mark.parametrize("L", [2, 3, 5, 6])
def test_table_file_round_trips_bit_for_bit(gp, tmp_path, L):
    tab = _table(gp, L, 0)
    rc = gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L).astype(np.int64)
    assert tab.V[rc][:, ::-1].tobytes() == tab.V.tobytes()
    path = str(tmp_path / "table_without_suffix")
    tab.save(path)
    assert os.path.isfile(path) and not os.path.exists(path + ".npz") and not os.path.exists(path + ".tmp")
    got = gp.load_importance_table(path)
    assert got.V.tobytes() == tab.V.tobytes() and got.V.shape == (4 ** L, L) and got.V.dtype == np.float64
    assert (got.kernel_type, got.L, got.k, got.d, got.M, got.H, got.rho) == (0, L, tab.k, tab.d, 50, 50.0, -1.5e-7)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(("format", "kernel_type", "L", "k", "d", "M", "H", "rho", "V"))
        assert str(z["format"]) == "gkmqc-lmer-importance-1"
        can = gp.canonical_codes(L)
        assert z["V"].shape == (len(can), L) and z["V"].tobytes() == tab.V[can].tobytes()
    import zipfile
    with zipfile.ZipFile(path) as zf:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in zf.infolist())


def _rewrite(path, **changes):
    """the file's members with some replaced (a value), dropped (None) or added"""
    with np.load(path, allow_pickle=False) as z:
        members = {key: z[key] for key in z.files}
    for key, val in changes.items():
        if val is None:
            del members[key]
        else:
            members[key] = val(members) if callable(val) else val
    with open(path, "wb") as f:
        np.savez(f, **members)


FILE_REFUSALS = {
    "bad_format": (dict(format=np.array("gkmqc-lmer-importance-0")), "format"),
    "format_not_text": (dict(format=np.int64(1)), "format"),
    "weights_format": (dict(format=np.array("gkmqc-lmer-weights-1")), "format"),
    "missing_rho": (dict(rho=None), "missing key"),
    "missing_V": (dict(V=None), "missing key"),
    "missing_format": (dict(format=None), "missing key"),
    "unknown_key": (dict(gamma=np.float64(1.0)), "do not belong"),
    "rows_dropped": (dict(V=lambda m: m["V"][:-1]), "expected float64"),
    "rows_added": (dict(V=lambda m: np.concatenate((m["V"], m["V"][:1]))), "expected float64"),
    "whole_table": (dict(V=lambda m: np.zeros((4 ** 5, 5))), "expected float64"),
    "transposed": (dict(V=lambda m: np.ascontiguousarray(m["V"].T)), "expected float64"),
    "flat": (dict(V=lambda m: m["V"].reshape(-1)), "expected float64"),
    "float32": (dict(V=lambda m: np.zeros(m["V"].shape, np.float32)), "expected float64"),
    "L_is_an_array": (dict(L=np.array([5, 5])), "L must be one integer"),
    "L_is_a_float": (dict(L=np.float64(5.0)), "L must be one integer"),
    "H_is_an_integer": (dict(H=np.int64(50)), "H must be one float"),
    "bad_params": (dict(d=np.int64(9)), "rejected"),
    "rbf3": (dict(kernel_type=np.int64(3)), "RBF"),
    "rbf5": (dict(kernel_type=np.int64(5)), "RBF"),
    "k0": (dict(k=np.int64(0), d=np.int64(5)), "k = 0"),
    "bad_M": (dict(M=np.int64(256)), "M must lie"),
    "rho_not_finite": (dict(rho=np.float64("nan")), "finite"),
}


@pytest.mark.parametrize("case", sorted(FILE_REFUSALS))
def test_table_file_refusals(gp, tmp_path, case):
    path = str(tmp_path / "v.npz")
    _table(gp, 5).save(path)
    changes, reason = FILE_REFUSALS[case]
    _rewrite(path, **changes)
    with pytest.raises(gp.ModelError, match=reason):
        gp.load_importance_table(path)


def test_table_file_refuses_an_asymmetric_palindrome_row(gp, tmp_path):
    path = str(tmp_path / "v.npz")
    _table(gp, 4, k=2, d=2).save(path)
    can = gp.canonical_codes(4)
    row = int(np.nonzero(can == gp.lmer_rc(can, 4))[0][0])

    def bend(members):
        V = members["V"].copy()
        V[row, 0], V[row, 3] = 1.0, 2.0
        return V

    _rewrite(path, V=bend)
    with pytest.raises(gp.ModelError, match="mirror image"):
        gp.load_importance_table(path)


@pytest.mark.parametrize("case", ["empty", "text", "truncated", "pickled"])
def test_table_file_refuses_what_is_no_archive(gp, tmp_path, case):
    path = str(tmp_path / "v.npz")
    _table(gp, 5).save(path)
    if case == "empty":
        open(path, "wb").close()
    elif case == "text":
        _model(gp, L=5).save(path)
    elif case == "truncated":
        data = open(path, "rb").read()
        with open(path, "wb") as f:
            f.write(data[:len(data) // 2])
    else:
        with open(path, "wb") as f:
            np.savez(f, format=np.array("gkmqc-lmer-importance-1"), V=np.array([{"a": 1}], dtype=object))
    with pytest.raises(gp.ModelError, match="v.npz"):
        gp.load_importance_table(path)


def test_table_refuses_rbf_k0_and_a_wrong_shape(gp):
    for t in (3, 5):
        with pytest.raises(gp.ModelError, match="RBF"):
            gp.LmerImportanceTable(np.zeros((4 ** 5, 5)), t, 5, 3, 2, 50, 50.0, 0.0)
    with pytest.raises(gp.ModelError, match="k = 0"):
        gp.LmerImportanceTable(np.zeros((4 ** 5, 5)), 0, 5, 0, 5, 50, 50.0, 0.0)
    for shape in ((4 ** 5,), (4 ** 5, 4), (4 ** 5 - 1, 5), (5, 4 ** 5)):
        with pytest.raises(gp.ModelError, match="needs"):
            gp.LmerImportanceTable(np.zeros(shape), 4, 5, 3, 2, 50, 50.0, 0.0)


def test_api_refuses_rbf_and_k0_before_touching_a_device(gp):
    for t in (3, 5):
        with pytest.raises(gp.ModelError, match="RBF"):
            gp.lmer_importance(_model(gp, kernel_type=t), device=12345)
    with pytest.raises(gp.ModelError, match="k = 0"):
        gp.lmer_importance(_model(gp, kernel_type=0, L=6, k=0, d=6), device=12345)


def test_queries_are_checked_before_touching_a_device(gp):
    tab = _table(gp, 5)
    for fn in (gp.explain_with_table, gp.hypothetical_with_table):
        with pytest.raises(gp.ModelError, match="shorter than L"):
            fn(tab, [np.zeros(9, np.uint8), np.zeros(4, np.uint8)], device=12345)
        with pytest.raises(gp.ModelError, match="no query"):
            fn(tab, [], device=12345)


# ------------------------------------------------------------------ command line
def _run(*args):
    return subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                          capture_output=True, text=True)


@pytest.mark.parametrize("case", ["rbf3", "rbf5", "k0", "bad_model", "missing_model"])
def test_importance_table_refusals_exit_1_and_write_nothing(gp, tmp_path, case):
    model, out = str(tmp_path / "m.txt"), str(tmp_path / "v.npz")
    kw = dict(rbf3=dict(kernel_type=3), rbf5=dict(kernel_type=5), k0=dict(kernel_type=0, L=6, k=0, d=6)).get(case, {})
    _model(gp, **kw).save(model)
    if case == "bad_model":
        with open(model, "a") as f:
            f.write("extra line\n")
    r = _run("importance-table", "--device", "12345", model + ("x" if case == "missing_model" else ""), out)
    assert r.returncode == 1, (case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    if case.startswith("rbf"):
        assert "RBF" in r.stderr
    if case == "k0":
        assert "k = 0" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


_TABLE_CASES = ["short_query", "empty_file", "bad_block", "bad_table", "missing_table", "missing_query",
                "model_not_table", "weights_not_table", "rbf_table", "k0_table"]


# (both commands share one code path up to the compute function: the second takes the cases that reach it or name it)
@pytest.mark.parametrize("cmd,case", [("explain-table", c) for c in _TABLE_CASES] +
                         [("hypothetical-table", c) for c in ("short_query", "bad_block", "bad_table", "rbf_table",
                                                              "k0_table")])
def test_table_commands_refusals_exit_1_and_write_nothing(gp, tmp_path, cmd, case):
    table, query, out = str(tmp_path / "v.npz"), str(tmp_path / "q.fa"), str(tmp_path / "out.txt")
    _table(gp, 5).save(table)
    if case == "model_not_table":
        _model(gp, L=5).save(table)
    elif case == "weights_not_table":
        gp.LmerTable(np.zeros(4 ** 5), 4, 5, 3, 2, 50, 50.0, 0.0).save(table)
    elif case == "bad_table":
        _rewrite(table, V=lambda m: m["V"][:-1])
    elif case == "rbf_table":
        _rewrite(table, kernel_type=np.int64(5))
    elif case == "k0_table":
        _rewrite(table, kernel_type=np.int64(0), k=np.int64(0), d=np.int64(5))
    with open(query, "w") as f:
        f.write("" if case == "empty_file" else ">a\nACGTACGTACGTAC\n>b\n" + ("ACGT" if case == "short_query" else
                                                                             "GGGTTTACCAGTAC") + "\n")
    args = [cmd, "--device", "12345"] + (["--block", "0"] if case == "bad_block" else [])
    r = _run(*(args + [query + ("x" if case == "missing_query" else ""), table + ("x" if case == "missing_table" else ""),
                       out]))
    assert r.returncode == 1, (cmd, case, r.stdout, r.stderr)
    assert "gkmpredict: error:" in r.stderr
    if case == "rbf_table":
        assert "RBF" in r.stderr
    if case == "k0_table":
        assert "k = 0" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
