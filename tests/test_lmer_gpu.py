"""L-mer weight tables on the GPU (gkmhip_lmer_weights, gkmhip_lmer_score, gkmpredict.lmer_weights,
gkmpredict.score_with_table): exact enumeration against a numpy count, independence of the code range, trained models'
tables against the CPU reference (tests/lmer_ref.py), table scores against `score`, and the command line from `train` to
`predict-table`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import lmer_ref as LR

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


@pytest.fixture(scope="module")
def models(gp):
    return {t: gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3) for t in (0, 1, 2, 4)}


@pytest.fixture(scope="module")
def tables(gp, models):
    return {t: gp.lmer_weights(m) for t, m in models.items()}


def _classes(L, nv, seed):
    """nv distinct canonical codes, ascending, palindromes included where L is even; small integer weights"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 4 ** L, size=4 * nv)
    if L % 2 == 0:
        half = rng.integers(0, 4 ** (L // 2), size=3)
        u = np.concatenate((u, (half << L) | LR.rc_codes(half, L // 2)))     # palindromes: u == rc(u)
    v = np.unique(np.minimum(u, LR.rc_codes(u, L)))
    pal = v[v == LR.rc_codes(v, L)]
    v = np.unique(np.concatenate((rng.permutation(v)[:nv], pal)))
    cv = rng.integers(-7, 8, size=len(v)).astype(np.float64)
    cv[cv == 0] = 3.0
    return v.astype(np.uint32), cv


def _weights(dv, L, d, c, v, cv, ranges, k=None):
    """gkmhip_lmer_weights over each [u0, u1) of `ranges` into one output -> host array per range"""
    import torch
    k = max(0, L - d) if k is None else k
    ctx = dv.GramContext(0, L, k, d, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        d_v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).cuda()
        d_cv = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float64)).cuda()
        out = []
        for u0, u1 in ranges:
            W = torch.full((u1 - u0,), -7.25, dtype=torch.float64, device="cuda")
            ctx.lmer_weights(c, d_v.data_ptr(), d_cv.data_ptr(), len(v), u0, u1, W.data_ptr(), stream)
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_lmer_weights"
            assert ctx.last_comparisons() == 2.0 * len(v) * (u1 - u0)
            out.append(W.cpu().numpy())
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("L,d", [(2, 1), (5, 0), (5, 2), (8, 3), (8, 8), (10, 3), (12, 4), (12, 12)])
def test_exact_enumeration(dv, L, d):
    """c = e_m and integer cv: every W[u] is an exact integer count, bit for bit the numpy count (both strands; a
    palindrome counts twice)"""
    v, cv = _classes(L, 37, 10 * L + d)
    if L <= 8:
        ranges = [(0, 4 ** L)]
    else:
        top = 4 ** L
        ranges = [(0, 3000), (top // 3 - 777, top // 3 + 2222), (top - 2049, top)]
        ranges.append((max(0, int(v[5]) - 100), int(v[5]) + 157))                # around a class: hits at m = 0
    for m in range(d + 1):
        c = np.zeros(d + 1)
        c[m] = 1.0
        got = _weights(dv, L, d, c, v, cv, ranges)
        for (u0, u1), g in zip(ranges, got):
            want = LR.count(np.arange(u0, u1), v, cv, L, d, c)
            assert np.array_equal(g, want), (L, d, m, u0, u1, np.nonzero(g != want)[0][:5])
        if m == 0 and L <= 8:
            assert got[0][v.astype(np.int64)].min() != 0.0 or (cv == 0).any()
    if L % 2 == 0 and L <= 8:
        pal = v[v == LR.rc_codes(v, L)]
        assert len(pal) > 0
        c = np.zeros(d + 1)
        c[0] = 1.0
        W = _weights(dv, L, d, c, pal[:1], [1.0], [(0, 4 ** L)])[0]
        assert W[int(pal[0])] == 2.0 and W.sum() == 2.0


def test_range_independence(dv):
    """the whole table equals the same table computed in odd-sized pieces, bit for bit"""
    rng = np.random.default_rng(17)
    L, d = 8, 3
    v, _ = _classes(L, 301, 5)
    cv = rng.standard_normal(len(v)) * 10.0 ** rng.integers(-3, 3, size=len(v))
    c = dv.mismatch_weights(4, L, 5)[:d + 1]
    whole = _weights(dv, L, d, c, v, cv, [(0, 4 ** L)])[0]
    cuts = [0, 1, 8, 263, 4093, 4094, 30001, 4 ** L - 5, 4 ** L]
    pieces = _weights(dv, L, d, c, v, cv, list(zip(cuts[:-1], cuts[1:])))
    assert np.concatenate(pieces).tobytes() == whole.tobytes()
    u = np.arange(4 ** L)
    assert whole.tobytes() == whole[LR.rc_codes(u, L)].tobytes()
    assert (np.abs(whole) > 0).mean() > 0.5


@pytest.mark.parametrize("t", [0, 1, 2, 4])
def test_trained_model_tables(gp, models, tables, t):
    """W[u] == W[rc(u)] bit for bit over the whole table, two builds identical, sampled codes agree with the reference"""
    model, tab = models[t], tables[t]
    L = model.L
    assert tab.W.shape == (4 ** L,) and tab.W.dtype == np.float64
    assert (tab.kernel_type, tab.L, tab.k, tab.d, tab.M, tab.H, tab.rho) == \
        (t, 10, 6, 3, model.M, model.H, model.rho)
    u = np.arange(4 ** L)
    assert tab.W.tobytes() == tab.W[LR.rc_codes(u, L)].tobytes()
    again = gp.lmer_weights(model)
    assert again.W.tobytes() == tab.W.tobytes()
    rng = np.random.default_rng(t)
    lm = gp.pack_lmers(model.seqs[3], L).astype(np.int64)
    sample = np.concatenate((rng.integers(0, 4 ** L, size=150), lm[:40], LR.rc_codes(lm[40:60], L)))
    want, bound = LR.table(model, sample)
    assert (np.abs(tab.W[sample] - want) <= 1e-13 * bound).all(), (t, np.max(np.abs(tab.W[sample] - want) - 1e-13 * bound))
    assert (bound[150:] > 0).all()


def _ragged_queries(L=10, seed=23):
    rng = np.random.default_rng(seed)
    qs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (L, L + 1, 37, 200, 600, 1023, 2047)]
    return qs + [(3 - qs[4])[::-1].copy()]


@pytest.mark.parametrize("t", [0, 1, 2, 4])
def test_table_scores_match_score(gp, models, tables, t):
    model, tab = models[t], tables[t]
    from gkmqc_amd import device as dv
    queries, _, _, _ = dv.read_problem(POS, NEG)
    queries = [queries[i] for i in range(0, len(queries), 13)] + _ragged_queries()
    names, got = gp.score_with_table(tab, queries)
    assert names == ["seq%d" % i for i in range(len(queries))]
    _, want = gp.score(model, queries)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    assert got.dtype == np.float64 and got.shape == (len(queries),)
    assert (np.abs(got - want) <= tol).all(), (t, np.max(np.abs(got - want)), tol)
    for block in (1, 3, len(queries)):
        _, again = gp.score_with_table(tab, queries, block=block)
        assert again.tobytes() == got.tobytes(), block


def test_command_line_from_train_to_predict_table(gp, tmp_path):
    model, weights = str(tmp_path / "m.txt"), str(tmp_path / "w.txt")
    query, out_t, out_p = str(tmp_path / "q.fa"), str(tmp_path / "t.txt"), str(tmp_path / "p.txt")
    rng = np.random.default_rng(2)
    with open(query, "w") as f:
        for i, n in enumerate((10, 57, 200, 600, 2047)):
            f.write(">q%d some description\n%s\n" % (i, gp.codes_to_text(rng.integers(0, 4, size=n, dtype=np.uint8))))
        with open(POS) as p:
            f.write(p.read())

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)

    run("train", "-t", "4", "-L", "10", "-k", "6", "-d", "3", POS, NEG, model)
    run("weights", model, weights)
    run("predict-table", "--block", "7", query, weights, out_t)
    run("predict", query, model, out_p)
    lt = [x.split("\t") for x in open(out_t).read().split("\n")[:-1]]
    lp = [x.split("\t") for x in open(out_p).read().split("\n")[:-1]]
    assert [a[0] for a in lt] == [a[0] for a in lp] and len(lt) == 5 + 150
    m = gp.load(model)
    tol = 1e-12 * np.abs(m.dual_coef()).sum()
    for a, b in zip(lt, lp):
        assert abs(float(a[1]) - float(b[1])) <= tol, (a, b)
        assert a[1] == repr(float(a[1]))
    tab = gp.load_lmer_table(weights)
    assert tab.W.tobytes() == gp.lmer_weights(m).W.tobytes()
    assert (tab.kernel_type, tab.L, tab.k, tab.d, tab.M, tab.H, tab.rho) == (4, 10, 6, 3, m.M, m.H, m.rho)
