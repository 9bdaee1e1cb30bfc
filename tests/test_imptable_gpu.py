"""Per-base importance tables on the GPU (gkmhip_lmer_importance, gkmhip_lmer_explain, gkmhip_lmer_hyp,
gkmpredict.lmer_importance, explain_with_table, hypothetical_with_table): exact enumeration against a numpy count,
independence of the code range, trained models' tables against the CPU reference (tests/imp_ref.py) and the weight table,
explanations and hypothetical tables from the table against `explain` and `hypothetical`, and the command line from
`train` to `explain-table` / `hypothetical-table`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import imp_ref as IR
from tests import lmer_ref as LR
from tests.test_lmer_gpu import _classes, _ragged_queries

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")
SHAPES = {0: (10, 6, 3), 4: (10, 6, 3), 1: (7, 4, 3), 2: (7, 4, 3)}      # kernel type -> (L, k, d): an even and an odd L


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
    return {t: gp.train(POS, NEG, kernel_type=t, L=L, k=k, d=d) for t, (L, k, d) in SHAPES.items()}


@pytest.fixture(scope="module")
def itables(gp, models):
    return {t: gp.lmer_importance(m) for t, m in models.items()}


@pytest.fixture(scope="module")
def queries(dv):
    """per L: every 13th fixture sequence, ragged lengths from L to 2047 and one reverse complement"""
    seqs, _, _, _ = dv.read_problem(POS, NEG)
    return {L: [seqs[i] for i in range(0, len(seqs), 13)] + _ragged_queries(L) for L in (7, 10)}


@pytest.fixture(scope="module")
def explained(gp, itables, queries):
    """explain_with_table of every model's queries, computed once"""
    return {t: gp.explain_with_table(tab, queries[tab.L])[1] for t, tab in itables.items()}


@pytest.fixture(scope="module")
def hyped(gp, itables, queries):
    return {t: gp.hypothetical_with_table(tab, queries[tab.L])[1] for t, tab in itables.items()}


def _worst(got, want):
    """the largest |got - want| over a list of arrays.  A query whose G(x, x) is negative has no norm, and every route
    gives NaN for it (type 1's estimated weights at L=7 k=4 d=3 end in c_3 < 0, and the random 2 047-base query has
    enough 3-mismatch self pairs: sqrt(-134.8) in `score`, `explain` and `hypothetical` alike): NaN on both sides
    agrees, NaN on one side is infinitely wrong."""
    worst = 0.0
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape
        diff = np.abs(g - w)
        diff[np.isnan(g) & np.isnan(w)] = 0.0
        diff[np.isnan(g) != np.isnan(w)] = np.inf
        worst = max(worst, float(diff.max()))
    return worst


def _same(a, b):
    """bit for bit, but for the payload of a NaN (see _worst)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _importance(dv, L, d, share, v, cv, ranges):
    """gkmhip_lmer_importance over each [u0, u1) of `ranges` -> host (u1 - u0, L) array per range"""
    import torch
    ctx = dv.GramContext(0, L, max(0, L - d), d, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        d_v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).cuda()
        d_cv = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float64)).cuda()
        out = []
        for u0, u1 in ranges:
            V = torch.full((u1 - u0 + 1, L), -7.25, dtype=torch.float64, device="cuda")     # (+ 1: a guard row)
            ctx.lmer_importance(share, d_v.data_ptr(), d_cv.data_ptr(), len(v), u0, u1, V.data_ptr(), stream)
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_lmer_importance"
            assert ctx.last_comparisons() == 2.0 * len(v) * (u1 - u0)
            host = V.cpu().numpy()
            assert (host[-1] == -7.25).all()
            out.append(host[:-1])
        return out
    finally:
        ctx.close()


def _ranges(L, v):
    if L <= 8:
        return [(0, 4 ** L)]
    top = 4 ** L
    return [(0, 3000), (top // 3 - 777, top // 3 + 2222), (top - 2049, top),
            (max(0, int(v[5]) - 100), int(v[5]) + 157)]                      # around a class: hits at m = 0


def _check_exact(dv, L, d, v, cv, ranges):
    want = [IR.count_exact(np.arange(u0, u1), v, cv, L, d) for u0, u1 in ranges]
    total = 0.0
    for m in range(d + 1):
        got = _importance(dv, L, d, np.eye(d + 1)[m], v, cv, ranges)
        for (u0, u1), g, w in zip(ranges, got, want):
            assert np.array_equal(g, w[m]), (L, d, m, u0, u1, np.argwhere(g != w[m])[:5])
            total += np.abs(g).sum()
    return total


@pytest.mark.parametrize("L,d", [(2, 1), (5, 0), (5, 2), (8, 3), (8, 8), (10, 3), (12, 4), (12, 12),
                                 (3, 1), (4, 2), (6, 3), (7, 3), (9, 4), (11, 3)])         # (every L of k_lmer_importance<L>)
def test_exact_enumeration(dv, L, d):
    """share = e_m and integer cv: every V[u][i] is an exact integer count, bit for bit the numpy count (both strands; a
    palindrome credits its own row twice).  d = L is the dense case: every lane hits every class on both strands."""
    v, cv = _classes(L, 37, 10 * L + d)
    assert _check_exact(dv, L, d, v, cv, _ranges(L, v)) > 0
    if L % 2 == 0 and L <= 8:
        pal = v[v == LR.rc_codes(v, L)]
        assert len(pal) > 0
        V = _importance(dv, L, d, np.eye(d + 1)[0], pal[:1], [1.0], [(0, 4 ** L)])[0]
        assert (V[int(pal[0])] == 2.0).all() and V.sum() == 2.0 * L


@pytest.mark.parametrize("nv", [0, 1, 7, 8, 9, 37])
def test_exact_enumeration_around_the_request_size(dv, nv):
    """the classes stream eight per request: none, fewer than one request, exactly one, one and a tail"""
    L, d = 5, 2
    v, cv = _classes(L, 37, 3)
    keep = np.sort(np.random.default_rng(nv).permutation(len(v))[:nv])
    total = _check_exact(dv, L, d, v[keep], cv[keep], [(0, 4 ** L), (5, 70)])
    assert (total > 0) == (nv > 0)


def test_dense_hits_within_d_of_the_whole_range(dv):
    """classes inside a range of 64 codes that differ in the last three bases only: with d = 3 every lane of the wave
    hits every class on the forward strand"""
    L, d = 8, 3
    v = np.arange(4 ** L // 2, 4 ** L // 2 + 64, 5, dtype=np.uint32)
    cv = np.arange(1, len(v) + 1, dtype=np.float64)
    u0 = int(v[0])
    assert (LR.mismatches(np.arange(u0, u0 + 64), v, L) <= d).all()
    _check_exact(dv, L, d, v, cv, [(u0, u0 + 64), (u0 - 64, u0 + 192)])


def test_range_independence_and_symmetry(dv):
    """the whole table equals the same table computed in odd-sized pieces, and V[rc u][L-1-i] equals V[u][i], bit for
    bit"""
    rng = np.random.default_rng(17)
    L, d = 8, 3
    v, _ = _classes(L, 301, 5)
    cv = rng.standard_normal(len(v)) * 10.0 ** rng.integers(-3, 3, size=len(v))
    share = dv.mismatch_weights(4, L, 5)[:d + 1] / (L - np.arange(d + 1))
    whole = _importance(dv, L, d, share, v, cv, [(0, 4 ** L)])[0]
    cuts = [0, 1, 8, 263, 4093, 4094, 30001, 4 ** L - 5, 4 ** L]
    pieces = _importance(dv, L, d, share, v, cv, list(zip(cuts[:-1], cuts[1:])))
    assert np.concatenate(pieces).tobytes() == whole.tobytes()
    rc = LR.rc_codes(np.arange(4 ** L), L)
    assert whole.tobytes() == np.ascontiguousarray(whole[rc][:, ::-1]).tobytes()
    assert (np.abs(whole) > 0).mean() > 0.4


@pytest.mark.parametrize("t", [0, 1, 2, 4])
def test_trained_model_tables(gp, models, itables, t):
    """symmetry bit for bit over the whole table, two builds identical, sampled rows agree with the reference, row sums
    agree with the weight table"""
    model, tab = models[t], itables[t]
    L, k, d = SHAPES[t]
    assert tab.V.shape == (4 ** L, L) and tab.V.dtype == np.float64
    assert (tab.kernel_type, tab.L, tab.k, tab.d, tab.M, tab.H, tab.rho) == (t, L, k, d, model.M, model.H, model.rho)
    rc = LR.rc_codes(np.arange(4 ** L), L)
    assert tab.V.tobytes() == np.ascontiguousarray(tab.V[rc][:, ::-1]).tobytes()
    assert gp.lmer_importance(model).V.tobytes() == tab.V.tobytes()
    rng = np.random.default_rng(t)
    lm = gp.pack_lmers(model.seqs[3], L).astype(np.int64)
    sample = np.concatenate((rng.integers(0, 4 ** L, size=60), lm[:20], LR.rc_codes(lm[20:30], L)))
    want, bound = IR.table_by_sv(model, sample)
    err = np.abs(tab.V[sample] - want) - 1e-13 * bound
    print("type %d: worst |V - ref| / bound %.3g" % (t, np.max(np.abs(tab.V[sample] - want) / np.maximum(bound, 1e-300))))
    assert (err <= 0).all(), (t, err.max())
    assert (bound[60:].sum(1) > 0).all()
    W = gp.lmer_weights(model).W
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    print("type %d: worst |sum_i V - W| %.3g, tolerance %.3g" % (t, np.max(np.abs(tab.V.sum(1) - W)), tol))
    assert (np.abs(tab.V.sum(1) - W) <= tol).all()


@pytest.mark.parametrize("t", [0, 1, 2, 4])
def test_explain_with_table_matches_explain(gp, models, itables, queries, explained, t):
    model, tab, qs, got = models[t], itables[t], queries[SHAPES[t][0]], explained[t]
    names, want = gp.explain(model, qs)
    assert names == ["seq%d" % i for i in range(len(qs))]
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    for x, g in zip(qs, got):
        assert g.dtype == np.float64 and g.shape == (len(x),)
    worst = _worst(got, want)
    print("type %d: worst |explain_with_table - explain| %.3g, tolerance %.3g" % (t, worst, tol))
    assert worst <= tol
    assert sum(bool(np.isnan(g).any()) for g in got) <= 1 and max(np.abs(g[~np.isnan(g)]).max(initial=0.0) for g in got) > 0
    for block in (1, 3, len(qs)):
        _, again = gp.explain_with_table(tab, qs, block=block)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), block
    _, scores = gp.score_with_table(gp.lmer_weights(model), qs)
    worst = _worst([np.array([g.sum() for g in got])], [scores - model.rho])
    print("type %d: worst |sum_t E - (score - rho)| %.3g" % (t, worst))
    assert worst <= tol


@pytest.mark.parametrize("t", [0, 1, 2, 4])
def test_hypothetical_with_table(gp, models, itables, queries, explained, hyped, t):
    model, tab, qs, E, got = models[t], itables[t], queries[SHAPES[t][0]], explained[t], hyped[t]
    rng = np.random.default_rng(40 + t)
    mutants, where = [], []
    for q, (x, h, e) in enumerate(zip(qs, got, E)):
        assert h.dtype == np.float64 and h.shape == (len(x), 4)
        assert _same(h[np.arange(len(x)), x], e), q                          # the own column is the explanation
        for pos in {0, len(x) - 1, int(rng.integers(0, len(x)))}:
            b = int((x[pos] + 1 + rng.integers(0, 3)) % 4)
            y = x.copy()
            y[pos] = b
            mutants.append(y)
            where.append((q, pos, b))
    _, Ey = gp.explain_with_table(tab, mutants)
    for (q, pos, b), ey in zip(where, Ey):
        assert _same(got[q][pos, b], ey[pos]), (q, pos, b)                    # a mutant column is the mutant's explanation
    _, want = gp.hypothetical(model, qs)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    worst = _worst(got, want)
    print("type %d: worst |hypothetical_with_table - hypothetical| %.3g, tolerance %.3g" % (t, worst, tol))
    assert worst <= tol
    for block in (1, 3, len(qs)):
        _, again = gp.hypothetical_with_table(tab, qs, block=block)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), block


def test_gather_entries_describe_their_kernels(dv, gp, itables, queries):
    import torch
    tab, qs = itables[4], queries[10][:5]
    ctx = dv.GramContext(*tab.kernel_params(), device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        from gkmqc_amd import gkmquery
        flat = gkmquery._as_queries(qs)[0]
        ctx.set_sequences(flat, stream)
        V = torch.from_numpy(tab.V).cuda()
        nb, lmers = int(flat.off[-1]), sum(len(x) - tab.L + 1 for x in qs)
        xs = torch.ones(len(qs), dtype=torch.float64, device="cuda")
        E = torch.full((nb + 1,), -7.25, dtype=torch.float64, device="cuda")
        R = torch.full((nb + 1, 4), -7.25, dtype=torch.float64, device="cuda")
        ctx.lmer_explain(0, len(qs), V.data_ptr(), xs.data_ptr(), E.data_ptr(), stream)
        torch.cuda.synchronize()
        assert ctx.last_kernel_name() == "k_lmer_explain" and ctx.last_comparisons() == tab.L * lmers
        ctx.lmer_hyp(0, len(qs), V.data_ptr(), R.data_ptr(), stream)
        torch.cuda.synchronize()
        assert ctx.last_kernel_name() == "k_lmer_hyp" and ctx.last_comparisons() == 4 * tab.L * lmers
        E, R = E.cpu().numpy(), R.cpu().numpy()
        assert E[-1] == -7.25 and (R[-1] == -7.25).all()                       # nothing written behind the range
        assert R[np.arange(nb), flat.codes].tobytes() == E[:nb].tobytes()
        # a range inside the upload: the same values, at the range's own offsets
        E2 = torch.empty(nb, dtype=torch.float64, device="cuda")
        ctx.lmer_explain(2, 4, V.data_ptr(), xs.data_ptr(), E2.data_ptr(), stream)
        torch.cuda.synchronize()
        a, b = int(flat.off[2]), int(flat.off[4])
        assert E2.cpu().numpy()[:b - a].tobytes() == E[a:b].tobytes()
        with pytest.raises(dv.GkmError):
            ctx.lmer_explain(3, 3, V.data_ptr(), xs.data_ptr(), E2.data_ptr(), stream)
        with pytest.raises(dv.GkmError):
            ctx.lmer_hyp(0, len(qs) + 1, V.data_ptr(), R_ptr=E2.data_ptr(), stream=stream)
    finally:
        ctx.close()


def test_command_line_from_train_to_the_table_commands(gp, tmp_path):
    model, table = str(tmp_path / "m.txt"), str(tmp_path / "v.npz")
    query, out_e, out_h = str(tmp_path / "q.fa"), str(tmp_path / "e.txt"), str(tmp_path / "h.txt")
    rng = np.random.default_rng(2)
    qs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (7, 8, 57, 200, 600, 2047)]
    with open(query, "w") as f:
        for i, x in enumerate(qs):
            f.write(">q%d some description\n%s\n" % (i, gp.codes_to_text(x)))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)

    run("train", "-t", "4", "-L", "7", "-k", "4", "-d", "3", POS, NEG, model)
    run("importance-table", model, table)
    run("explain-table", "--block", "4", query, table, out_e)
    run("hypothetical-table", "--block", "5", query, table, out_h)
    tab = gp.load_importance_table(table)
    m = gp.load(model)
    assert tab.V.tobytes() == gp.lmer_importance(m).V.tobytes()
    assert (tab.kernel_type, tab.L, tab.k, tab.d, tab.M, tab.H, tab.rho) == (4, 7, 4, 3, m.M, m.H, m.rho)
    names, E = gp.read_explanation(out_e)
    assert names == ["q%d some description" % i for i in range(len(qs))]
    _, want = gp.explain_with_table(tab, qs)
    assert all(e.tobytes() == w.tobytes() for e, w in zip(E, want))
    names, H = gp.read_ism(out_h)
    assert names == ["q%d some description" % i for i in range(len(qs))]
    _, want = gp.hypothetical_with_table(tab, qs)
    assert all(h.tobytes() == w.tobytes() for h, w in zip(H, want))
