"""The interpretation kernels (k_explain, k_ism, k_ism<true>, k_ism_self_base + k_ism_self, k_lmer_weights, k_lmer_score)
on dense-hit input (tests/dense_inputs.py): homopolymers, short-period repeats, copies and near copies of support vectors,
at weights up to 255.  On iid bases a hit is the rare event (2 % of the pairs at L = 10, d = 3); here it is the common
one, so the uint32 tallies grow to 1.58e9, all 64 lanes add to neighbouring LDS words in one instruction, the hit
queues of k_ism fill to every depth of their design, and support vectors at the edges of a chunk carry weight.  Every
tally is compared bit for bit with the CPU references (explain_ref, ism_ref, hyp_ref, lmer_ref), which
tests/test_dense_host.py checks against closed forms.

The entry points of gkmpredict are compared with each other on the same queries: inside the no-wrap domain (every
profile of the query, of its mutants and of the support vectors below 2^31) against `score`; beyond it `score` keeps
the reference's 32-bit wrap (pinned to the oracle) and explain / ism / hypothetical / the l-mer tables are exact, which
is asserted against an exact score formed from the reference's 64-bit profiles."""
import types

import numpy as np
import pytest

from tests import dense_inputs as D
from tests import explain_ref as E
from tests import hyp_ref as HR
from tests import ism_ref as R
from tests import lmer_ref as LR
from tests.test_hyp_gpu import _Launcher as HypLauncher
from tests.test_ism_gpu import _Launcher as IsmLauncher
from tests.test_ism_gpu import _split, _unit
from tests.test_lmer_gpu import _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


class ExplainLauncher:
    """test_explain_gpu._launch on one context kept over many launches"""

    def __init__(self, dv, params, seqs):
        import torch
        self.torch = torch
        t, L, k, d, M, H = params
        self.seqs = seqs
        self.ctx = dv.GramContext(t, L, k, d, M, H, 1.0, 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ctx.set_sequences(seqs, self.stream)

    def block(self, rows, c0, c1, share, coef):
        torch = self.torch
        nb = sum(len(s) for s in self.seqs[c0:c1])
        out = torch.full((nb,), -7.25, dtype=torch.float64, device="cuda")
        d_coef = torch.tensor(np.asarray(coef, dtype=np.float64), device="cuda")
        self.ctx.explain_block(rows, c0, c1, share, d_coef.data_ptr(), None, out.data_ptr(), self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_explain"
        return out.cpu().numpy()

    def close(self):
        self.ctx.close()


def _params(weights, shape):
    t, M, H = D.WEIGHTS[weights]
    L, k, d = shape
    return (t, L, k, d, M, H)


def _explainable(L, k, d):
    return k > 0 and d < L


def _check_explain(run, rows, c0, queries, want, d, tag):
    """want[qi]: the reference's H (len(x), d + 1) for the rows, coef 1"""
    for m in range(d + 1):
        got = run.block(rows, c0, c0 + len(queries), _unit(d + 1, m), [1.0] * len(rows))
        for qi, g in enumerate(_split(got, queries, ())):
            assert np.array_equal(g, want[qi][:, m].astype(np.float64)), tag + ("H", m, qi)


def _check_ism(run, rows, c0, queries, want, profiles, L, d, tag):
    """want[qi] = (U, B) of the reference; profiles[qi] = P_m(x, s) or None"""
    mb = min(d + 1, L)
    c1 = c0 + len(queries)
    ones = [1.0] * len(rows)
    for m in range(d + 1):
        out, base = run.block(rows, c0, c1, _unit(d + 1, m), _unit(d + 1, None), _unit(d + 1, m), ones)
        for qi, (g, x) in enumerate(zip(_split(out, queries, (4,)), queries)):
            w = np.repeat(want[qi][0][:, m:m + 1].astype(np.float64), 4, axis=1)
            w[np.arange(len(x)), x] = 0.0
            assert np.array_equal(g, w), tag + ("U", m, qi)
            if profiles is not None:
                assert base[qi] == float(profiles[qi][m]), tag + ("P", m, qi, base[qi], profiles[qi][m])
    for m in range(1, mb + 1):
        out, _ = run.block(rows, c0, c1, _unit(d + 1, None), _unit(d + 1, m - 1), _unit(d + 1, None), ones)
        for qi, g in enumerate(_split(out, queries, (4,))):
            assert np.array_equal(g, want[qi][1][:, m].astype(np.float64)), tag + ("B", m, qi)


def _check_hyp(run, rows, c0, queries, want, d, tag):
    for m in range(d + 1):
        out = run.block(rows, c0, c0 + len(queries), _unit(d + 1, m), [1.0] * len(rows))
        for qi, (g, x) in enumerate(zip(_split(out, queries, (4,)), queries)):
            w = HR.raw_from_tallies(x, want[qi][0], want[qi][1], _unit(d + 1, m), d)
            assert np.array_equal(g, w), tag + ("hyp", m, qi)


SMALL = [("w50", (10, 6, 3)), ("w254", (10, 6, 3)), ("w255", (10, 6, 3)), ("unit", (10, 6, 3)), ("w254", (12, 4, 8)),
         ("w255", (12, 8, 4)), ("w254", (12, 1, 11)), ("unit", (5, 0, 5)), ("w50", (5, 2, 3))]


@pytest.mark.parametrize("weights,shape", SMALL, ids=["%s-%d-%d-%d" % ((w,) + s) for w, s in SMALL])
def test_all_against_all_tallies_are_exact(dv, weights, shape):
    """every (query, support vector) pair of the small dense set, one support vector per launch, coef 1, unit fold
    vectors: k_explain's H[m], k_ism's U[m], B[m] and P_m(x, s), k_ism<true>'s four columns, bit for bit"""
    t, L, k, d, M, H = params = _params(weights, shape)
    named = D.small_set(L, d)
    seqs = [x for _, x in named]
    n = len(seqs)
    runs = [IsmLauncher(dv, params, seqs)]
    if _explainable(L, k, d):
        runs += [ExplainLauncher(dv, params, seqs), HypLauncher(dv, params, seqs)]
    try:
        biggest = 0
        for si, s in enumerate(seqs):
            tag = (weights, shape, named[si][0])
            UB = [R.tallies(x, s, t, L, d, M, H) for x in seqs]
            P = [R.profile(x, s, t, L, d, M, H) for x in seqs]
            biggest = max([biggest] + [int(u.max()) for u, _ in UB] + [int(b.max()) for _, b in UB])
            _check_ism(runs[0], [si], 0, seqs, UB, P, L, d, tag)
            if len(runs) > 1:
                Hs = [E.tallies(x, s, t, L, d, M, H) for x in seqs]
                assert all(np.array_equal(h, u) for h, (u, _) in zip(Hs, UB))      # (the two references agree)
                _check_explain(runs[1], [si], 0, seqs, Hs, d, tag)
                _check_hyp(runs[2], [si], 0, seqs, UB, d, tag)
    finally:
        for r in runs:
            r.close()
    print("%s %s: %d sequences, largest reference tally %d" % (weights, shape, n, biggest))
    assert biggest > 0


@pytest.mark.parametrize("shape", [(12, 4, 8), (8, 2, 6)])
def test_a_dense_stretch_across_the_tile_boundary(dv, shape):
    """a tiled shape: 2 047-base queries with (AT)n and poly-A from 60 bases before to 60 bases after the tile boundary,
    against support vectors that hit them on both strands"""
    L, k, d = shape
    params = _params("w254", shape)
    t, _, _, _, M, H = params
    tile = D.ism_tile(L, d)
    assert tile == {(12, 8): 1094, (8, 6): 1407}[(L, d)]
    queries = []
    for unit in ((D.A, D.T), (D.A,)):
        x = D.spliced(D.MAX_LEN, L, 50 + len(unit))
        x[tile - 60:tile + 60] = D.repeat(unit, 120)
        queries.append(x)
    svs = [D.repeat((D.A, D.T), 40), D.homopolymer(D.T, 30)]
    seqs = svs + queries
    irun, hrun = IsmLauncher(dv, params, seqs), HypLauncher(dv, params, seqs)
    try:
        for si, s in enumerate(svs):
            UB = [R.tallies(x, s, t, L, d, M, H) for x in queries]
            P = [R.profile(x, s, t, L, d, M, H) for x in queries]
            assert all(u[tile - 5:tile + 5].sum() > 0 for u, _ in UB)
            _check_ism(irun, [si], len(svs), queries, UB, P, L, d, (shape, si))
            _check_hyp(hrun, [si], len(svs), queries, UB, d, (shape, si))
    finally:
        irun.close()
        hrun.close()


def test_tallies_at_the_top_of_their_range(dv):
    """2 047-base homopolymers at L = 12 with every weight 254 (and 255): the interior tallies are 12 x 2 036 x 254^2 =
    1 576 254 912, 0.367 of 2^32 and far above 2^24 (a float conversion), and the weight product of a hit is 64 516 (all
    16 bits of the ISM hit record).  The expected maximum is asserted on the reference's numbers, then the device
    output is compared bit for bit.  Inputs on which both strands hit the same row, (AT)n against itself or poly-A
    against (AT)n, reach the same value, not a larger one: each strand then supplies half of the pairs."""
    L, n = 12, D.MAX_LEN
    top = 12 * 2036 * 254 * 254
    assert top == 1576254912
    polyA, polyC, at = D.homopolymer(D.A, n), D.homopolymer(D.C, n), D.repeat((D.A, D.T), n)
    seqs = [polyA, polyC, at]

    # k_explain, poly-A against itself: H[0]
    for weights, least in (("w254", top), ("w255", 1.5e9)):
        t, _, k, d, M, H = params = _params(weights, (12, 8, 4))
        want = E.tallies(polyA, polyA, t, L, d, M, H)
        print("explain %s: largest reference tally %d" % (weights, want.max()))
        assert want.max() >= 1.5e9 and want.max() >= least and want.max() < 2 ** 32
        if weights == "w254":
            assert want.max() == top
        run = ExplainLauncher(dv, params, seqs)
        try:
            _check_explain(run, [0], 0, [polyA], [want], d, (weights, "explain"))
        finally:
            run.close()

    # k_ism and k_ism<true>, poly-A against (AT)n at d = 6: every pair has six mismatches on either strand -> U[6], B[6]
    t, _, k, d, M, H = params = _params("w254", (12, 6, 6))
    U, B = R.tallies(polyA, at, t, L, d, M, H)
    print("ism poly-A x (AT)n: largest U %d (row %d), largest B %d" % (U.max(), int(np.argmax(U.max(axis=0))), B.max()))
    assert U[:, 6].max() == top and B.max() >= 1.5e9 and max(U.max(), B.max()) < 2 ** 32
    P = R.profile(polyA, at, t, L, d, M, H)
    irun, hrun = IsmLauncher(dv, params, seqs), HypLauncher(dv, params, seqs)
    try:
        _check_ism(irun, [2], 0, [polyA], [(U, B)], [P], L, d, ("w254", "ism AT"))
        _check_hyp(hrun, [2], 0, [polyA], [(U, B)], d, ("w254", "hyp AT"))
    finally:
        irun.close()
        hrun.close()

    # k_ism, poly-A against poly-C at d = 11: every pair mismatches on all 12 bases -> B[12] only, on both strands
    t, _, k, d, M, H = params = _params("w254", (12, 1, 11))
    U, B = R.tallies(polyA, polyC, t, L, d, M, H)
    print("ism poly-A x poly-C: largest B[12] %d" % B[:, 12].max())
    assert B[:, 12, D.C].max() == top and B[:, 12, D.G].max() == top and not U.any() and not B[:, :12].any()
    irun = IsmLauncher(dv, params, seqs)
    try:
        _check_ism(irun, [1], 0, [polyA], [(U, B)], None, L, d, ("w254", "ism C"))
    finally:
        irun.close()


def test_queue_inputs_are_exact(dv):
    """the inputs that tests/test_dense_host.py shows to flush k_ism's hit queues at every depth 64 .. 127: U, B, P and the
    hypothetical columns bit for bit (a hit lost or doubled at a full queue, or written into a neighbouring wave's queue,
    changes a tally)"""
    t, L, k, d = D.QUEUE_SHAPE
    params = (t, L, k, d, 50, 50.0)
    sv, queries = D.queue_inputs()
    seqs = [sv] + queries
    UB = [R.tallies(x, sv, t, L, d) for x in queries]
    P = [R.profile(x, sv, t, L, d) for x in queries]
    irun, hrun = IsmLauncher(dv, params, seqs), HypLauncher(dv, params, seqs)
    try:
        _check_ism(irun, [0], 1, queries, UB, P, L, d, ("queue",))
        _check_hyp(hrun, [0], 1, queries, UB, d, ("queue",))
    finally:
        irun.close()
        hrun.close()


@pytest.mark.parametrize("weights,shape", [("w254", (10, 6, 3)), ("unit", (12, 4, 8)), ("w255", (5, 2, 3))])
def test_self_profiles_of_dense_queries_are_exact(dv, weights, shape):
    """P_m(y, y) of every single-base mutant of a homopolymer, of (AT)n and of a spliced query: all positions at 200
    bases, the ends, L - 1 and the middle of a 2 047-base poly-A"""
    t, L, k, d, M, H = params = _params(weights, shape)
    queries = [D.homopolymer(D.A, 200), D.repeat((D.A, D.T), 200), D.spliced(200, L, 11), D.homopolymer(D.A, L),
               D.homopolymer(D.A, D.MAX_LEN)]
    if shape != (10, 6, 3):
        queries.pop()                                        # (the 2 047-base reference once)
    run = IsmLauncher(dv, params, [D.homopolymer(D.C, 30)] + queries)
    try:
        pad = 32
        got = run.self_profiles(1, 1 + len(queries), pad)
    finally:
        run.close()
    assert (got[:pad] == -77).all() and (got[-pad:] == -77).all()
    for qi, (g, x) in enumerate(zip(_split(got[pad:-pad], queries, (4, d + 1)), queries)):
        positions = None if len(x) < 1000 else [0, L - 1, 1000, len(x) - 1]
        want = R.self_profiles(x, t, L, d, M, H, positions=positions)
        rows = np.arange(len(x)) if positions is None else np.array(positions)
        assert np.array_equal(g[rows], want[rows]), (weights, shape, qi)
        if qi == 0 and weights == "w254":
            assert want[rows].max() >= 2 ** 31                # (beyond the 32-bit profiles of the Gram kernel)


@pytest.mark.parametrize("L,d", [(8, 3), (10, 3), (12, 4), (5, 5)])
def test_lmer_tables_of_low_complexity_classes_are_exact(dv, L, d):
    """classes taken from low-complexity support vectors (homopolymers, (AC)n, the palindromic (AT)^(L/2) for even L, a
    spliced sequence) and every class one substitution away from A^L, integer weights, c = e_m: k_lmer_weights bit for
    bit the numpy count; then k_lmer_score of the generator's queries over the whole integer table, bit for bit"""
    import torch
    svs = [D.homopolymer(D.A, L + 3), D.homopolymer(D.C, L), D.repeat((D.A, D.T), 2 * L), D.repeat((D.A, D.C), 2 * L),
           D.spliced(60, L, 3)]
    f = np.concatenate([E.pack(s, L).astype(np.int64) for s in svs])
    one_off = np.array([b << (2 * i) for i in range(L) for b in (1, 2, 3)], dtype=np.int64)
    f = np.concatenate((f, one_off))
    v = np.unique(np.minimum(f, LR.rc_codes(f, L))).astype(np.uint32)
    if L % 2 == 0:
        pal = int(E.pack(D.repeat((D.A, D.T), L), L)[0])
        assert pal in v and LR.rc_codes(np.array([pal]), L)[0] == pal
    rng = np.random.default_rng(L + d)
    cv = rng.integers(-7, 8, size=len(v)).astype(np.float64)
    cv[cv == 0] = 5.0
    top = 4 ** L
    if L <= 8:
        ranges = [(0, top)]
    else:
        ranges = [(0, 4096), (top - 4096, top), (top // 3 - 100, top // 3 + 2000)]            # A.., T.., CCCC..
        ranges += [(max(0, int(c) - 300), min(top, int(c) + 300)) for c in v[len(v) // 2:len(v) // 2 + 2]]
    for m in range(d + 1):
        c = np.zeros(d + 1)
        c[m] = 1.0
        got = _weights(dv, L, d, c, v, cv, ranges)
        for (u0, u1), g in zip(ranges, got):
            want = LR.count(np.arange(u0, u1), v, cv, L, d, c)
            assert np.array_equal(g, want), (L, d, m, u0, u1, np.nonzero(g != want)[0][:5])
            if m <= 1:
                assert np.abs(want).max() > 0
    if L > 8:
        return
    # the whole table at c = (1, 2, .. d + 1), integers: table scores of dense queries are exact whatever the order
    c = np.arange(1.0, d + 2)
    W = _weights(dv, L, d, c, v, cv, [(0, top)])[0]
    assert np.array_equal(W, LR.count(np.arange(top), v, cv, L, d, c))
    for weights in ("w50", "w254", "w255", "unit"):
        t, M, H = D.WEIGHTS[weights]
        model = types.SimpleNamespace(L=L, kernel_type=t, M=M, H=H)
        queries = [x for _, x in D.queries(L, d)]
        ctx = dv.GramContext(t, L, max(0, L - d), d, M, H, 1.0, 0)
        try:
            stream = torch.cuda.current_stream().cuda_stream
            ctx.set_sequences(queries, stream)
            d_W = torch.from_numpy(W).cuda()
            out = torch.full((len(queries),), -7.25, dtype=torch.float64, device="cuda")
            ctx.lmer_score(0, len(queries), d_W.data_ptr(), out.data_ptr(), stream)
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_lmer_score"
            got = out.cpu().numpy()
        finally:
            ctx.close()
        want = np.array([LR.table_score(model, W, x) for x in queries])
        assert np.array_equal(got, want), (L, d, weights, np.nonzero(got != want)[0])
        assert np.abs(want).max() > 0



# ------------------------------------------------------------------ chunk edges
def _chunk_problem(L, seed=5):
    """1 040 support vectors of L .. L + 3 bases, about half of them pieces of the two queries (either strand), so that a
    support vector dropped or counted twice at any chunk edge changes a tally; small integer coefficients of mixed sign"""
    rng = np.random.default_rng(seed)
    queries = [D.spliced(300, L, 9), D.homopolymer(D.A, 64 + L - 1)]
    svs = []
    for i in range(1040):
        n = L + int(rng.integers(0, 4))
        if i % 2 == 0 or i % 64 in (0, 1, 63) or i % 65 in (0, 1, 64):
            x = queries[int(rng.integers(0, 2))]
            p = int(rng.integers(0, len(x) - n + 1))
            s = x[p:p + n].copy()
            if rng.random() < 0.3:
                s = D.rc(s)
        else:
            s = rng.integers(0, 4, size=n, dtype=np.uint8)
        svs.append(s)
    coef = rng.integers(-6, 7, size=len(svs)).astype(np.float64)
    coef[coef == 0] = 2.0
    return svs, queries, coef


ROW_LISTS = [63, 64, 65, 1024, 1025, 1040, "subset"]


def test_chunk_edges_are_exact(dv):
    """explain_block, ism_block and hyp_block over 63, 64, 65, 1 024, 1 025 and 1 040 support vectors (one chunk, the
    first edge, 16 chunks of 64, the chunk growing to 65) and over a non-contiguous ascending row list, with col_begin >
    0: integer coefficients and unit fold vectors make every partial sum an integer below 2^53, so any order of summation
    gives the reference's double and the comparison is array_equal"""
    L, k, d = 10, 6, 3
    t, M, H = D.WEIGHTS["w50"]
    params = (t, L, k, d, M, H)
    svs, queries, coef = _chunk_problem(L)
    S = len(svs)
    spare = D.spliced(77, L, 1)                              # a column before the range: col_begin = S + 1
    seqs = svs + [spare] + queries
    c0 = S + 1
    UB = [[R.tallies(x, s, t, L, d, M, H) for s in svs] for x in queries]
    PR = [[R.profile(x, s, t, L, d, M, H) for s in svs] for x in queries]
    rng = np.random.default_rng(1)
    subset = np.sort(rng.choice(S, size=700, replace=False))
    runs = [ExplainLauncher(dv, params, seqs), IsmLauncher(dv, params, seqs), HypLauncher(dv, params, seqs)]
    try:
        for rows in ROW_LISTS:
            rows = subset if isinstance(rows, str) else np.arange(rows)
            cf = coef[rows]
            want, prof = [], []
            for qi in range(len(queries)):
                U = sum(c * UB[qi][i][0] for c, i in zip(cf, rows))
                B = sum(c * UB[qi][i][1] for c, i in zip(cf, rows))
                assert np.abs(U).max() < 2 ** 53 and np.abs(B).max() < 2 ** 53 and np.abs(U).max() > 0
                want.append((U, B))
                prof.append(sum(c * PR[qi][i] for c, i in zip(cf, rows)))
            tag = ("chunk", len(rows))
            for m in range(d + 1):
                got = runs[0].block(rows, c0, c0 + 2, _unit(d + 1, m), cf)
                for qi, g in enumerate(_split(got, queries, ())):
                    assert np.array_equal(g, want[qi][0][:, m]), tag + ("H", m, qi)
                out, base = runs[1].block(rows, c0, c0 + 2, _unit(d + 1, m), _unit(d + 1, None), _unit(d + 1, m), cf)
                for qi, (g, x) in enumerate(zip(_split(out, queries, (4,)), queries)):
                    w = np.repeat(want[qi][0][:, m:m + 1], 4, axis=1)
                    w[np.arange(len(x)), x] = 0.0
                    assert np.array_equal(g, w), tag + ("U", m, qi)
                    assert base[qi] == prof[qi][m], tag + ("P", m, qi)
                out, _ = runs[1].block(rows, c0, c0 + 2, _unit(d + 1, None), _unit(d + 1, m), _unit(d + 1, None), cf)
                for qi, g in enumerate(_split(out, queries, (4,))):
                    assert np.array_equal(g, want[qi][1][:, m + 1]), tag + ("B", m + 1, qi)
                out = runs[2].block(rows, c0, c0 + 2, _unit(d + 1, m), cf)
                for qi, (g, x) in enumerate(zip(_split(out, queries, (4,)), queries)):
                    w = want[qi][1][:, m + 1].astype(np.float64)
                    w[np.arange(len(x)), x] = want[qi][0][:, m]
                    assert np.array_equal(g, w), tag + ("hyp", m, qi)
    finally:
        for r in runs:
            r.close()


# ------------------------------------------------------------------ agreement of the entry points
def _model(gp, weights, shape, svs):
    t, L, k, d, M, H = _params(weights, shape)
    alpha = np.linspace(0.2, 1.0, len(svs))
    return gp.Model(t, L, k, d, M, H, 1.0, 1.0, 1e-3, False, 0.125, len(svs) // 2, alpha,
                    ["sv%d" % i for i in range(len(svs))], svs)


def _raw(P, c):
    g = 0.0
    for m in range(len(c)):
        g += c[m] * float(P[m])
    return g


class _Exact:
    """the score from the reference's 64-bit profiles: sum_s dual_coef_s G(x, s) / (sq_s sq_x) + rho, each G in ascending
    m from 0.0; and the largest profile entry seen for a query (what decides the no-wrap domain)"""

    def __init__(self, model):
        from oracle import oracle as O
        self.m = model
        self.kp = (model.kernel_type, model.L, model.d, model.M, model.H)
        self.c = O.mismatch_weights(model.kernel_type, model.L, model.k)[:model.d + 1]
        self.svP = [R.profile(s, s, *self.kp) for s in model.seqs]
        self.sq = [np.sqrt(_raw(P, self.c)) for P in self.svP]
        self.largest_sv = max(int(P.max()) for P in self.svP)

    def score(self, x):
        """-> (score, largest profile entry among P(x, s) and P(x, x))"""
        Pxx = R.profile(x, x, *self.kp)
        sqx = np.sqrt(_raw(Pxx, self.c))
        total, largest = 0.0, int(Pxx.max())
        for coef, s, sqs in zip(self.m.dual_coef(), self.m.seqs, self.sq):
            P = R.profile(x, s, *self.kp)
            largest = max(largest, int(P.max()))
            total += coef * _raw(P, self.c) / (sqs * sqx)
        return total + self.m.rho, largest


def _sampled(x, L):
    """mutant positions: both ends, L - 1 and the middle (a 2 047-base query: the start and the middle)"""
    return [0, len(x) // 2] if len(x) > 1000 else sorted({0, L - 1, len(x) // 2, len(x) - 1})


AGREE = [("w50", (10, 6, 3)), ("w254", (10, 6, 3)), ("w50", (12, 4, 8))]


@pytest.mark.parametrize("weights,shape", AGREE, ids=["%s-%d-%d-%d" % ((w,) + s) for w, s in AGREE])
def test_entry_points_agree_on_dense_queries(gp, weights, shape):
    """score, explain, ism, hypothetical and score_with_table of hand-built models with low-complexity support vectors,
    on the generator's queries.  Everywhere: completeness, ism and the table score against the exact score of the
    reference's 64-bit profiles, and the hypothetical columns against explain of the query and of each sampled mutant bit
    for bit.  Inside the no-wrap domain (computed from the reference alone): the same against `score`, with the
    tolerances of the tests of the same properties on iid input (1e-10 and 1e-12 x sum |dual_coef|)."""
    L, k, d = shape
    svs = [D.homopolymer(D.A, 150), D.repeat((D.A, D.T), 120), D.spliced(150, L, 2), D.homopolymer(D.C, L + 2),
           D.repeat(D.unit_of(3, 0), 90), D.rc(D.spliced(150, L, 2))[:100], D.repeat((D.C, D.G), 64), D.spliced(100, L, 4)]
    model = _model(gp, weights, shape, svs)
    ex = _Exact(model)
    assert ex.largest_sv < 2 ** 31                              # the support vectors themselves are inside the domain
    named = [(n, x) for n, x in D.queries(L, d) if len(x) < 1000 or n.startswith("polyA") or n.startswith("spliced")]
    if weights == "w50" and shape == (10, 6, 3):
        named.append(("polyA_2047", D.homopolymer(D.A, D.MAX_LEN)))
    named = [(n, x) for n, x in named if len(x) < 1000 or shape == (10, 6, 3)]        # (the long references once per weight)
    queries = [x for _, x in named]
    tol10 = 1e-10 * np.abs(model.dual_coef()).sum()
    tol12 = 1e-12 * np.abs(model.dual_coef()).sum()

    _, Ex = gp.explain(model, queries)
    _, Is = gp.ism(model, queries)
    _, Hy = gp.hypothetical(model, queries)
    _, sc = gp.score(model, queries)
    table = gp.lmer_weights(model)
    _, ts = gp.score_with_table(table, queries)

    mutants, index = [], []
    for qi, x in enumerate(queries):
        for t in _sampled(x, L):
            for b in range(4):
                if b != x[t]:
                    mutants.append(R.mutant(x, t, b))
                    index.append((qi, t, b))
    _, Ey = gp.explain(model, mutants)
    _, sy = gp.score(model, mutants)

    inside, long_inside = [], 0
    exact = [ex.score(x) for x in queries]
    exact_y = [ex.score(y) for y in mutants]
    for qi, (name, x) in enumerate(named):
        s_exact, largest = exact[qi]
        mine = [i for i, (q, _, _) in enumerate(index) if q == qi]
        largest = max([largest] + [exact_y[i][1] for i in mine])
        ok = largest < 2 ** 31
        inside.append(ok)
        tag = (weights, shape, name, ok)
        # everywhere: exact
        assert abs(Ex[qi].sum() - (s_exact - model.rho)) <= tol10, tag + ("completeness", Ex[qi].sum(), s_exact - model.rho)
        assert abs(ts[qi] - s_exact) <= tol12, tag + ("table", ts[qi], s_exact)
        assert Hy[qi][np.arange(len(x)), x].tobytes() == Ex[qi].tobytes(), tag + ("own column",)
        for i in mine:
            _, t, b = index[i]
            assert abs(Is[qi][t, b] - (exact_y[i][0] - s_exact)) <= tol12, tag + ("ism", t, b)
            assert Hy[qi][t, b] == Ey[i][t] and np.signbit(Hy[qi][t, b]) == np.signbit(Ey[i][t]), tag + ("hyp", t, b)
        if ok:                                                  # inside the domain: the same against `score`
            long_inside += len(x) == D.MAX_LEN and name.startswith("polyA")
            assert abs(Ex[qi].sum() - (sc[qi] - model.rho)) <= tol10, tag + ("completeness vs score",)
            assert abs(ts[qi] - sc[qi]) <= tol12, tag + ("table vs score", ts[qi], sc[qi])
            for i in mine:
                _, t, b = index[i]
                assert abs(Is[qi][t, b] - (sy[i] - sc[qi])) <= tol12, tag + ("ism vs score", t, b)
    print("%s %s: %d of %d queries inside the no-wrap domain" % (weights, shape, sum(inside), len(inside)))
    if weights == "w50":
        assert all(inside), [n for (n, _), ok in zip(named, inside) if not ok]
        if shape == (10, 6, 3):
            assert long_inside >= 1                             # a 2 047-base low-complexity query among them
    else:
        assert any(inside) and not all(inside)


def test_beyond_the_no_wrap_domain(gp):
    """poly-A, 2 047 bases, every weight 254, a poly-A support vector of 400 bases
    (and a short poly-C one): P_0(x, x) = 2 038^2 x 254^2 = 2.7e11.  `score`
    follows the reference, whose 32-bit profiles wrap (asserted against the oracle, NaN for NaN); explain, ism,
    hypothetical and the table score take every norm from exact 64-bit profiles and agree with the exact score."""
    weights, shape = "w254", (10, 6, 3)
    L, k, d = shape
    x = D.homopolymer(D.A, D.MAX_LEN)
    model = _model(gp, weights, shape, [D.homopolymer(D.A, 400), D.homopolymer(D.C, 30)])
    ex = _Exact(model)
    s_exact, largest = ex.score(x)
    assert largest == 2038 ** 2 * 254 ** 2 and ex.largest_sv >= 2 ** 31
    _, sc = gp.score(model, [x])
    want = LR.oracle_score(model, x, E.sv_norms(model))
    print("beyond the domain: score %r, oracle %r, exact %r" % (sc[0], want, s_exact))
    tol12 = 1e-12 * np.abs(model.dual_coef()).sum()
    assert (np.isnan(sc[0]) and np.isnan(want)) or abs(sc[0] - want) <= tol12 * max(1.0, abs(want))
    assert np.isnan(sc[0]) or abs(sc[0] - s_exact) > 1e-3        # (the wrap is visible: this query is outside the domain)
    _, Ex = gp.explain(model, [x])
    _, Is = gp.ism(model, [x])
    _, Hy = gp.hypothetical(model, [x])
    _, ts = gp.score_with_table(gp.lmer_weights(model), [x])
    print("explain sum %r, table %r, ism[1000] %r" % (Ex[0].sum(), ts[0], Is[0][1000]))
    assert np.isfinite(Ex[0]).all() and np.isfinite(Is[0]).all() and np.isfinite(Hy[0]).all()
    assert abs(Ex[0].sum() - (s_exact - model.rho)) <= 1e-10 * np.abs(model.dual_coef()).sum()
    assert abs(ts[0] - s_exact) <= tol12
    assert Hy[0][np.arange(len(x)), x].tobytes() == Ex[0].tobytes()
    for t in (0, 1000):
        for b in (D.C, D.T):
            y = R.mutant(x, t, b)
            assert abs(Is[0][t, b] - (ex.score(y)[0] - s_exact)) <= tol12, (t, b)
            _, Ey = gp.explain(model, [y])
            assert Hy[0][t, b] == Ey[0][t], (t, b)
