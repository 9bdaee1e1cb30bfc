"""gkmneighbours on the GPU: nearest neighbours, pairs above a threshold, de-duplication and grouped folds on a small pool
with planted near-copies, against the restatement (tests/neighbours_ref.py) applied to the matrices the project already
computes (gram_matrix, cross_kernel), and the planted pairs against the CPU oracle's matrix."""
import numpy as np
import pytest

from tests import helpers
from tests import neighbours_ref as R

L, K_, D = 8, 5, 2
TYPES = [0, 4, 5]
N_POOL, N_QUERIES = 48, 9
# (source, planted copy) as indices into the 44 original sequences and the 4 planted ones behind them, before the shuffle
PLANTED = [(3, "sub2"), (10, "sub3"), (20, "revcomp"), (30, "same")]
MOTIF = np.array([3, 2, 0, 1, 3, 1, 0, 2, 1, 0], dtype=np.uint8)        # TGACTCAGCA


def _mutate(rng, s, count):
    s = s.copy()
    for p in rng.choice(len(s), count, replace=False):
        s[p] = (s[p] + rng.randint(1, 4)) & 3
    return s


def _copy_of(rng, s, kind):
    if kind == "revcomp":
        return (3 - s)[::-1].copy()
    return _mutate(rng, s, {"sub2": 2, "sub3": 3, "same": 0}[kind])


def make_pool(seed=21):
    """-> (pool: 48 base-code arrays of 40..80 bp, pairs: the planted (i, j), i < j, sorted, queries: 9 more)."""
    from gkmqc_amd import synth
    from gkmqc_amd.device import encode
    rng = np.random.RandomState(seed)
    base = [encode(s) for s in synth.make_sequences(seed, N_POOL - len(PLANTED), length_range=(40, 80))]
    seqs = base + [_copy_of(rng, base[src], kind) for src, kind in PLANTED]
    perm = rng.permutation(N_POOL)                                     # pool[p] = seqs[perm[p]]
    where = np.argsort(perm)
    pairs = sorted(tuple(sorted((int(where[src]), int(where[len(base) + n])))) for n, (src, _) in enumerate(PLANTED))
    queries = [encode(s) for s in synth.make_sequences(seed + 1, N_QUERIES, length_range=(40, 80))]
    return [seqs[p] for p in perm], pairs, queries


def make_classes(seed=33, n_each=30, n_planted=6):
    """30 positives (a motif planted in each) + 30 negatives of 50..70 bp; the last n_planted of each class are copies,
    2 or 3 substitutions, of the first sequences of that class, two of them of the same source (a group of three).
    -> (seqs, groups: the planted labels)."""
    from gkmqc_amd import synth
    from gkmqc_amd.device import encode
    rng = np.random.RandomState(seed)
    seqs, labels = [], []
    for cls in (1, 0):
        own = [encode(s) for s in synth.make_sequences(seed + cls, n_each - n_planted, length_range=(50, 70))]
        if cls:
            for s in own:
                at = rng.randint(0, len(s) - len(MOTIF))
                s[at:at + len(MOTIF)] = _mutate(rng, MOTIF, 3)
        first = len(seqs)
        src = [0, 0, 1, 2, 3, 4][:n_planted]
        seqs += own + [_mutate(rng, own[a], 2 + n % 2) for n, a in enumerate(src)]
        labels += list(range(first, first + len(own))) + [first + a for a in src]
    return seqs, np.array(labels, dtype=np.int64)


def gap_of(K, pairs):
    """(the smallest planted-pair value, the largest other value) of the strict upper triangle."""
    iu, ju = np.triu_indices(K.shape[0], 1)
    planted = np.zeros(K.shape, dtype=bool)
    for i, j in pairs:
        planted[i, j] = True
    return float(K[iu, ju][planted[iu, ju]].min()), float(K[iu, ju][~planted[iu, ju]].max())


@pytest.fixture(scope="module")
def gn(built):
    from gkmqc_amd import gkmneighbours
    return gkmneighbours


@pytest.fixture(scope="module")
def pool():
    return make_pool()


@pytest.fixture(scope="module")
def matrices(built, pool):
    """Per kernel type, computed once and left alone: the pool's own matrix (gram_matrix, symmetric, still on the device,
    and its host copy) and the queries' rows against the pool (cross_kernel)."""
    from gkmqc_amd import device as dv
    seqs, _, queries = pool
    out = {}
    for t in TYPES:
        res = dv.gram_matrix(seqs, t, L, K_, D, symmetric=True)
        cross = dv.cross_kernel(queries + seqs, range(N_QUERIES), t, L, K_, D)["K"].cpu().numpy()[:, N_QUERIES:]
        out[t] = dict(dev=res["K"], own=res["K"].cpu().numpy(), cross=np.ascontiguousarray(cross))
    return out


def test_oracle_separates_the_planted_pairs(built, pool):
    """The precondition of the threshold tests, on the CPU: in the oracle's matrix every planted pair lies above every
    other pair, for each kernel type."""
    seqs, pairs, _ = pool
    assert len(seqs) == N_POOL and len(pairs) == 4 and all(40 <= len(s) <= 80 for s in seqs)
    for t in TYPES:
        lo, hi = gap_of(helpers.oracle_problem(seqs, (t, L, K_, D, 50, 50.0, 1.0))["K"], pairs)
        assert lo > hi, (t, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("t", TYPES)
def test_nearest_against_the_matrices(gn, pool, matrices, t):
    seqs, _, queries = pool
    m = matrices[t]
    own_ids = np.arange(N_POOL)
    for k_nn in (1, 4, 64):                                   # 64 > the pool: trailing -1 / nan
        want_own = R.topk(m["own"], own_ids, 0, k_nn)
        want_cross = R.topk(m["cross"], [-1] * N_QUERIES, 0, k_nn)
        for block in (1, 5, None):
            got = gn.nearest(seqs, None, k_nn, t, L, K_, D, block=block)
            assert R.same_lists(got, want_own), (k_nn, block)
            got = gn.nearest(queries, seqs, k_nn, t, L, K_, D, block=block)
            assert R.same_lists(got, want_cross), (k_nn, block)
        assert R.same_lists(gn.nearest_in_matrix(m["dev"], k_nn), want_own)
        assert R.same_lists(gn.nearest_in_matrix(m["dev"][:N_QUERIES], k_nn, exclude_self=False),
                            R.topk(m["own"][:N_QUERIES], [-1] * N_QUERIES, 0, k_nn))
    idx, val = gn.nearest(seqs, None, 64, t, L, K_, D)
    assert (idx[:, N_POOL - 1:] == -1).all() and np.isnan(val[:, N_POOL - 1:]).all() and (idx[:, :N_POOL - 1] >= 0).all()
    assert not (idx == own_ids[:, None]).any()                # never its own neighbour


@pytest.mark.gpu
@pytest.mark.parametrize("t", TYPES)
def test_pairs_above_against_the_matrices(gn, pool, matrices, t):
    seqs, _, queries = pool
    m = matrices[t]
    for q in (50, 90):
        thr = float(np.percentile(m["own"], q))
        want = R.pairs_flat(m["own"], np.arange(N_POOL), 1, thr)
        for block in (1, 5, None):
            got = gn.pairs_above(seqs, thr, kernel_type=t, L=L, k=K_, d=D, block=block)
            assert all(R.same_bits(g, w) for g, w in zip(got, want)), (q, block)
        got = gn.pairs_in_matrix(m["dev"], thr)
        assert all(R.same_bits(g, w) for g, w in zip(got, want))
        thr = float(np.percentile(m["cross"], q))
        want = R.pairs_flat(m["cross"], [-1] * N_QUERIES, 0, thr)
        for block in (5, None):
            got = gn.pairs_above(queries, thr, other=seqs, kernel_type=t, L=L, k=K_, d=D, block=block)
            assert all(R.same_bits(g, w) for g, w in zip(got, want)), (q, block)
    whole = R.pairs_flat(m["own"][:7], [-1] * 7, 0, thr)
    assert all(R.same_bits(g, w) for g, w in zip(gn.pairs_in_matrix(m["dev"][:7], thr, upper=False), whole))


@pytest.mark.gpu
@pytest.mark.parametrize("t", TYPES)
def test_planted_pairs_and_dedupe(gn, pool, t):
    seqs, pairs, _ = pool
    lo, hi = gap_of(helpers.oracle_problem(seqs, (t, L, K_, D, 50, 50.0, 1.0))["K"], pairs)
    assert lo > hi                                            # (the precondition; test_oracle_separates_the_planted_pairs)
    thr = (lo + hi) / 2
    i, j, v = gn.pairs_above(seqs, thr, kernel_type=t, L=L, k=K_, d=D, block=7)
    assert list(zip(i.tolist(), j.tolist())) == pairs and (v >= thr).all()
    keep, labels = gn.dedupe(seqs, thr, kernel_type=t, L=L, k=K_, d=D)
    want = np.arange(N_POOL)
    for a, b in pairs:
        want[b] = a
    assert np.array_equal(labels, want)
    assert keep.tolist() == [s for s in range(N_POOL) if s not in {b for _, b in pairs}]      # the lowest of each group


@pytest.mark.gpu
def test_max_pairs_exceeded_is_raised_by_name(gn, pool, matrices):
    seqs = pool[0]
    total = N_POOL * (N_POOL - 1) // 2
    assert len(gn.pairs_above(seqs, -1.0, max_pairs=total, kernel_type=0, L=L, k=K_, d=D)[0]) == total
    for block in (5, None):
        with pytest.raises(gn.ModelError, match="pairs_above: %d pairs at or above the threshold, more than max_pairs = %d"
                           % (total, total - 1)):
            gn.pairs_above(seqs, -1.0, max_pairs=total - 1, kernel_type=0, L=L, k=K_, d=D, block=block)
    with pytest.raises(gn.ModelError, match="pairs_in_matrix: %d pairs .* more than max_pairs = 3" % total):
        gn.pairs_in_matrix(matrices[0]["dev"], -1.0, max_pairs=3)


@pytest.mark.gpu
def test_cli_writes_what_the_functions_return(gn, pool, tmp_path):
    import os
    from gkmqc_amd import synth
    seqs, pairs, _ = pool
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    fa = str(tmp_path / "pool.fa")
    synth.write_fasta(fa, [letters[s].tobytes() for s in seqs], "s")
    base = ["-t", "0", "-L", str(L), "-k", str(K_), "-d", str(D)]
    out = str(tmp_path / "nn.tsv")
    assert gn.main(["nearest", "-K", "3"] + base + [fa, out]) == 0
    names, idx, val = gn.read_nearest(out)
    assert names == ["s%d" % s for s in range(N_POOL)] and R.same_lists((idx, val), gn.nearest(seqs, None, 3, 0, L, K_, D))
    out = str(tmp_path / "dd")
    assert gn.main(["dedupe", "--threshold", "0.6"] + base + [fa, out]) == 0
    gnames, labels = gn.read_groups(out + ".groups.tsv")
    keep, want = gn.dedupe(seqs, 0.6, kernel_type=0, L=L, k=K_, d=D)
    assert np.array_equal(labels, want) and open(out + ".pos.fa").read().count(">") == len(keep)
    assert not [n for n in os.listdir(str(tmp_path)) if ".tmp" in n]


@pytest.mark.gpu
def test_cross_validation_on_grouped_folds_matches_scikit_learn(gn):
    """crossValidate on the folds of grouped_plan: mean and std of the AUC as scikit-learn's SVC(kernel="precomputed")
    gives them on the same folds of the same matrix (the comparison of tests/test_gkmsvm_mirror.py)."""
    from sklearn.metrics import roc_auc_score
    from sklearn.svm import SVC
    from gkmqc_amd import device as dv
    from gkmqc_amd import svmcv
    seqs, groups = make_classes()
    K = dv.gram_matrix(seqs, 4, L, K_, D, symmetric=True)["K"]
    host = K.cpu().numpy()
    iu, ju = np.triu_indices(60, 1)
    same = groups[iu] == groups[ju]
    lo, hi = float(host[iu, ju][same].min()), float(host[iu, ju][~same].max())
    assert lo > hi, (lo, hi)
    i, j, _ = gn.pairs_in_matrix(K, (lo + hi) / 2)
    labels = gn.redundancy_groups(60, i, j)
    assert np.array_equal(labels, groups)
    plan = gn.grouped_plan(30, 30, labels, ncv=5, seed=1)
    for train, test in zip(plan["u_trains"], plan["u_tests"]):
        assert not set(labels[train].tolist()) & set(labels[test].tolist())
    args_svm = [1.0, 1e-3, 0, 512, 5, 1, 0, 1, 1]
    auc, std = svmcv.crossValidate(args_svm, K, 30, 30, plan=plan)
    y = plan["y"]
    aucs = []
    for train, test in zip(plan["u_trains"], plan["u_tests"]):
        sv = SVC(kernel="precomputed", C=1.0, tol=1e-3, shrinking=False, cache_size=512)
        sv.fit(host[np.ix_(train, train)], y[train])
        aucs.append(roc_auc_score(y[test], sv.decision_function(host[np.ix_(test, train)])))
    assert abs(auc - np.mean(aucs)) < 1e-9 and abs(std - np.std(aucs)) < 1e-9
    assert 0.0 < np.std(aucs) and 0.5 < np.mean(aucs) < 1.0              # (folds that differ, a problem that is one)
