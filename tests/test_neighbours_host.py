"""gkmneighbours without a GPU: the restatement (tests/neighbours_ref.py) against hand-written cases, redundancy groups,
grouped folds, the files' round trips and the argument errors."""
import os

import numpy as np
import pytest

from tests import neighbours_ref as R

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ the restatement against hand-written cases
def test_restatement_order_and_eligibility_by_hand():
    K = np.array([[0.5, 2.0, 0.5, NAN, 2.0, -1.0],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    # mode 0, own columns 1 and 12 (col_base 10): row 0 loses column 11, row 1 column 12
    idx, val = R.topk(K, [11, 12], 0, 3, col_base=10)
    assert idx.tolist() == [[14, 10, 12], [10, 11, 13]]
    assert val.tolist() == [[2.0, 0.5, 0.5], [1.0, 1.0, 1.0]]
    # mode 1: only the columns behind the own one
    idx, val = R.topk(K, [11, 14], 1, 4, col_base=10)
    assert idx.tolist() == [[14, 12, 15, -1], [15, -1, -1, -1]]
    assert np.isnan(val[0, 3]) and np.isnan(val[1, 1:]).all() and val[0, :3].tolist() == [2.0, 0.5, -1.0]
    # -1: no own column; NaN is never listed
    idx, _ = R.topk(K, [-1, -1], 0, 6)
    assert idx.tolist() == [[1, 4, 0, 2, 5, -1], [0, 1, 2, 3, 4, 5]]


def test_restatement_zero_signs_infinities_and_cut():
    K = np.array([[0.0, -0.0, INF, -INF, -0.0]])
    idx, val = R.topk(K, [-1], 0, 5)
    assert idx.tolist() == [[2, 0, 1, 4, 3]]                      # the zeros tie: ascending column
    assert np.signbit(val[0]).tolist() == [False, False, True, True, True]      # each cell's own bits
    whole = R.topk(K, [-1], 0, 2)
    bi, bv = R.empty_lists(1, 2)
    for c0 in (3, 0):                                             # two blocks, the later columns first
        bi, bv = R.merge(K[:, c0:c0 + 3], min(3, 5 - c0), [-1], c0, 0, 2, bi, bv)
    assert R.same_lists((bi, bv), whole)


def test_restatement_pairs_by_hand():
    K = np.array([[1.0, 0.7, NAN, 0.9],
                  [0.7, 1.0, 0.7, 0.2],
                  [0.1, 0.2, 0.3, 0.4]])
    rows = R.pairs(K, 4, [0, 1, 2], 0, 1, 0.7)
    assert rows == [[(0, 1, 0.7), (0, 3, 0.9)], [(1, 2, 0.7)], []]
    i, j, v = R.pairs_flat(K, [0, 1, 2], 1, 0.7)
    assert i.tolist() == [0, 0, 1] and j.tolist() == [1, 3, 2] and v.tolist() == [0.7, 0.9, 0.7]
    assert [len(r) for r in R.pairs(K, 4, [-1, -1, -1], 0, 0, NAN)] == [0, 0, 0]


# ------------------------------------------------------------------ groups
@pytest.mark.parametrize("n,edges,want", [
    (6, [], [0, 1, 2, 3, 4, 5]),                                               # singletons
    (6, [(4, 5), (3, 4), (2, 3), (1, 2)], [0, 1, 1, 1, 1, 1]),                 # a chain, given from its far end
    (7, [(3, 0), (3, 6), (3, 5), (1, 2)], [0, 1, 1, 0, 4, 0, 0]),              # a star around 3 and a pair
    (4, [(0, 1), (1, 0), (0, 1), (2, 2)], [0, 0, 2, 3]),                       # repeated edges and a loop
])
def test_redundancy_groups(n, edges, want):
    from gkmqc_amd import gkmneighbours as gn
    i, j = [e[0] for e in edges], [e[1] for e in edges]
    labels = gn.redundancy_groups(n, i, j)
    assert labels.dtype == np.int64 and labels.tolist() == want
    assert R.components(n, i, j).tolist() == want
    keep = gn.representatives(labels)
    assert keep.tolist() == sorted(set(want))


def test_redundancy_groups_random_against_restatement():
    from gkmqc_amd import gkmneighbours as gn
    rng = np.random.RandomState(5)
    for n, m in ((1, 0), (40, 15), (200, 120), (200, 400)):
        i, j = rng.randint(0, n, m), rng.randint(0, n, m)
        assert np.array_equal(gn.redundancy_groups(n, i, j), R.components(n, i, j))


def test_groups_refusals():
    from gkmqc_amd import gkmneighbours as gn
    with pytest.raises(gn.ModelError, match="outside 0..3"):
        gn.redundancy_groups(4, [0], [4])
    with pytest.raises(gn.ModelError, match="one entry per edge"):
        gn.redundancy_groups(4, [0, 1], [1])
    with pytest.raises(gn.ModelError, match="lowest member"):
        gn.representatives([1, 1, 2])
    with pytest.raises(gn.ModelError, match="lowest member"):
        gn.representatives([0, 0, 1])


# ------------------------------------------------------------------ grouped folds
def _planted(n_p, n_n, seed, n_groups=9, largest=5):
    rng = np.random.RandomState(seed)
    n = n_p + n_n
    i, j = [], []
    for _ in range(n_groups):
        mem = rng.choice(n, rng.randint(2, largest + 1), replace=False)
        i.extend(mem[:-1].tolist())
        j.extend(mem[1:].tolist())
    return i, j


@pytest.mark.parametrize("n_p,n_n,ncv,seed", [(30, 30, 5, 1), (41, 57, 4, 2), (12, 90, 3, 3)])
def test_grouped_plan_properties(n_p, n_n, ncv, seed):
    from gkmqc_amd import gkmneighbours as gn
    n = n_p + n_n
    labels = gn.redundancy_groups(n, *_planted(n_p, n_n, seed))
    assert len(set(labels.tolist())) < n
    plan = gn.grouped_plan(n_p, n_n, labels, ncv=ncv, seed=seed)
    # the format of svmcv.plan_folds, key for key, and what crossValidate reads from it
    from gkmqc_amd import svmcv
    want = svmcv.plan_folds((None, 1e-3, 0, None, ncv, 1, 0, seed), n_p, n_n)
    assert sorted(plan) == sorted(want) and plan["sizes"] == (n_p, n_n) and plan["sizes"] == want["sizes"]
    assert np.array_equal(plan["y"], want["y"]) and plan["n_folds"] == ncv and plan["which"] == list(range(ncv))
    assert len(plan["u_trains"]) == len(plan["u_tests"]) == ncv
    seen = np.zeros(n, dtype=int)
    for train, test in zip(plan["u_trains"], plan["u_tests"]):
        assert train.dtype == want["u_trains"][0].dtype and test.dtype == want["u_tests"][0].dtype
        assert len(np.intersect1d(train, test)) == 0 and len(train) + len(test) == n
        assert (np.diff(train) > 0).all() and (np.diff(test) > 0).all()
        assert not set(labels[train].tolist()) & set(labels[test].tolist())          # no group on both sides
        for part in (train, test):
            assert 0 < plan["y"][part].sum() < len(part)
        seen[test] += 1
    assert (seen == 1).all()                                                            # tested exactly once
    fold = gn.plan_fold_of(plan)
    assert np.array_equal(fold, R.deal_groups(n_p, n_n, labels, ncv, seed))            # the documented rule
    again = gn.grouped_plan(n_p, n_n, labels, ncv=ncv, seed=seed)
    assert all(np.array_equal(a, b) for a, b in zip(plan["u_tests"], again["u_tests"]))


def test_grouped_plan_seed_moves_only_equal_sized_groups():
    from gkmqc_amd import gkmneighbours as gn
    labels = gn.redundancy_groups(60, *_planted(30, 30, 1))
    folds = set()
    for seed in range(8):
        fold = gn.plan_fold_of(gn.grouped_plan(30, 30, labels, 5, seed))
        assert np.array_equal(fold, R.deal_groups(30, 30, labels, 5, seed))
        folds.add(tuple(fold.tolist()))
    assert len(folds) > 1


def test_grouped_plan_refusals():
    from gkmqc_amd import gkmneighbours as gn
    one = np.zeros(20, dtype=np.int64)                     # a single group: four folds stay empty
    with pytest.raises(gn.ModelError, match="part of fold .* does not hold both classes"):
        gn.grouped_plan(10, 10, one, ncv=5)
    pos_glued = np.arange(20)
    pos_glued[:10] = 0                                     # all positives in one group: the other folds test no positive
    with pytest.raises(gn.ModelError, match="does not hold both classes"):
        gn.grouped_plan(10, 10, pos_glued, ncv=2)
    with pytest.raises(gn.ModelError, match="ncv must be at least 2"):
        gn.grouped_plan(10, 10, np.arange(20), ncv=1)
    with pytest.raises(gn.ModelError, match="19 labels for 20 sequences"):
        gn.grouped_plan(10, 10, np.arange(19))
    with pytest.raises(gn.ModelError, match="both classes need"):
        gn.grouped_plan(0, 10, np.arange(10))


# ------------------------------------------------------------------ files
def test_file_round_trips(tmp_path):
    from gkmqc_amd import gkmneighbours as gn
    names = ["a b", "c", "d|e"]
    idx = np.array([[2, 1, -1], [0, -1, -1], [0, 1, -1]], dtype=np.int32)
    val = np.array([[0.1 + 0.2, -0.0, NAN], [INF, NAN, NAN], [1e-310, -2.5, NAN]])
    p = str(tmp_path / "nn.tsv")
    gn.write_nearest(p, names, idx, val)
    got = gn.read_nearest(p)
    assert got[0] == names and R.same_lists(got[1:], (idx, val)) and got[1].dtype == np.int32
    assert np.signbit(got[2][0, 1])

    i, j, v = np.array([0, 0, 2], np.int32), np.array([1, 2, 1], np.int32), np.array([0.1 + 0.2, 1.0, 5e-324])
    p = str(tmp_path / "pairs.tsv")
    gn.write_pairs(p, i, j, v, names, names)
    gi, gj, gv = gn.read_pairs(p)
    assert R.same_bits(gi, i) and R.same_bits(gj, j) and R.same_bits(gv, v)
    gn.write_pairs(p, i[:0], j[:0], v[:0], names, names)
    assert [len(a) for a in gn.read_pairs(p)] == [0, 0, 0]

    labels = np.array([0, 1, 0], dtype=np.int64)
    p = str(tmp_path / "groups.tsv")
    gn.write_groups(p, names, labels)
    assert open(p).read().split("\n")[2] == "2\td|e\t0\t0"
    gnames, glabels = gn.read_groups(p)
    assert gnames == names and np.array_equal(glabels, labels)

    lab = gn.redundancy_groups(24, [0, 13], [1, 20])
    plan = gn.grouped_plan(12, 12, lab, ncv=3, seed=4)
    fnames = ["s%d" % s for s in range(24)]
    p = str(tmp_path / "folds.tsv")
    gn.write_folds(p, fnames, plan, lab)
    rnames, rlab, rplan = gn.read_folds(p)
    assert rnames == fnames and np.array_equal(rlab, lab) and rplan["sizes"] == plan["sizes"]
    assert rplan["which"] == plan["which"] and rplan["n_folds"] == 3 and np.array_equal(rplan["y"], plan["y"])
    for key in ("u_trains", "u_tests"):
        assert all(np.array_equal(a, b) for a, b in zip(rplan[key], plan[key]))

    from gkmqc_amd import device as dv
    seqs = dv.FlatSequences(np.array([0, 1, 2, 3, 3, 3, 0], np.uint8), np.array([0, 4, 5, 7]))
    p = str(tmp_path / "kept.fa")
    gn.write_fasta(p, seqs, names, [0, 2])
    assert open(p).read() == ">a b\nACGT\n>d|e\nTA\n"


def test_readers_name_the_bad_line(tmp_path):
    from gkmqc_amd import gkmneighbours as gn
    p = str(tmp_path / "bad.tsv")
    open(p, "w").write("q\t1,2\t0.5,0.25\nr\t1\t0.5,0.25\n")
    with pytest.raises(gn.ModelError, match="bad.tsv:2: the lists' lengths"):
        gn.read_nearest(p)
    open(p, "w").write("0\t1\ta\tb\n")
    with pytest.raises(gn.ModelError, match="bad.tsv:1: expected 5 tab-separated fields"):
        gn.read_pairs(p)
    open(p, "w").write("0\ta\t0\t1\n2\tb\t0\t0\n")
    with pytest.raises(gn.ModelError, match="bad.tsv:2: expected the running index"):
        gn.read_groups(p)


# ------------------------------------------------------------------ arguments
def _fasta(path, n=4, length=30):
    from gkmqc_amd import synth
    synth.write_fasta(path, synth.make_sequences(7, n, length), "s")
    return path


@pytest.mark.parametrize("argv,message", [
    (["nearest", "-K", "0", "FA", "OUT"], "nearest: k_nn must lie in 1..64, not 0"),
    (["nearest", "-K", "65", "FA", "OUT"], "nearest: k_nn must lie in 1..64, not 65"),
    (["nearest", "-L", "13", "FA", "OUT"], "nearest: "),
    (["nearest", "--block", "0", "FA", "OUT"], "nearest: block must be at least 1"),
    (["pairs", "--threshold", "nan", "FA", "OUT"], "pairs: the threshold is not a number"),
    (["pairs", "--threshold", "0.5", "--max-pairs", "-1", "FA", "OUT"], "pairs: max_pairs must not be negative"),
    (["pairs", "--threshold", "0.5", "-L", "10", "-k", "6", "-d", "3", "SHORT", "OUT"],
     "pairs_above: sequence 0 is shorter than L = 10"),
    (["dedupe", "--threshold", "0.5", "MISSING", "OUT"], "cannot read"),
    (["folds", "--threshold", "0.5", "-x", "1", "FA", "FA", "OUT"], "folds: ncv must be at least 2, not 1"),
])
def test_cli_argument_errors_by_name(built, tmp_path, capsys, argv, message):
    """Each is refused before any device call, with the argument's name, exit status 1 and no file left behind."""
    from gkmqc_amd import gkmneighbours as gn
    fa = _fasta(str(tmp_path / "in.fa"))
    short = _fasta(str(tmp_path / "short.fa"), 2, 8)
    out = str(tmp_path / "out")
    place = {"FA": fa, "SHORT": short, "OUT": out, "MISSING": str(tmp_path / "none.fa")}
    assert gn.main([place.get(a, a) for a in argv]) == 1
    err = capsys.readouterr().err
    assert err.startswith("gkmneighbours: error: ") and message in err
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa", "short.fa"]


def test_cli_requires_a_threshold_and_a_command():
    from gkmqc_amd import gkmneighbours as gn
    for argv in ([], ["pairs", "a.fa", "out"], ["cluster", "a.fa", "out"]):
        with pytest.raises(SystemExit) as e:
            gn.main(argv)
        assert e.value.code == 2


def test_function_argument_errors_by_name(built):
    from gkmqc_amd import gkmneighbours as gn
    seqs = [np.zeros(20, np.uint8), np.ones(20, np.uint8)]
    with pytest.raises(gn.ModelError, match="nearest: k_nn must lie in 1..64"):
        gn.nearest(seqs, k_nn=100)
    with pytest.raises(gn.ModelError, match="nearest: no pool sequences"):
        gn.nearest(seqs, pool=[], L=8, k=5, d=2)
    with pytest.raises(gn.ModelError, match="pairs_above: pool sequence 1 is shorter than L = 8"):
        gn.pairs_above(seqs, 0.5, other=[seqs[0], np.zeros(5, np.uint8)], L=8, k=5, d=2)
    with pytest.raises(gn.ModelError, match="pairs_in_matrix: the threshold is not a number"):
        gn.pairs_in_matrix(None, NAN)
    with pytest.raises(gn.ModelError, match="nearest_in_matrix: K must be"):
        gn.nearest_in_matrix(np.eye(3), 2)


def test_default_blocks_fit_the_budget():
    from gkmqc_amd import gkmneighbours as gn
    assert gn.default_block(10000, 10000) == 10000                       # gkmQC's subset: one tile
    b = gn.default_block(100000, 10000)
    assert b == gn.BLOCK_BYTES // (16 * gn.ROW_CHUNK) and 16 * gn._row_chunk(100000, b) * b <= gn.BLOCK_BYTES
    assert gn._row_chunk(100000, 1) == gn.ROW_CHUNK and gn._row_chunk(5, 1) == 5
    assert 16 * gn._row_chunk(10 ** 6, 10 ** 6) * 10 ** 6 <= gn.BLOCK_BYTES
