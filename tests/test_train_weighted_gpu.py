"""Class weights from the model file down to the solver, and the grid cross-validation, on the GPU:
gkmmodel.train / gkmpanels.train_panel with `class_weight`, the gkmqc-model-2 file, svmcv.cross_validate_grid,
gkmmodel.select and the command lines of gkmselect and gkmpanels.  The data: 20 sequences of 60 bp with a planted motif
(label 1) against 60 without (label 0), L = 6, k = 4, d = 2.  Every comparison is exact: scikit-learn's SVC on the Gram
matrix gram_matrix returns.  Every solve is asserted to come from the GPU solver (iters >= 0), not from the scikit-learn
re-solve of a capped problem."""
import os

import numpy as np
import pytest

from tests.test_explain_gpu import _planted

pytestmark = pytest.mark.gpu

KP = dict(kernel_type=4, L=6, k=4, d=2)
MOTIF = np.array([0, 3, 2, 0, 1, 2, 3, 1], np.uint8)
NPOS, NNEG, NQ = 20, 60, 15
TOL = 1e-3


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _write_fasta(gm, path, seqs, names):
    with open(path, "w") as f:
        for name, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (name, gm.codes_to_text(s)))


class _Data:
    def __init__(self, tmp):
        import torch
        from gkmqc_amd import device as dv
        from gkmqc_amd import gkmmodel as gm
        self.tmp = tmp
        pos, _ = _planted(31, NPOS, 60, MOTIF)
        neg, _ = _planted(32, NNEG, 60, None)
        qry = _planted(33, NQ // 2, 60, MOTIF)[0] + _planted(34, NQ - NQ // 2, 60, None)[0]
        self.pos_fa, self.neg_fa, self.query_fa = (os.path.join(tmp, n) for n in ("pos.fa", "neg.fa", "query.fa"))
        self.names = ["p%d" % i for i in range(NPOS)] + ["n%d" % i for i in range(NNEG)]
        _write_fasta(gm, self.pos_fa, pos, self.names[:NPOS])
        _write_fasta(gm, self.neg_fa, neg, self.names[NPOS:])
        _write_fasta(gm, self.query_fa, qry, ["q%d" % i for i in range(NQ)])
        self.seqs = pos + neg
        everything = pos + neg + qry
        off = np.zeros(len(everything) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in everything], out=off[1:])
        res = dv.gram_matrix(dv.FlatSequences(np.concatenate(everything), off), KP["kernel_type"], KP["L"], KP["k"], KP["d"],
                             symmetric=True)
        K = res["K"].cpu().numpy()
        del res
        torch.cuda.empty_cache()
        nt = NPOS + NNEG
        self.K, self.Kq = np.ascontiguousarray(K[:nt, :nt]), np.ascontiguousarray(K[nt:, :nt])
        self.y = np.concatenate((np.repeat(1, NPOS), np.repeat(0, NNEG)))
        # a pool for train_panel: the same records in mixed order, three unbalanced tasks, one leaving records out
        rng = np.random.default_rng(35)
        self.order = rng.permutation(nt)
        self.Y = np.empty((nt, 3), dtype=np.int8)
        self.Y[:, 0] = self.y[self.order]
        self.Y[:, 1] = np.arange(nt) % 7 == 0
        self.Y[:, 2] = np.where(rng.random(nt) < 0.2, -1, (rng.random(nt) < 0.3).astype(np.int8))
        self.tasks = ["motif", "sevenths", "sparse"]
        self.pool_fa = os.path.join(tmp, "pool.fa")
        self.pool_names = [self.names[i] for i in self.order]
        _write_fasta(gm, self.pool_fa, [self.seqs[i] for i in self.order], self.pool_names)
        self.labels_tsv = os.path.join(tmp, "labels.tsv")
        sym = {1: "1", 0: "0", -1: "."}
        with open(self.labels_tsv, "w") as f:
            f.write("\t".join(["name"] + self.tasks) + "\n")
            for name, row in zip(self.pool_names, self.Y.tolist()):
                f.write("\t".join([name] + [sym[x] for x in row]) + "\n")
        self.split = []
        for t, task in enumerate(self.tasks):
            files = []
            for lab, word in ((1, "pos"), (0, "neg")):
                keep = np.flatnonzero(self.Y[:, t] == lab)
                files.append(os.path.join(tmp, "%s_%s.fa" % (task, word)))
                _write_fasta(gm, files[-1], [self.seqs[self.order[i]] for i in keep], [self.pool_names[i] for i in keep])
            self.split.append(files)


@pytest.fixture(scope="module")
def data(built, tmp_path_factory):
    return _Data(str(tmp_path_factory.mktemp("weighted")))


@pytest.fixture
def solver_runs(monkeypatch):
    """every svmcv.train_tasks call of the test, recorded: (boxed?, iters) -- and no problem may have hit the cap"""
    from gkmqc_amd import svmcv
    runs = []
    real = svmcv.train_tasks

    def spy(K, trains, labels, C=1.0, tol=1e-3, shrinking=False, about_to_launch=None, class_weight=None):
        sol, handles = real(K, trains, labels, C, tol, shrinking, about_to_launch, class_weight)
        assert (np.asarray(sol.iters) >= 0).all(), list(sol.iters)
        runs.append((not (np.ndim(C) == 0 and class_weight is None), [int(i) for i in sol.iters]))
        return sol, handles
    monkeypatch.setattr(svmcv, "train_tasks", spy)
    return runs


def _sk(data, C, cw, shrinking=False):
    from sklearn.svm import SVC
    return SVC(kernel="precomputed", C=C, tol=TOL, shrinking=shrinking,
               class_weight=cw if cw is None or isinstance(cw, str) else {0: cw[0], 1: cw[1]}).fit(data.K, data.y)


def _file(model, path):
    model.save(path)
    with open(path, "rb") as f:
        return f.read()


# ------------------------------------------------------------------ training
@pytest.mark.parametrize("cw", [(1, 3), "balanced", (4.0, 0.25)], ids=str)
@pytest.mark.parametrize("shrinking", [False, True], ids=["k_smo", "shrinking"])
def test_train_with_class_weights_is_scikit_learn(data, solver_runs, tmp_path, cw, shrinking):
    """support set, alpha and rho bit for bit; the file loads back to the same model, whose scores are scikit-learn's
    decision_function"""
    from gkmqc_amd import gkmmodel as gm
    from gkmqc_amd import gkmquery as gq
    model = gm.train(data.pos_fa, data.neg_fa, C=0.5, tol=TOL, shrinking=shrinking, class_weight=cw, **KP)
    assert len(solver_runs) == 1 and solver_runs[0][0]
    m = _sk(data, 0.5, cw, shrinking)
    assert solver_runs[0][1] == [int(np.ravel(m.n_iter_)[0])]
    assert model.names == [data.names[i] for i in m.support_]
    assert model.n0 == int(m.n_support_[0])
    assert _same(model.dual_coef(), m.dual_coef_[0]) and _same(model.rho, m.intercept_[0])
    assert _same(model.class_weight, m.class_weight_) and model.class_weight[0] != model.class_weight[1]
    if cw == "balanced":
        assert model.class_weight == (80 / 120, 80 / 40)
    path = str(tmp_path / "m.txt")
    text = _file(model, path)
    assert text.startswith(b"format gkmqc-model-2\n")
    assert ("weight0 %r\nweight1 %r\n" % model.class_weight).encode() in text
    back = gm.load(path)
    assert back.class_weight == model.class_weight and _same(back.alpha, model.alpha) and back.names == model.names
    assert back.rho == model.rho and back.n0 == model.n0 and _file(back, str(tmp_path / "again.txt")) == text
    names, scores = gq.score(back, data.query_fa)
    assert names == ["q%d" % i for i in range(NQ)]
    assert _same(scores, m.decision_function(data.Kq))


def test_train_without_weights_is_unchanged(data, solver_runs, tmp_path):
    """class_weight=None: the unboxed solver entry, a gkmqc-model-1 file"""
    from gkmqc_amd import gkmmodel as gm
    model = gm.train(data.pos_fa, data.neg_fa, C=0.5, tol=TOL, **KP)
    assert solver_runs == [(False, [int(np.ravel(_sk(data, 0.5, None).n_iter_)[0])])]
    assert model.class_weight is None and _file(model, str(tmp_path / "m.txt")).startswith(b"format gkmqc-model-1\n")
    same = gm.train(data.pos_fa, data.neg_fa, C=0.5, tol=TOL, class_weight=(1.0, 1.0), **KP)
    assert solver_runs[1][0] and solver_runs[1][1] == solver_runs[0][1]
    assert _same(same.alpha, model.alpha) and same.rho == model.rho and same.names == model.names
    assert same.class_weight == (1.0, 1.0)


# ------------------------------------------------------------------ train_panel
@pytest.mark.parametrize("cw", ["balanced", (1.0, 3.0)], ids=str)
def test_train_panel_with_class_weights_writes_trains_bytes(data, solver_runs, tmp_path, cw):
    from gkmqc_amd import gkmmodel as gm
    from gkmqc_amd import gkmpanels as pn
    tasks, models = pn.train_panel(data.pool_fa, data.labels_tsv, C=0.5, tol=TOL, class_weight=cw, **KP)
    assert tasks == data.tasks and len(solver_runs) == 1 and solver_runs[0][0] and len(solver_runs[0][1]) == 3
    weights = set()
    for t, (m, (pf, nf)) in enumerate(zip(models, data.split)):
        single = gm.train(pf, nf, C=0.5, tol=TOL, class_weight=cw, **KP)
        assert _file(m, str(tmp_path / "a.txt")) == _file(single, str(tmp_path / "b.txt")), tasks[t]
        assert solver_runs[1 + t][1] == [solver_runs[0][1][t]]
        n1, n0 = int((data.Y[:, t] == 1).sum()), int((data.Y[:, t] == 0).sum())
        assert n1 != n0
        if cw == "balanced":
            assert m.class_weight == ((n0 + n1) / (2 * n0), (n0 + n1) / (2 * n1))
        weights.add(m.class_weight)
    assert len(weights) == (3 if cw == "balanced" else 1)       # "balanced" is resolved per task


# ------------------------------------------------------------------ the grid
GRID_CS = (0.1, 1.0, 10.0)
GRID_WEIGHTS = (None, "balanced", (1.0, 3.0))
NCV, REPEATS, SEED = 5, 2, 1


@pytest.fixture(scope="module")
def grid(data):
    import torch
    from gkmqc_amd import svmcv
    Kd = torch.from_numpy(data.K).cuda()
    runs = []
    real = svmcv.train_tasks

    def spy(*a, **kw):
        sol, handles = real(*a, **kw)
        runs.append([int(i) for i in sol.iters])
        return sol, handles
    svmcv.train_tasks = spy
    try:
        records = svmcv.cross_validate_grid(Kd, NPOS, NNEG, GRID_CS, GRID_WEIGHTS, NCV, REPEATS, SEED, TOL)
    finally:
        svmcv.train_tasks = real
    return dict(Kd=Kd, records=records, runs=runs)


def test_the_grid_is_one_launch(grid):
    assert len(grid["runs"]) == 1 and len(grid["runs"][0]) == len(GRID_CS) * len(GRID_WEIGHTS) * NCV   # (equal repeats solved once)
    assert min(grid["runs"][0]) > 0
    assert [(r["C"], r["class_weight"]) for r in grid["records"]] == [(C, w) for C in GRID_CS for w in GRID_WEIGHTS]
    assert all(r["capped"] == 0 for r in grid["records"])


@pytest.mark.parametrize("C", GRID_CS)
def test_the_unweighted_records_are_crossValidates_floats(data, grid, solver_runs, C):
    from gkmqc_amd import svmcv
    mean, std = svmcv.crossValidate((C, TOL, 0, 512, NCV, REPEATS, 0, SEED), grid["Kd"], NPOS, NNEG)
    assert solver_runs and not solver_runs[0][0]          # (crossValidate itself: the unboxed entry, as ever)
    rec = [r for r in grid["records"] if r["C"] == C and r["class_weight"] is None][0]
    assert _same(rec["auc_mean"], mean) and _same(rec["auc_std"], std)
    assert type(rec["auc_mean"]) is type(mean) and type(rec["auc_std"]) is type(std)


def test_the_weighted_records_are_a_scikit_learn_loop(data, grid):
    from sklearn.metrics import roc_auc_score
    from sklearn.svm import SVC
    from gkmqc_amd import svmcv
    plan = svmcv.plan_folds((None, TOL, 0, None, NCV, REPEATS, 0, SEED), NPOS, NNEG)
    assert plan["n_folds"] == NCV * REPEATS and len(plan["u_trains"]) == NCV
    y = plan["y"]
    assert (y == data.y).all()
    distinct = set()
    for rec in grid["records"]:
        cw = rec["class_weight"]
        aucs = []
        for tr, te in zip(plan["u_trains"], plan["u_tests"]):
            m = SVC(kernel="precomputed", C=rec["C"], tol=TOL, shrinking=False,
                    class_weight=cw if cw is None or isinstance(cw, str) else {0: cw[0], 1: cw[1]})
            m.fit(data.K[np.ix_(tr, tr)], y[tr])
            aucs.append(roc_auc_score(y[te], m.decision_function(data.K[np.ix_(te, tr)])))
        aucs = [aucs[w] for w in plan["which"]]
        assert _same(rec["auc_mean"], np.mean(aucs)) and _same(rec["auc_std"], np.std(aucs)), (rec, np.mean(aucs))
        distinct.add(float(rec["auc_mean"]))
    assert len(distinct) > 1


def test_the_grid_with_shrinking_is_scikit_learns_shrinking_run(data, grid):
    """the grid through the general solver with shrinking: scikit-learn's own shrinking run, fold by fold"""
    from sklearn.metrics import roc_auc_score
    from sklearn.svm import SVC
    from gkmqc_amd import svmcv
    records = svmcv.cross_validate_grid(grid["Kd"], NPOS, NNEG, (1.0,), ((1.0, 3.0),), NCV, 1, SEED, TOL, shrinking=True)
    plan = svmcv.plan_folds((None, TOL, 1, None, NCV, 1, 0, SEED), NPOS, NNEG)
    aucs = []
    for tr, te in zip(plan["u_trains"], plan["u_tests"]):
        m = SVC(kernel="precomputed", C=1.0, tol=TOL, shrinking=True, class_weight={0: 1.0, 1: 3.0})
        m.fit(data.K[np.ix_(tr, tr)], data.y[tr])
        aucs.append(roc_auc_score(data.y[te], m.decision_function(data.K[np.ix_(te, tr)])))
    assert len(records) == 1 and records[0]["capped"] == 0
    assert _same(records[0]["auc_mean"], np.mean(aucs)) and _same(records[0]["auc_std"], np.std(aucs))


# ------------------------------------------------------------------ select and the command lines
def test_select_and_its_tie_rule(data, grid, solver_runs):
    from gkmqc_amd import gkmmodel as gm
    from gkmqc_amd import svmcv
    records, best = gm.select(data.pos_fa, data.neg_fa, GRID_CS, GRID_WEIGHTS, NCV, REPEATS, SEED, tol=TOL, **KP)
    assert len(solver_runs) == 1                               # one Gram matrix, one launch
    for a, b in zip(records, grid["records"]):
        assert (a["C"], a["class_weight"]) == (b["C"], b["class_weight"])
        assert _same(a["auc_mean"], b["auc_mean"]) and _same(a["auc_std"], b["auc_std"])
    top = max(float(r["auc_mean"]) for r in records)
    assert best == [i for i, r in enumerate(records) if float(r["auc_mean"]) == top][0] == svmcv.best_record(records)
    # equal bounds give equal bits, so these two settings tie: the earlier weighting wins
    records, best = gm.select(data.pos_fa, data.neg_fa, (1.0,), ((1.0, 1.0), None), NCV, 1, SEED, tol=TOL, **KP)
    assert _same(records[0]["auc_mean"], records[1]["auc_mean"]) and best == 0
    # C so large that no alpha reaches a bound: the same solution for both, the smaller C wins wherever it stands
    records, best = gm.select(data.pos_fa, data.neg_fa, (1e7, 1e6), (None,), NCV, 1, SEED, tol=TOL, **KP)
    assert _same(records[0]["auc_mean"], records[1]["auc_mean"]) and best == 1


def test_command_lines_end_to_end(data, solver_runs, tmp_path, capsys):
    from gkmqc_amd import gkmmodel as gm
    from gkmqc_amd import gkmpanels as pn
    from gkmqc_amd import gkmselect as gs
    kernel = ["-t", "4", "-L", "6", "-k", "4", "-d", "2"]
    # cv-grid
    out = str(tmp_path / "grid.tsv")
    assert gs.main(["cv-grid"] + kernel + ["-C", "0.1,1,10", "--class-weight", "none,balanced,1:3", "--repeats", "2",
                                          data.pos_fa, data.neg_fa, out]) == 0
    err = capsys.readouterr().err
    records, best = gm.select(data.pos_fa, data.neg_fa, GRID_CS, GRID_WEIGHTS, NCV, REPEATS, SEED, tol=TOL, **KP)
    want = str(tmp_path / "want.tsv")
    gs.write_grid(want, records)
    assert open(out).read() == open(want).read() and len(open(out).read().split("\n")) == 11
    assert [(r["C"], r["class_weight"]) for r in gs.read_grid(out)] == [(r["C"], r["class_weight"]) for r in records]
    assert "9 settings" in err and "best: C %r, class weights %s, mean AUC %r" % (
        float(records[best]["C"]), gs.class_weight_text(records[best]["class_weight"]), float(records[best]["auc_mean"])) in err
    assert not os.path.exists(out + ".tmp")
    # train --class-weight
    for text, cw in (("1:3", (1.0, 3.0)), ("balanced", "balanced"), ("none", None)):
        path = str(tmp_path / "m.txt")
        assert gs.main(["train"] + kernel + ["-C", "0.5", "--class-weight", text, data.pos_fa, data.neg_fa, path]) == 0
        with open(path, "rb") as f:
            got = f.read()
        assert got == _file(gm.train(data.pos_fa, data.neg_fa, C=0.5, class_weight=cw, **KP), str(tmp_path / "w.txt")), text
        assert got.startswith(b"format gkmqc-model-1\n" if cw is None else b"format gkmqc-model-2\n")
    # gkmpanels train --class-weight
    prefix = str(tmp_path / "panel")
    assert pn.main(["train"] + kernel + ["-C", "0.5", "--class-weight", "balanced", data.pool_fa, data.labels_tsv, prefix]) == 0
    _, models = pn.train_panel(data.pool_fa, data.labels_tsv, C=0.5, class_weight="balanced", **KP)
    for task, m in zip(data.tasks, models):
        with open(pn.model_path(prefix, task), "rb") as f:
            assert f.read() == _file(m, str(tmp_path / "w.txt")), task
    assert all(not boxed or min(iters) > 0 for boxed, iters in solver_runs)
