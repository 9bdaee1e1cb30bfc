"""Class weights and a C per problem, without a GPU: tests/smo_box_ref.py against scikit-learn's
SVC(class_weight=...) on every problem tests/test_svm_box_gpu.py holds the GPU solvers to, the conditions each of those
problems is there for, svmcv.problem_boxes against scikit-learn's class_weight_, the gkmqc-model-2 file format, and the
parsing of the cv-grid command line.  Exact comparisons throughout."""
import os

import numpy as np
import pytest

from tests import smo_ref
from tests import svm_box_cases as B
from tests import svm_cases as S


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _order(p):
    from gkmqc_amd import svmcv
    return svmcv.libsvm_order(p.train, S.labels(p.case.n))


def _counts(p):
    """support vectors at class 0's bound, at class 1's bound, free"""
    ref, (_, n0), box = B.reference(p), _order(p), B.box_of(p)
    at0, at1 = int((ref.alpha[:n0] >= box[0]).sum()), int((ref.alpha[n0:] >= box[1]).sum())
    return at0, at1, int((ref.alpha > 0).sum()) - at0 - at1


# ------------------------------------------------------------------ the reference against scikit-learn
@pytest.mark.parametrize("p", B.KSMO_PROBLEMS, ids=B.problem_id)
def test_smo_box_ref_is_scikit_learn(built, p):
    """support, dual coefficients, intercept and n_iter_"""
    m, ref = B.sklearn_fit(p), B.reference(p)
    idx, n0 = _order(p)
    sv, coef, rho = smo_ref.svc_sklearn_view(ref, n0)
    where = {g: k for k, g in enumerate(p.train)}
    assert np.array_equal(np.array([where[g] for g in idx[sv]]), m.support_)
    assert _same(coef, m.dual_coef_[0])
    assert _same(rho, m.intercept_[0])
    assert ref.iters == B.iters_of(m) and ref.iters > 0


def test_equal_bounds_are_smo_ref(built):
    """smo_box_ref with Cp == Cn is smo_ref: alpha, gradient, rho, iterations, and every census count they share"""
    from tests import smo_box_ref
    c = B.case("vardiag-600-C1")
    refs = S.svc_reference(c.name)
    from gkmqc_amd import svmcv
    for tr, ref in zip(S.svc_folds(c)[0], refs):
        idx, n0 = svmcv.libsvm_order(tr, S.labels(c.n))
        got = smo_box_ref.svc(S.svc_matrix(c), idx, n0, (c.C, c.C), c.tol)
        assert got.iters == ref.iters and _same(got.alpha, ref.alpha) and _same(got.grad, ref.grad) and got.rho == ref.rho
        assert got.census["clip_split"] == 0
        assert {k: got.census[k] for k in smo_ref.CENSUS_KEYS} == ref.census


# ------------------------------------------------------------------ what each problem is there for
def test_vectors_sit_at_both_bounds_and_the_bounds_differ(built):
    for p, want in zip(B.TABLE, B.TABLE_COUNTS):
        box = B.box_of(p)
        assert box[0] != box[1]
        assert _counts(p) == want, (p.name, _counts(p))
    assert B.reference(B.TABLE[4]).iters == 14076
    both = [p for p in B.TABLE if min(_counts(p)[:2]) > 0]
    assert len(both) >= 3


def test_the_second_clipping_is_decided_by_the_difference_of_the_bounds(built):
    """the census counter of smo_box_ref: updates in which `diff > C_i - C_j` and `diff > 0` disagree; and in some of them
    the second clipping then clips (clip2 / clip3 nonzero beside it)"""
    split = {p.name: B.reference(p).census["clip_split"] for p in B.TABLE + B.BALANCED}
    assert all(v > 0 for v in split.values()), split
    c = B.reference(B.TABLE[0]).census
    assert c["clip2"] + c["clip3"] > 0


def test_balanced_runs_on_an_unbalanced_problem(built):
    from gkmqc_amd import svmcv
    c = B.case("vardiag-600-C1")
    for tr in S.svc_folds(c)[0]:        # on the committed folds "balanced" is no weighting at all
        assert _same(svmcv.problem_weights([S.labels(c.n)[tr]], "balanced"), [[1.0, 1.0]])
    for p in B.BALANCED:
        lab = B.labels_of(p)
        assert (int((lab == 0).sum()), int((lab == 1).sum())) == (263, 37)
        w = B.sklearn_fit(p).class_weight_
        assert _same(w, [300 / (2 * 263), 300 / (2 * 37)]) and 0.5703 < w[0] < 0.5704 and 4.054 < w[1] < 4.055
        at0, at1, _free = _counts(p)
        assert at0 > 0 and at1 > 0, (p.name, at0, at1)


def test_no_free_vector(built):
    """rho is (ub + lb) / 2 with "at the upper bound" judged per class"""
    for p in B.NO_FREE:
        ref = B.reference(p)
        assert ref.census["rho_no_free"] == 1
        assert _counts(p) == (200, 100, 0)
        assert 200 <= ref.iters <= 201


@pytest.mark.parametrize("p", B.SHRINK, ids=B.problem_id)
def test_shrinking_changes_the_path(built, p):
    assert B.iters_of(B.sklearn_fit(p, True)) != B.iters_of(B.sklearn_fit(p, False))


def test_the_documented_shrinking_figures(built):
    p = [q for q in B.SHRINK if q.name == "poly-400-C10/f1/0.25:4/C10"][0]
    assert (B.iters_of(B.sklearn_fit(p, False)), B.iters_of(B.sklearn_fit(p, True))) == (10505, 35871)
    assert "lowrank-400-C10" not in B.SHRINK_NAMES
    assert max(B.iters_of(B.sklearn_fit(q, sh)) for q in B.SHRINK for sh in (False, True)) == 65804


# ------------------------------------------------------------------ problem_boxes
@pytest.mark.parametrize("p", B.TABLE + B.BALANCED + B.NO_FREE + B.TINY, ids=B.problem_id)
def test_problem_boxes_is_class_weight_times_C(built, p):
    from gkmqc_amd import svmcv
    m = B.sklearn_fit(p)
    box = svmcv.problem_boxes([B.labels_of(p)], p.C, p.weights)
    assert box.shape == (1, 2) and box.dtype == np.float64 and box.flags["C_CONTIGUOUS"]
    assert _same(box[0], m.class_weight_ * p.C)
    assert _same(svmcv.problem_weights([B.labels_of(p)], p.weights)[0], m.class_weight_)


def test_problem_boxes_per_problem_arguments(built):
    from gkmqc_amd import svmcv
    labs = [B.labels_of(B.BALANCED[0]), B.labels_of(B.TABLE[0]), B.labels_of(B.TINY[3])]
    box = svmcv.problem_boxes(labs, [0.1, 1.0, 10.0], ["balanced", None, (0.25, 4.0)])
    assert _same(box, [[0.1 * (300 / 526), 0.1 * (300 / 74)], [1.0, 1.0], [2.5, 40.0]])
    assert _same(svmcv.problem_boxes(labs, 3.0, None), np.full((3, 2), 3.0))
    assert _same(svmcv.problem_boxes(labs, 3.0, (1, 2)), [[3.0, 6.0]] * 3)
    assert _same(svmcv.problem_boxes(labs[:2], 1.0, [(1.0, 2.0), (3.0, 4.0)]), [[1.0, 2.0], [3.0, 4.0]])
    # labels other than 0 / 1: the class that sorts first is "label 0"
    assert _same(svmcv.problem_boxes([np.array([-1, 1, 1, 1])], 1.0, "balanced"), [[2.0, 4 / 6]])
    # the product is ONE rounded multiplication
    assert svmcv.problem_boxes([labs[0]], 0.1, (0.3, 0.7))[0, 0] == np.float64(0.1) * np.float64(0.3)


@pytest.mark.parametrize("kw", [
    dict(C=1.0, class_weight=(0.0, 1.0)), dict(C=1.0, class_weight=(1.0, -2.0)), dict(C=1.0, class_weight=(float("nan"), 1.0)),
    dict(C=1.0, class_weight=(1.0, float("inf"))), dict(C=0.0), dict(C=-1.0), dict(C=float("nan")), dict(C=float("inf")),
    dict(C=[1.0, 2.0, 3.0]), dict(C=[1.0, 0.0]), dict(C=1.0, class_weight=[None]), dict(C=1.0, class_weight="balance"),
    dict(C=1.0, class_weight=[(1.0, 2.0), (1.0, 2.0, 3.0)]), dict(C=1e308, class_weight=(10.0, 1.0)),
    dict(C=1e-308, class_weight=(1e-308, 1.0)), dict(C=1.0, class_weight=7), dict(C="x"),
], ids=str)
def test_problem_boxes_refusals(built, kw):
    from gkmqc_amd import svmcv
    labs = [B.labels_of(B.TABLE[0]), B.labels_of(B.TINY[3])]
    with pytest.raises(svmcv.SvmError):
        svmcv.problem_boxes(labs, **kw)


def test_balanced_needs_two_classes(built):
    from gkmqc_amd import svmcv
    with pytest.raises(svmcv.SvmError, match="two classes"):
        svmcv.problem_boxes([np.zeros(4, dtype=int)], 1.0, "balanced")


def test_best_record_tie_rule(built):
    from gkmqc_amd import svmcv
    def rec(C, cw, auc):
        return dict(C=C, class_weight=cw, auc_mean=auc, auc_std=0.0, capped=0)
    assert svmcv.best_record([rec(1.0, None, 0.8), rec(10.0, None, 0.9), rec(100.0, None, 0.85)]) == 1
    assert svmcv.best_record([rec(10.0, None, 0.9), rec(1.0, None, 0.9)]) == 1                      # the smaller C
    assert svmcv.best_record([rec(1.0, None, 0.9), rec(1.0, "balanced", 0.9), rec(10.0, None, 0.9)]) == 0   # then the earlier
    assert svmcv.best_record([rec(1.0, None, 0.5), rec(1.0, "balanced", 0.9), rec(1.0, (1, 2), 0.9)]) == 1


# ------------------------------------------------------------------ the model file
def _model(gm, class_weight=None):
    return gm.Model(4, 5, 3, 2, 50, 50.0, 1.0, 0.1, 1e-3, False, -0.25, 1, [0.1, 0.7], ["neg one", "pos\tone"],
                    [np.zeros(9, np.uint8), np.array([0, 1, 2, 3, 0, 1, 2, 3, 3], np.uint8)], class_weight=class_weight)


PLAIN_TEXT = ("format gkmqc-model-1\nkernel_type 4\nL 5\nk 3\nd 2\nM 50\nH 50.0\ngamma 1.0\nC 0.1\ntol 0.001\nshrinking 0\n"
              "rho -0.25\nn0 1\nn_sv 2\nSV\n0.1\tneg one\tAAAAAAAAA\n0.7\tpos\tone\tACGTACGTT\n")


def test_a_weightless_model_is_saved_as_before(built, tmp_path):
    from gkmqc_amd import gkmmodel as gm
    path = str(tmp_path / "m.txt")
    m = _model(gm)
    assert m.class_weight is None
    m.save(path)
    assert open(path).read() == PLAIN_TEXT
    assert gm.load(path).class_weight is None


def test_model_2_round_trip(built, tmp_path):
    from gkmqc_amd import gkmmodel as gm
    path, again = str(tmp_path / "m.txt"), str(tmp_path / "n.txt")
    w = (300 / 526, 300 / 74)
    m = _model(gm, w)
    m.save(path)
    text = open(path).read()
    assert text == PLAIN_TEXT.replace("gkmqc-model-1", "gkmqc-model-2").replace(
        "C 0.1\n", "C 0.1\nweight0 %r\nweight1 %r\n" % w)
    got = gm.load(path)
    assert got.class_weight == w and got.svm_type == gm.C_SVC and got.C == 0.1 and got.rho == -0.25 and got.n0 == 1
    assert got.alpha.tobytes() == m.alpha.tobytes() and got.names == m.names
    got.save(again)
    assert open(again).read() == text
    assert gm.WEIGHTED_FORMAT == "gkmqc-model-2" and gm.FORMAT == "gkmqc-model-1"


@pytest.mark.parametrize("edit", [
    lambda t: t.replace("weight1 2.0\n", ""),                                   # a weight missing
    lambda t: t.replace("weight0 0.5\n", ""),
    lambda t: t.replace("gkmqc-model-2", "gkmqc-model-1"),                       # weights in a format that has none
    lambda t: t.replace("weight0 0.5", "weight0 0.5\nweight0 0.5"),              # twice
    lambda t: t.replace("weight0 0.5", "weight0 half"),
    lambda t: t.replace("weight0 0.5", "weight0 0.0"),
    lambda t: t.replace("weight1 2.0", "weight1 -2.0"),
    lambda t: t.replace("weight1 2.0", "weight1 nan"),
    lambda t: t.replace("weight1 2.0", "weight1 inf"),
    lambda t: t.replace("weight1 2.0", "weight2 2.0"),
    lambda t: t.replace("gkmqc-model-2", "gkmqc-model-3"),
], ids=range(11))
def test_malformed_weight_keys_are_refused(built, tmp_path, edit):
    from gkmqc_amd import gkmmodel as gm
    path = str(tmp_path / "m.txt")
    _model(gm, (0.5, 2.0)).save(path)
    text = open(path).read()
    assert gm.load(path).class_weight == (0.5, 2.0)
    bad = edit(text)
    assert bad != text
    with open(path, "w") as f:
        f.write(bad)
    with pytest.raises(gm.ModelError):
        gm.load(path)


def test_model_refuses_bad_weights(built):
    from gkmqc_amd import gkmmodel as gm
    for w in ((0.0, 1.0), (1.0, float("nan")), (1.0, float("inf")), (-1.0, 1.0), (1.0,), (1.0, 2.0, 3.0), "balanced", 3.0):
        with pytest.raises(gm.ModelError):
            _model(gm, w)
    with pytest.raises(gm.ModelError, match="only a C-SVC"):
        gm.Model(4, 5, 3, 2, 50, 50.0, 1.0, 0.1, 1e-3, False, -0.25, 0, [0.1], ["a"], [np.zeros(9, np.uint8)],
                 gm.EPSILON_SVR, 0.1, class_weight=(1.0, 2.0))
    assert gm.resolve_class_weight(None, [0, 1]) is None
    assert gm.resolve_class_weight("balanced", [1] * 37 + [0] * 263) == (300 / 526, 300 / 74)
    assert gm.resolve_class_weight((1, 3), [0, 1]) == (1.0, 3.0)
    with pytest.raises(gm.ModelError):
        gm.resolve_class_weight((1, 0), [0, 1])


# ------------------------------------------------------------------ the command line
def test_cv_grid_parsing(built, tmp_path):
    from gkmqc_amd import gkmselect as gs
    from gkmqc_amd.gkmmodel import ModelError
    assert list(gs.COMMANDS) == ["train", "cv-grid"]
    a = gs.build_parser().parse_args(["cv-grid", "-C", "0.01,0.1,1,10", "--class-weight", "none,balanced", "p.fa", "n.fa",
                                      "out.tsv"])
    assert (a.pos_fa, a.neg_fa, a.output, a.ncv, a.repeats, a.seed, a.shrinking) == ("p.fa", "n.fa", "out.tsv", 5, 1, 1, 0)
    assert gs.parse_Cs(a.regularization) == [0.01, 0.1, 1.0, 10.0]
    assert gs.parse_class_weights(a.class_weight) == [None, "balanced"]
    assert gs.parse_class_weights("1:3,balanced,0.25:4") == [(1.0, 3.0), "balanced", (0.25, 4.0)]
    a = gs.build_parser().parse_args(["cv-grid", "p.fa", "n.fa", "out.tsv"])
    assert gs.parse_Cs(a.regularization) == [0.01, 0.1, 1.0, 10.0] and gs.parse_class_weights(a.class_weight) == [None]
    for bad in ("", "1,,2", "1,x", "0", "-1", "nan", "inf"):
        with pytest.raises(ModelError):
            gs.parse_Cs(bad)
    for bad in ("", "balance", "1", "1:2:3", "1:x", "0:1", "1:-1", "nan:1", "1:inf", "none,"):
        with pytest.raises(ModelError):
            gs.parse_class_weights(bad)
    a = gs.build_parser().parse_args(["train", "--class-weight", "1:3", "p.fa", "n.fa", "m.txt"])
    assert gs.parse_class_weight(a.class_weight) == (1.0, 3.0) and a.regularization == 1.0
    assert gs.build_parser().parse_args(["train", "p.fa", "n.fa", "m.txt"]).class_weight == "none"
    # the output file: floats as repr, read back to the same doubles
    records = [dict(C=0.1, class_weight=None, auc_mean=np.float64(2 / 3), auc_std=np.float64(0.1) / 3, capped=0),
               dict(C=10.0, class_weight="balanced", auc_mean=np.float64(0.9), auc_std=np.float64(0.0), capped=2),
               dict(C=10.0, class_weight=(0.25, 1 / 3), auc_mean=np.float64(1.0), auc_std=np.float64(1e-17), capped=0)]
    path = str(tmp_path / "grid.tsv")
    gs.write_grid(path, records)
    lines = open(path).read().split("\n")
    assert lines[0] == gs.GRID_HEADER == "C\tclass_weight\tauc_mean\tauc_std\tcapped"
    assert lines[1] == "0.1\tnone\t%r\t%r\t0" % (2 / 3, 0.1 / 3) and lines[2] == "10.0\tbalanced\t0.9\t0.0\t2"
    assert lines[3] == "10.0\t0.25:%r\t1.0\t1e-17\t0" % (1 / 3) and lines[4:] == [""]
    back = gs.read_grid(path)
    assert [(r["C"], r["class_weight"], float(r["auc_mean"]), float(r["auc_std"]), r["capped"]) for r in records] == \
           [(r["C"], r["class_weight"], r["auc_mean"], r["auc_std"], r["capped"]) for r in back]


def test_command_lines_refuse_before_computing(built, tmp_path, capsys):
    from gkmqc_amd import gkmpanels as pn
    from gkmqc_amd import gkmselect as gs
    fa = str(tmp_path / "s.fa")
    with open(fa, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n")
    out = str(tmp_path / "out")
    assert gs.main(["cv-grid", "-C", "1,zero", fa, fa, out]) == 1
    assert "-C:" in capsys.readouterr().err
    assert gs.main(["cv-grid", "--class-weight", "1:0", fa, fa, out]) == 1
    assert "--class-weight" in capsys.readouterr().err
    assert gs.main(["cv-grid", fa, str(tmp_path / "missing"), out]) == 1
    assert "cannot read" in capsys.readouterr().err
    assert gs.main(["train", "--class-weight", "heavy", fa, fa, out]) == 1
    assert "--class-weight" in capsys.readouterr().err
    tsv = str(tmp_path / "l.tsv")
    with open(tsv, "w") as f:
        f.write("name\tt\na\t1\n")
    assert pn.main(["train", "--class-weight", "1:x", fa, tsv, out]) == 1
    assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("out")]
