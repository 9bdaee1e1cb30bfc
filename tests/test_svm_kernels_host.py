"""What entitles tests/test_svm_kernels_gpu.py to its references and its cases, checked without a GPU:

* tests/smo_ref.py (LIBSVM's solver without shrinking, numpy) equals scikit-learn bit for bit -- support set, dual
  coefficients, intercept, iteration count -- on every problem the GPU tests compare with it, C-SVC and epsilon-SVR.
  scikit-learn does not return the gradient; the GPU tests take it from smo_ref on the strength of this.
* the CONDITIONS the cases of tests/svm_cases.py are there for, from smo_ref's census of the branches it took and from
  scikit-learn itself, so that an edit of a generator cannot empty the GPU tests silently: strictly negative and zero
  `quad_coef` in selection and update, all eight clipping outcomes, rho without a free vector, ties in both selections,
  a diagonal spread over at least two decades within every fold, shrinking runs that take a path of their own."""
import functools

import numpy as np
import pytest

from tests import smo_ref
from tests import svm_cases as S

pytest.importorskip("sklearn")


def _iters(m):
    return int(np.ravel(m.n_iter_)[0])


@functools.lru_cache(maxsize=None)
def _svc_fits(name, shrinking):
    from sklearn.svm import SVC
    c = [x for x in S.SVC_CASES + S.SHRINK_CASES if x.name == name][0]
    K, y = S.svc_matrix(c), S.labels(c.n)
    trains, _ = S.svc_folds(c)
    return tuple(SVC(kernel="precomputed", C=c.C, tol=c.tol, shrinking=shrinking, cache_size=512).fit(K[tr][:, tr], y[tr])
                 for tr in trains)


def _assert_svc_equal(ref, K, train, y, C, tol):
    """one smo_ref C-SVC solution against scikit-learn fitted on the same fold"""
    from sklearn.svm import SVC
    from gkmqc_amd import svmcv
    idx, n0 = svmcv.libsvm_order(train, y)
    m = SVC(kernel="precomputed", C=C, tol=tol, shrinking=False, cache_size=512).fit(K[train][:, train], y[train])
    _assert_svc_equal_fit(ref, m, idx, n0, train)


def _assert_svc_equal_fit(ref, m, idx, n0, train):
    sv, coef, intercept = smo_ref.svc_sklearn_view(ref, n0)
    pos_in_train = {g: p for p, g in enumerate(train)}
    assert np.array_equal([pos_in_train[g] for g in idx[sv]], m.support_)
    assert coef.tobytes() == m.dual_coef_[0].tobytes()
    assert np.float64(intercept).tobytes() == np.float64(m.intercept_[0]).tobytes()
    assert ref.iters == _iters(m)


@pytest.mark.parametrize("case", S.SVC_CASES, ids=S.svc_case_id)
def test_reference_equals_sklearn_svc(case):
    from gkmqc_amd import svmcv
    y = S.labels(case.n)
    trains, _ = S.svc_folds(case)
    refs, fits = S.svc_reference(case.name), _svc_fits(case.name, False)
    assert len(refs) == len(trains) == 3
    for ref, m, tr in zip(refs, fits, trains):
        idx, n0 = svmcv.libsvm_order(tr, y)
        _assert_svc_equal_fit(ref, m, idx, n0, tr)
        assert ref.iters > 0


@pytest.mark.parametrize("case", S.SVR_CASES, ids=lambda c: c.name)
def test_reference_equals_sklearn_svr(case):
    from sklearn.svm import SVR
    K, z = S.matrix(case.family, case.n, case.seed), S.svr_targets(case.n)
    trains, _ = S.svr_folds(case)
    for ref, tr in zip(S.svr_reference(case.name), trains):
        m = SVR(kernel="precomputed", C=case.C, epsilon=case.epsilon, tol=case.tol, shrinking=False, cache_size=512)
        m.fit(K[tr][:, tr], z[tr])
        sv, coef, intercept = smo_ref.svr_sklearn_view(ref)
        assert np.array_equal(sv, m.support_)
        assert coef.tobytes() == m.dual_coef_[0].tobytes()
        assert np.float64(intercept).tobytes() == np.float64(m.intercept_[0]).tobytes()
        assert ref.iters == _iters(m) and ref.iters > 0


def test_reference_equals_sklearn_on_the_mixed_folds():
    """folds of 2, 65 and 600 samples (the GPU tests solve them in one launch)"""
    from gkmqc_amd import svmcv
    from sklearn.svm import SVR
    K, y, z = S.matrix("vardiag", 600, S.SEED), S.labels(600), S.svr_targets(600)
    trains = S.mixed_folds(600)
    assert [len(t) for t in trains] == [2, 65, 600]
    assert all(len(np.unique(y[t])) == 2 for t in trains)
    for tr in trains:
        idx, n0 = svmcv.libsvm_order(tr, y)
        ref = smo_ref.svc(K, idx, n0, *S.MIXED_SVC)
        _assert_svc_equal(ref, K, tr, y, *S.MIXED_SVC)
        C, eps, tol = S.MIXED_SVR
        ref = smo_ref.svr(K, tr, z, C, eps, tol)
        m = SVR(kernel="precomputed", C=C, epsilon=eps, tol=tol, shrinking=False).fit(K[tr][:, tr], z[tr])
        sv, coef, intercept = smo_ref.svr_sklearn_view(ref)
        assert np.array_equal(sv, m.support_) and coef.tobytes() == m.dual_coef_[0].tobytes()
        assert np.float64(intercept).tobytes() == np.float64(m.intercept_[0]).tobytes() and ref.iters == _iters(m)


# ------------------------------------------------------------------ the conditions
def _census(refs):
    return {k: sum(r.census[k] for r in refs) for k in smo_ref.CENSUS_KEYS}


def test_every_branch_is_taken_by_some_csvc_case():
    total = _census([r for c in S.SVC_CASES for r in S.svc_reference(c.name)])
    assert all(total[k] > 0 for k in smo_ref.CENSUS_KEYS), total


def test_strictly_negative_quad_coef_in_selection_and_update():
    svc = [c.name for c in S.SVC_CASES if all(_census(S.svc_reference(c.name))[k] > 0 for k in ("sel_quad_neg", "upd_quad_neg"))]
    svr = [c.name for c in S.SVR_CASES if all(_census(S.svr_reference(c.name))[k] > 0 for k in ("sel_quad_neg", "upd_quad_neg"))]
    assert svc and svr, (svc, svr)
    # and per family: every krein case, in every fold
    for c in S.SVC_CASES:
        if c.family == "krein":
            assert all(r.census["sel_quad_neg"] > 0 and r.census["upd_quad_neg"] > 0 for r in S.svc_reference(c.name))


def test_zero_quad_coef_and_ties_beside_unequal_diagonals():
    """the duplicated-sample variant: quad_coef == 0 exactly in every fold, and ties in the first selection beyond the
    one of the first iteration, where all gradients are -1; ties in the second selection come from krein"""
    refs = S.svc_reference("vardiag_dup-600-C1")
    for r in refs:
        assert r.census["sel_quad_zero"] > 0 and r.census["upd_quad_zero"] > 0
    assert _census(refs)["tie_first"] > len(refs)
    for c in S.SVC_CASES:
        if c.family == "krein":
            assert all(r.census["tie_second"] > 0 for r in S.svc_reference(c.name))


def test_near_copies_have_a_quad_coef_between_zero_and_tau():
    """vardiag_neardup: a copy in the other class sees quad_coef == 0 against the sample and 0 < quad_coef < TAU against
    its near copy (all three with equal rows, so with equal gradients), and every fold meets the zero in a selection"""
    K = S.matrix("vardiag_neardup", 600, S.SEED)
    src, near, dst = np.arange(S.NDUP), np.arange(S.NDUP, 2 * S.NDUP), np.arange(600 - S.NDUP, 600)
    d = np.diag(K)

    def quad(a, b):
        return (d[a] + d[b]) - 2.0 * K[a, b].astype(np.float32).astype(np.float64)
    assert (quad(dst, src) == 0).all()
    q = quad(dst, near)
    assert (q > 0).all() and (q < smo_ref.TAU).all()
    assert (K[near] == K[src]).sum() == K[src].size - S.NDUP          # equal rows but for the diagonal entry
    for r in S.svc_reference("vardiag_neardup-600-C1"):
        assert r.census["sel_quad_zero"] > 0 and r.census["upd_quad_zero"] > 0


@pytest.mark.parametrize("case", S.SHRINK_CASES, ids=S.svc_case_id)
def test_shrinking_changes_the_path(case):
    """scikit-learn's own iteration count differs between shrinking=True and False on every fold used"""
    a, b = _svc_fits(case.name, True), _svc_fits(case.name, False)
    assert len(a) == (1 if case.whole else 3)
    for x, y in zip(a, b):
        assert _iters(x) != _iters(y), (case.name, _iters(x))


def test_svr_shrinking_changes_the_path():
    from sklearn.svm import SVR
    for case in S.SVR_CASES:
        if not case.shrinking:
            continue
        K, z = S.matrix(case.family, case.n, case.seed), S.svr_targets(case.n)
        for tr in S.svr_folds(case)[0]:
            a, b = (SVR(kernel="precomputed", C=case.C, epsilon=case.epsilon, tol=case.tol, shrinking=sh).fit(K[tr][:, tr], z[tr])
                    for sh in (True, False))
            assert _iters(a) != _iters(b)


def test_varied_diagonals_span_two_decades_in_every_fold():
    seen = 0
    for c in S.SVC_CASES + S.SHRINK_CASES:
        if c.vardiag:
            d = np.abs(np.diag(S.svc_matrix(c)))
            for tr in S.svc_folds(c)[0]:
                assert d[tr].max() / d[tr].min() >= 100, c.name
                seen += 1
    for c in S.SVR_CASES:
        if c.family == "vardiag":
            d = np.abs(np.diag(S.matrix(c.family, c.n, c.seed)))
            for tr in S.svr_folds(c)[0]:
                assert d[tr].max() / d[tr].min() >= 100, c.name
                seen += 1
    d = np.abs(np.diag(S.matrix("vardiag", 600, S.SEED)))
    for tr in S.mixed_folds(600):
        assert d[tr].max() / d[tr].min() >= 100
    assert seen >= 6 * 3


def test_families_are_what_their_names_say():
    """the signs the cases rely on: krein and negshift are indefinite with diagonals of both signs / a constant one,
    lowrank has rank 3, vardiag is positive definite"""
    n = 600
    ev = {f: np.linalg.eigvalsh(S.matrix(f, n, S.SEED)) for f in S.FAMILIES}
    assert ev["krein"][0] < -100 and ev["negshift"][0] < -10 and ev["vardiag"][0] > 0
    assert (np.abs(ev["lowrank"]) > 1e-9 * ev["lowrank"][-1]).sum() == 3
    dk = np.diag(S.matrix("krein", n, S.SEED))
    assert dk.min() < 0 < dk.max()
    assert (np.diag(S.matrix("negshift", n, S.SEED)) == 0.5).all()
    for f in S.FAMILIES + ("vardiag_dup", "vardiag_neardup"):
        K = S.matrix(f, n, S.SEED)
        assert (K == K.T).all()
