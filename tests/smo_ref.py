"""LIBSVM's Solver::Solve without the shrinking heuristic, in plain numpy: the reference the SVM tests hold the GPU
solvers' alpha, gradient, rho and iteration count to (tests/test_svm_kernels_gpu.py), itself held to scikit-learn bit for
bit on every case those tests use (tests/test_svm_kernels_host.py).

Written from the published algorithm (Fan, Chen, Lin 2005, "Working set selection using second order information", as
LIBSVM 3.x implements it) and the description in include/gkm_svm.h:

* kernel values are rounded to float (LIBSVM's Qfloat) wherever a row Q_i is used, the diagonal QD stays double, every
  other operation is fp64;
* both selections scan the positions in ascending order and replace the incumbent on `>=` / `<=`: of equal candidates
  the LAST index wins;
* `quad_coef > 0 ? quad_coef : TAU` in the second selection, `quad_coef <= 0 -> TAU` in the update;
* the gradient update is G_k += (Q_ik dalpha_i + Q_jk dalpha_j), the two products added first;
* rho is the mean of y G over the free positions summed in ascending position, or the midpoint of the bounds when no
  position is free.

The solver counts which of its branches it took (`census`), so that the tests can assert that a case reaches the code it
is there for.
"""
import numpy as np

TAU = 1e-12

CENSUS_KEYS = ("sel_quad_neg", "sel_quad_zero", "upd_quad_neg", "upd_quad_zero", "clip0", "clip1", "clip2", "clip3",
               "clip4", "clip5", "clip6", "clip7", "rho_no_free", "tie_first", "tie_second")


class Solution:
    """alpha, grad (LIBSVM's sign: what FoldSolutions.grad holds) by solver position, rho, iters, census (a dict)"""

    def __init__(self, alpha, grad, rho, iters, census, y):
        self.alpha, self.grad, self.rho, self.iters, self.census, self.y = alpha, grad, rho, iters, census, y


def solve(Ksub, y, p, C, eps, max_iter=10000000):
    """min 0.5 a^T Q a + p^T a, 0 <= a <= C, y^T a = 0 with Q_ij = y_i y_j Ksub_ij, from a = 0.
    Ksub: the (symmetric) kernel matrix of the solver's positions, fp64; y: +-1 per position; p: the linear term."""
    Ksub = np.asarray(Ksub, dtype=np.float64)
    l = len(y)
    y = np.asarray(y, dtype=np.float64)
    Kf = Ksub.astype(np.float32)                    # Qfloat
    Q = (Kf * y.astype(np.float32)[:, None] * y.astype(np.float32)[None, :]).astype(np.float64)   # (Qfloat)(y_i y_k K_ik): signs are exact
    twoK = 2.0 * Kf.astype(np.float64)              # 2 y_i y_k Q_ik = 2 (Qfloat)K_ik, exactly
    QD = np.ascontiguousarray(np.diag(Ksub))        # double
    pos = y > 0
    yl, QDl = y.tolist(), QD.tolist()               # (scalars of the two-variable update as Python floats: the same IEEE doubles)
    alpha = np.zeros(l)
    G = np.array(p, dtype=np.float64)               # alpha = 0: G = p
    census = dict.fromkeys(CENSUS_KEYS, 0)
    yG = np.empty(l)
    iters = 0
    while iters < max_iter:
        # ---- first index: the last argmax over I_up of -y G
        below, above = alpha < C, alpha > 0
        up, low = np.where(pos, below, above), np.where(pos, above, below)
        np.multiply(y, G, out=yG)
        v = np.where(up, -yG, -np.inf)
        i = l - 1 - int(v[::-1].argmax())
        Gmax = float(v[i])
        if Gmax == -np.inf:                         # I_up is empty
            break
        census["tie_first"] += int(np.count_nonzero(v == Gmax) > 1)
        # ---- second index: the last argmin over I_low, grad_diff > 0, of -(grad_diff^2) / quad_coef
        Gmax2 = float(np.where(low, yG, -np.inf).max())
        grad_diff = Gmax + yG
        cand = low & (grad_diff > 0)
        # y_k = +1: QD_i + QD_k - 2 y_i Q_ik;  y_k = -1: QD_i + QD_k + 2 y_i Q_ik
        quad = (QD[i] + QD) - twoK[i]
        obj = np.where(cand, -(grad_diff * grad_diff) / np.where(quad > 0, quad, TAU), np.inf)
        j = l - 1 - int(obj[::-1].argmin())
        if obj[j] == np.inf:                        # no candidate
            j = -1
        else:
            qc = quad[cand]
            census["sel_quad_neg"] += int(qc.min() < 0)
            census["sel_quad_zero"] += int(np.count_nonzero(qc == 0) > 0)
            census["tie_second"] += int(np.count_nonzero(obj == obj[j]) > 1)
        if Gmax + Gmax2 < eps or j < 0:
            break
        iters += 1
        # ---- the two-variable update with LIBSVM's clipping
        Qij = float(Q[i, j])
        Gi, Gj = float(G[i]), float(G[j])
        ai, aj = old_i, old_j = float(alpha[i]), float(alpha[j])
        if yl[i] != yl[j]:
            quad_coef = QDl[i] + QDl[j] + 2 * Qij
            census["upd_quad_neg"] += int(quad_coef < 0)
            census["upd_quad_zero"] += int(quad_coef == 0)
            if quad_coef <= 0:
                quad_coef = TAU
            delta = (-Gi - Gj) / quad_coef
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
                    census["clip0"] += 1
            else:
                if ai < 0:
                    ai, aj = 0.0, -diff
                    census["clip1"] += 1
            if diff > C - C:
                if ai > C:
                    ai, aj = C, C - diff
                    census["clip2"] += 1
            else:
                if aj > C:
                    aj, ai = C, C + diff
                    census["clip3"] += 1
        else:
            quad_coef = QDl[i] + QDl[j] - 2 * Qij
            census["upd_quad_neg"] += int(quad_coef < 0)
            census["upd_quad_zero"] += int(quad_coef == 0)
            if quad_coef <= 0:
                quad_coef = TAU
            delta = (Gi - Gj) / quad_coef
            s = ai + aj
            ai -= delta
            aj += delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
                    census["clip4"] += 1
            else:
                if aj < 0:
                    aj, ai = 0.0, s
                    census["clip5"] += 1
            if s > C:
                if aj > C:
                    aj, ai = C, s - C
                    census["clip6"] += 1
            else:
                if ai < 0:
                    ai, aj = 0.0, s
                    census["clip7"] += 1
        alpha[i], alpha[j] = ai, aj
        dai, daj = ai - old_i, aj - old_j
        G += Q[i] * dai + Q[j] * daj
    else:
        iters = -iters
    # ---- rho
    yG = y * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    ub_set = (upper & ~pos) | (lower & ~upper & pos)
    lb_set = (upper & pos) | (lower & ~upper & ~pos)
    if free.any():
        s = 0.0
        for x in yG[free]:              # in ascending position, from 0.0
            s += x
        rho = s / int(free.sum())
    else:
        census["rho_no_free"] += 1
        ub = yG[ub_set].min() if ub_set.any() else np.inf
        lb = yG[lb_set].max() if lb_set.any() else -np.inf
        rho = (ub + lb) / 2
    return Solution(alpha, G, float(rho), iters, census, y)


def svc(K, idx, n0, C, tol):
    """C-SVC on K[idx][:, idx], idx in LIBSVM's internal order (svmcv.libsvm_order): the first n0 positions have y = +1.
    Solution.alpha / grad are what FoldSolutions.alpha[f] / grad[f] hold."""
    idx = np.asarray(idx)
    y = np.where(np.arange(len(idx)) < n0, 1.0, -1.0)
    return solve(K[np.ix_(idx, idx)], y, -np.ones(len(idx)), float(C), float(tol))


def svc_sklearn_view(sol, n0):
    """(support positions in LIBSVM's order, scikit-learn's dual_coef_[0], intercept_[0]) of a two-class `svc` solution:
    scikit-learn flips the sign of both for a two-class problem"""
    sv = np.nonzero(sol.alpha > 0)[0]
    return sv, -(sol.alpha[sv] * sol.y[sv]), sol.rho


def svr(K, train, z, C, epsilon, tol):
    """epsilon-SVR as LIBSVM's 2l-position problem: position k < l is sample k with y = +1, p = epsilon - z_k, position
    l + k the same sample with y = -1, p = epsilon + z_k."""
    train = np.asarray(train)
    l = len(train)
    zt = np.asarray(z, dtype=np.float64)[train]
    g = np.concatenate((train, train))
    y = np.concatenate((np.ones(l), -np.ones(l)))
    p = np.concatenate((epsilon - zt, epsilon + zt))
    return solve(K[np.ix_(g, g)], y, p, float(C), float(tol))


def svr_sklearn_view(sol):
    """(support_, dual_coef_[0], intercept_[0]) of an `svr` solution"""
    l = len(sol.alpha) // 2
    coef = sol.alpha[:l] - sol.alpha[l:]
    sv = np.nonzero(coef != 0)[0]
    return sv, coef[sv], (-sol.rho if sol.rho != 0 else 0.0)
