"""tests/smo_ref.py's `solve` restated with a bound per class: LIBSVM's Solver::Solve without shrinking, with
get_C(i) = y_i > 0 ? Cp : Cn wherever C enters -- the reference tests/test_svm_box_gpu.py holds the boxed GPU solvers'
alpha, gradient, rho and iteration count to, itself held to scikit-learn's SVC(class_weight=...) bit for bit on every
problem those tests use (tests/test_svm_box_host.py).

Where C enters (everything else is smo_ref's, see its docstring):

* I_up and I_low in both selections: alpha_k < C_k;
* the two-variable update.  y_i != y_j: the first clipping tests diff > 0, the second diff > C_i - C_j and clips to C_i
  and C_j.  y_i == y_j: one class, C_i == C_j, LIBSVM's `sum > C_i` (first) and `sum > C_j` (second);
* rho: "at the upper bound" is alpha_k >= C_k.

The census counts smo_ref's branches and `clip_split`: updates of a pair with y_i != y_j in which `diff > C_i - C_j` and
`diff > 0` disagree, i.e. the second clipping tests another variable than a single-C solver's would.
"""
import numpy as np

from tests.smo_ref import CENSUS_KEYS as _BASE_KEYS, TAU, Solution

CENSUS_KEYS = _BASE_KEYS + ("clip_split",)


def solve(Ksub, y, p, Cp, Cn, eps, max_iter=10000000):
    """min 0.5 a^T Q a + p^T a, 0 <= a_k <= C_k, y^T a = 0 with Q_ij = y_i y_j Ksub_ij and C_k = Cp (y_k = +1) or Cn, from
    a = 0."""
    Ksub = np.asarray(Ksub, dtype=np.float64)
    l = len(y)
    y = np.asarray(y, dtype=np.float64)
    Kf = Ksub.astype(np.float32)
    Q = (Kf * y.astype(np.float32)[:, None] * y.astype(np.float32)[None, :]).astype(np.float64)
    twoK = 2.0 * Kf.astype(np.float64)
    QD = np.ascontiguousarray(np.diag(Ksub))
    pos = y > 0
    Cp, Cn = float(Cp), float(Cn)
    Cv = np.where(pos, Cp, Cn)
    yl, QDl, Cl = y.tolist(), QD.tolist(), Cv.tolist()
    alpha = np.zeros(l)
    G = np.array(p, dtype=np.float64)
    census = dict.fromkeys(CENSUS_KEYS, 0)
    yG = np.empty(l)
    iters = 0
    while iters < max_iter:
        below, above = alpha < Cv, alpha > 0
        up, low = np.where(pos, below, above), np.where(pos, above, below)
        np.multiply(y, G, out=yG)
        v = np.where(up, -yG, -np.inf)
        i = l - 1 - int(v[::-1].argmax())
        Gmax = float(v[i])
        if Gmax == -np.inf:
            break
        census["tie_first"] += int(np.count_nonzero(v == Gmax) > 1)
        Gmax2 = float(np.where(low, yG, -np.inf).max())
        grad_diff = Gmax + yG
        cand = low & (grad_diff > 0)
        quad = (QD[i] + QD) - twoK[i]
        obj = np.where(cand, -(grad_diff * grad_diff) / np.where(quad > 0, quad, TAU), np.inf)
        j = l - 1 - int(obj[::-1].argmin())
        if obj[j] == np.inf:
            j = -1
        else:
            qc = quad[cand]
            census["sel_quad_neg"] += int(qc.min() < 0)
            census["sel_quad_zero"] += int(np.count_nonzero(qc == 0) > 0)
            census["tie_second"] += int(np.count_nonzero(obj == obj[j]) > 1)
        if Gmax + Gmax2 < eps or j < 0:
            break
        iters += 1
        Qij = float(Q[i, j])
        Gi, Gj = float(G[i]), float(G[j])
        ai, aj = old_i, old_j = float(alpha[i]), float(alpha[j])
        Ci, Cj = Cl[i], Cl[j]
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
            census["clip_split"] += int((diff > Ci - Cj) != (diff > 0))
            if diff > Ci - Cj:
                if ai > Ci:
                    ai, aj = Ci, Ci - diff
                    census["clip2"] += 1
            else:
                if aj > Cj:
                    aj, ai = Cj, Cj + diff
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
            if s > Ci:
                if ai > Ci:
                    ai, aj = Ci, s - Ci
                    census["clip4"] += 1
            else:
                if aj < 0:
                    aj, ai = 0.0, s
                    census["clip5"] += 1
            if s > Cj:
                if aj > Cj:
                    aj, ai = Cj, s - Cj
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
    yG = y * G
    upper, lower = alpha >= Cv, alpha <= 0
    free = ~upper & ~lower
    ub_set = (upper & ~pos) | (lower & ~upper & pos)
    lb_set = (upper & pos) | (lower & ~upper & ~pos)
    if free.any():
        s = 0.0
        for x in yG[free]:
            s += x
        rho = s / int(free.sum())
    else:
        census["rho_no_free"] += 1
        ub = yG[ub_set].min() if ub_set.any() else np.inf
        lb = yG[lb_set].max() if lb_set.any() else -np.inf
        rho = (ub + lb) / 2
    return Solution(alpha, G, float(rho), iters, census, y)


def svc(K, idx, n0, box, tol):
    """C-SVC on K[idx][:, idx], idx in LIBSVM's internal order (svmcv.libsvm_order): the first n0 positions have y = +1 and
    the bound box[0], the rest box[1].  Solution.alpha / grad are what FoldSolutions.alpha[f] / grad[f] hold."""
    idx = np.asarray(idx)
    y = np.where(np.arange(len(idx)) < n0, 1.0, -1.0)
    return solve(K[np.ix_(idx, idx)], y, -np.ones(len(idx)), box[0], box[1], float(tol))
