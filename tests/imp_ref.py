"""CPU reference of the per-base importance table, for the importance-table tests: plain numpy from the
definition over the l-mer classes of tests/lmer_ref.py, nothing shared with the device code or gkmpredict.  Test
infrastructure; positional weights, mismatch weights and norms come from the oracle."""
import numpy as np

from tests import explain_ref as R
from tests import lmer_ref as LR


def matches(u, v, L):
    """eq[a, b, i]: base i (from the first base) of code u[a] equals base i of code v[b]"""
    u = np.asarray(u, dtype=np.int64)[:, None, None]
    v = np.asarray(v, dtype=np.int64)[None, :, None]
    sh = 2 * (L - 1 - np.arange(L))[None, None, :]
    return ((u >> sh) & 3) == ((v >> sh) & 3)


def terms(u, v, cv, L, d, share):
    """T[a, j, i] = cv[j] (share[m(u_a, v_j)] [u_a[i] == v_j[i]] + share[m(u_a, rc v_j)] [u_a[i] == rc(v_j)[i]]) with
    share[m] = 0 for m > d: the strands' terms added first, then the product"""
    se = np.zeros(L + 1)
    se[:d + 1] = share[:d + 1]
    v = np.asarray(v, dtype=np.int64)
    ef, er = matches(u, v, L), matches(u, LR.rc_codes(v, L), L)
    sf = se[L - ef.sum(2)][:, :, None]
    sr = se[L - er.sum(2)][:, :, None]
    return (sf * ef + sr * er) * np.asarray(cv, dtype=np.float64)[None, :, None]


def count(u, v, cv, L, d, share):
    """V[a, i] = sum_j T[a, j, i], the classes in ascending j one after the other from 0.0"""
    T = terms(u, v, cv, L, d, share)
    out = np.zeros((len(u), L))
    for j in range(T.shape[1]):
        out += T[:, j, :]
    return out


def count_exact(u, v, cv, L, d):
    """-> int64 (d + 1, len(u), L): the same sum for share = e_m, m = 0..d, and integer cv -- what
    gkmhip_lmer_importance must give exactly"""
    v = np.asarray(v, dtype=np.int64)
    cv = np.asarray(cv).astype(np.int64)
    ef, er = matches(u, v, L), matches(u, LR.rc_codes(v, L), L)
    mf, mr = L - ef.sum(2), L - er.sum(2)
    out = np.zeros((d + 1, len(u), L), dtype=np.int64)
    for m in range(d + 1):
        hit = (ef & (mf == m)[:, :, None]).astype(np.int64) + (er & (mr == m)[:, :, None])
        out[m] = np.einsum("ajl,j->al", hit, cv)
    return out


class _Absolute:
    """a model with every coefficient replaced by its absolute value: its classes bound the terms of the real ones"""

    def __init__(self, model):
        self.L, self.seqs, self.kernel_type, self.M, self.H = model.L, model.seqs, model.kernel_type, model.M, model.H
        self._coef = np.abs(model.dual_coef())

    def dual_coef(self):
        return self._coef


def table(model, u, norms=None):
    """-> (V, bound), (len(u), L) each: V(u, i) from the definition over lmer_ref.classes, and the sum of the absolute
    values of its terms (the scale of the rounding error any summation order makes)."""
    L, d = model.L, model.d
    norms = R.sv_norms(model) if norms is None else norms
    share = R.shares(model.kernel_type, L, model.k, d)
    out = []
    for m in (model, _Absolute(model)):
        cl = LR.classes(m, norms)
        v = np.array(sorted(cl), dtype=np.int64)
        out.append(count(u, v, [cl[int(key)] for key in v], L, d, share))
    return out[0], np.abs(out[1])


def table_by_sv(model, u, norms=None):
    """-> (V, bound) as `table`, support vector by support vector without forming the classes (a trained model has too
    many l-mers for lmer_ref.classes' plain loop)."""
    L, d = model.L, model.d
    norms = R.sv_norms(model) if norms is None else norms
    share = R.shares(model.kernel_type, L, model.k, d)
    V = np.zeros((len(u), L))
    bound = np.zeros((len(u), L))
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        f = R.pack(s, L).astype(np.int64)
        w = R.weights(model.kernel_type, len(f), model.M, model.H).astype(np.float64)
        # a forward l-mer f stands for the pair (f, rc f) whichever of the two is canonical: count() takes both strands
        T = terms(u, f, (coef / sqs) * w, L, d, share)
        V += T.sum(1)
        bound += np.abs(T).sum(1)
    return V, bound


def explain_from_table(model, V_lookup, x):
    """E(x)[t] = sum_{i, 0 <= t-i < n} w_x[t-i] V(u_{t-i}, i) / sq_x.  V_lookup(codes) -> the (len(codes), L) rows."""
    L = model.L
    u = R.pack(x, L).astype(np.int64)
    n = len(u)
    w = R.weights(model.kernel_type, n, model.M, model.H).astype(np.float64)
    rows = np.asarray(V_lookup(u), dtype=np.float64)
    E = np.zeros(len(x))
    for i in range(L):
        E[i:i + n] += w * rows[:, i]
    return E / R.self_norm(x, model.kernel_type, L, model.k, model.d, model.M, model.H)
