"""CPU reference of the l-mer weight table, for the lmer tests: plain numpy from the definition, support
vector by support vector, nothing shared with the device code or gkmpredict's host aggregation.  Test infrastructure;
positional weights, mismatch weights and profiles come from the oracle."""
import numpy as np

from tests import explain_ref as R


def rc_codes(u, L):
    """reverse complements of l-mer codes, base by base"""
    u = np.asarray(u, dtype=np.int64)
    bases = [(u >> (2 * (L - 1 - i))) & 3 for i in range(L)]   # first base first
    r = np.zeros_like(u)
    for b in reversed(bases):
        r = (r << 2) | (3 - b)
    return r


def mismatches(u, v, L):
    """m[i, j]: mismatched bases of l-mer codes u[i] and v[j]"""
    u = np.asarray(u, dtype=np.int64)[:, None]
    v = np.asarray(v, dtype=np.int64)[None, :]
    m = np.zeros((u.shape[0], v.shape[1]), dtype=np.int64)
    for i in range(L):
        m += ((u >> (2 * i)) & 3) != ((v >> (2 * i)) & 3)
    return m


def count(u, v, cv, L, d, c):
    """sum_i cv[i] (c[m(u, v_i)] + c[m(u, rc(v_i))]) with c[m] = 0 for m > d, for every code of u"""
    ce = np.zeros(L + 1)
    ce[:d + 1] = c[:d + 1]
    mf = mismatches(u, v, L)
    mr = mismatches(u, rc_codes(v, L), L)
    return (ce[mf] + ce[mr]) @ np.asarray(cv, dtype=np.float64)


def table(model, u, norms=None):
    """-> (W, bound) at the codes u: W(u) from the definition, and the sum of the absolute values of its terms (the scale
    of the rounding error any summation order makes)."""
    t_, L, k, d = model.kernel_type, model.L, model.k, model.d
    from oracle import oracle as O
    c = O.mismatch_weights(t_, L, k)[:d + 1]
    norms = R.sv_norms(model) if norms is None else norms
    W = np.zeros(len(u))
    bound = np.zeros(len(u))
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        f = R.pack(s, L).astype(np.int64)
        w = R.weights(t_, len(f), model.M, model.H).astype(np.float64)
        terms = count(u, f, (coef / sqs) * w, L, d, c)
        W += terms
        bound += np.abs(count(u, f, np.abs(coef / sqs) * w, L, d, c))
    return W, bound


def classes(model, norms):
    """{canonical code: sum of dual_coef_s / sq_s w_s[q]} with a plain loop over the support vectors and their l-mers"""
    L = model.L
    out = {}
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        f = R.pack(s, L).astype(np.int64)
        w = R.weights(model.kernel_type, len(f), model.M, model.H)
        for q in range(len(f)):
            key = int(min(f[q], rc_codes(f[q:q + 1], L)[0]))
            out[key] = out.get(key, 0.0) + (coef / sqs) * float(w[q])
    return out


def table_score(model, W, x):
    """T(x) = sum_p w_x[p] W(u_p) over the forward l-mers of x"""
    u = R.pack(x, model.L).astype(np.int64)
    w = R.weights(model.kernel_type, len(u), model.M, model.H).astype(np.float64)
    return float(np.dot(w, W[u]))


def oracle_score(model, x, norms):
    """sum_s dual_coef_s G(x, s) / (sq_s sq_x) + rho with G(x, s) = sum_m c_m P_m(x, s) from the oracle's profiles"""
    from oracle import oracle as O
    t_, L, k, d = model.kernel_type, model.L, model.k, model.d
    c = O.mismatch_weights(t_, L, k)[:d + 1]
    sqx = R.self_norm(x, t_, L, k, d, model.M, model.H)
    total = 0.0
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        P = R.profile(x, s, t_, L, k, d, model.M, model.H)
        total += coef * float(np.dot(c, P.astype(np.float64))) / (sqs * sqx)
    return total + model.rho
