"""CPU reference of the RBF fold of mutant scores, for the mutant-scores tests: the exact tallies of
tests/ism_ref.py folded in numpy, and the brute force that scores every explicit mutant through `score`.  Test
infrastructure; nothing shared with the device code."""
import numpy as np

from tests import ism_ref as R


def delta_g(x, s, kernel_type, L, d, fold_u, fold_b, M=50, H=50.0):
    """dG_s(t, b) = sum over ascending m of fold_u[m] U[t, m] + fold_b[m - 1] B[t, m, b] (B rows m = 1..min(d + 1, L))
    -> float64 (len(x), 4); the own-base column is whatever the tallies give there (callers overwrite it)"""
    U, B = R.tallies(x, s, kernel_type, L, d, M, H)
    mb = min(d + 1, L)
    dg = np.zeros((len(x), 4))
    for m in range(max(d, mb) + 1):
        if m <= d:
            dg += (fold_u[m] * U[:, m].astype(np.float64))[:, None]
        if 1 <= m <= mb:
            dg += fold_b[m - 1] * B[:, m, :].astype(np.float64)
    return dg


def term(dual, G, sq_s, n, gamma):
    """dual exp(gamma (G / (sq_s n) - 1)): product first, one division, then exp"""
    return dual * np.exp(gamma * (G / (sq_s * n) - 1.0))


def rbf_block(queries, svs, kernel_type, L, d, fold_u, fold_b, dual, sq_sv, sq_q, gx, ysq, gamma, M=50, H=50.0, dg=None):
    """The values gkmhip_ism_rbf_block defines, in numpy.  queries / svs: base-code arrays; dual, sq_sv: one per support
    vector; sq_q: one per query; gx[i][j]: raw G(query j, sv i); ysq: one (T, 4) array per query.  dg: delta_g of every
    (query, sv), if the caller keeps them (they do not depend on gamma).
    -> ([out (T, 4) per query, 0.0 at the own base], base per query)"""
    outs, base = [], np.zeros(len(queries))
    for j, x in enumerate(queries):
        out = np.zeros((len(x), 4))
        for i, s in enumerate(svs):
            g = dg[j][i] if dg is not None else delta_g(x, s, kernel_type, L, d, fold_u, fold_b, M, H)
            out += term(dual[i], gx[i][j] + g, sq_sv[i], ysq[j], gamma)
            base[j] += term(dual[i], gx[i][j], sq_sv[i], sq_q[j], gamma)
        out[np.arange(len(x)), np.asarray(x, dtype=np.int64)] = 0.0
        outs.append(out)
    return outs, base


def brute_force(gp, model, queries):
    """score(y) of every explicit single-base mutant y, through `score`; the own-base column is score(x)
    -> [float64 (T, 4) per query]"""
    mutants, index = [], []
    for qi, x in enumerate(queries):
        for t in range(len(x)):
            for b in range(4):
                if b != x[t]:
                    mutants.append(R.mutant(x, t, b))
                    index.append((qi, t, b))
    _, sx = gp.score(model, queries)
    _, sy = gp.score(model, mutants)
    want = [np.repeat(np.full((len(x), 1), sx[qi]), 4, axis=1) for qi, x in enumerate(queries)]
    for (qi, t, b), s in zip(index, sy):
        want[qi][t, b] = s
    return want
