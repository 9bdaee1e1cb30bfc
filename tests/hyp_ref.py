"""CPU reference of hypothetical importance, for the hypothetical tests: plain numpy on packed l-mers, built
on tests/explain_ref.py and tests/ism_ref.py, nothing shared with the device code.  Test infrastructure."""
import numpy as np

from tests import explain_ref as E
from tests import ism_ref as R


def raw_from_tallies(x, U, B, share, d):
    """raw[t, b] of one support vector from ism_ref.tallies: sum_{m=1..d+1} share[m-1] B[t, m, b] for b != x[t] and
    sum_{m=0..d} share[m] U[t, m] at b == x[t]"""
    raw = np.einsum("tmb,m->tb", B[:, 1:d + 2, :].astype(np.float64), np.asarray(share, dtype=np.float64))
    raw[np.arange(len(x)), np.asarray(x, dtype=np.int64)] = U.astype(np.float64) @ share
    return raw


def hypothetical(model, x, norms=None):
    """-> (hyp, bound), (len(x), 4) each, through the decomposition: sum_s coef_s raw_s(x)[t, b] / sqrt(G(y, y)), with
    G(y, y) from the exact self profiles of every mutant; bound is the same sum of absolute values (the scale of the
    rounding error any summation order makes)."""
    from oracle import oracle as O
    t_, L, k, d, M, H = model.kernel_type, model.L, model.k, model.d, model.M, model.H
    x = np.asarray(x, dtype=np.uint8)
    share = E.shares(t_, L, k, d)
    c = O.mismatch_weights(t_, L, k)[:d + 1]
    norms = E.sv_norms(model) if norms is None else norms
    sqy = np.sqrt(R.self_profiles(x, t_, L, d, M, H).astype(np.float64) @ c)
    hyp = np.zeros((len(x), 4))
    bound = np.zeros((len(x), 4))
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        U, B = R.tallies(x, s, t_, L, d, M, H)
        term = (coef / sqs) * raw_from_tallies(x, U, B, share, d)
        hyp += term
        bound += np.abs(term)
    return hyp / sqy, bound / sqy


def brute_force(model, x, positions=None, norms=None):
    """E(y)[t] for y = x with base t set to b, from explain_ref.explanation on every explicit mutant (b == x[t]: x
    itself); rows outside `positions` (default: all) are NaN"""
    x = np.asarray(x, dtype=np.uint8)
    norms = E.sv_norms(model) if norms is None else norms
    out = np.full((len(x), 4), np.nan)
    own, _ = E.explanation(model, x, norms)
    for t in range(len(x)) if positions is None else positions:
        for b in range(4):
            out[t, b] = own[t] if b == x[t] else E.explanation(model, R.mutant(x, t, b), norms)[0][t]
    return out
