"""A numpy restatement of k_panel_weights, for the panel fold tests: per (u, m) a plain loop over the
classes in ascending i, every term a rounded product followed by a rounded add from 0.0.  Test infrastructure; nothing
shared with the device code or gkmpanels' host side."""
import numpy as np

from tests import lmer_ref as LR


def panel_weights(c, v, CV, nm, L, d, u_begin, u_end):
    """-> float64 (u_end - u_begin, nm): P[u - u_begin, m] = sum over ascending i of CV[i, m] * (ce[mf] + ce[mr]) for the
    classes that hit on either strand (min(mf, mr) <= d), ce[m] = c[m] up to d and 0.0 beyond."""
    ce = np.zeros(L + 1)
    ce[:d + 1] = np.asarray(c, dtype=np.float64)[:d + 1]
    u = np.arange(u_begin, u_end, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    CV = np.asarray(CV, dtype=np.float64)
    P = np.zeros((len(u), nm))
    for i in range(len(v)):
        mf = LR.mismatches(u, v[i:i + 1], L)[:, 0]
        mr = LR.mismatches(u, LR.rc_codes(v[i:i + 1], L), L)[:, 0]
        hit = np.minimum(mf, mr) <= d
        term = (ce[mf] + ce[mr])[hit]
        P[hit] = P[hit] + CV[i, :nm][None, :] * term[:, None]
    return P
