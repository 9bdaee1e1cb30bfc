"""CPU reference of the scan, for the scan tests: windows cut out one by one and scored as sequences of
their own with tests/lmer_ref.py's table score and the oracle's self profiles -- nothing shared with the device code or
gkmpredict's scan.  Also a plain numpy rendering of the stretch formulation (every l-mer pair of a stretch of windows
compared once per strand and credited to the windows that hold it), which the host tests hold against the oracle.  Test
infrastructure."""
import numpy as np

from tests import explain_ref as R
from tests import lmer_ref as LR


def starts(T, width, stride):
    """window starts 0, stride, ... while start + width <= T, by a plain loop"""
    out, a = [], 0
    while a + width <= T:
        out.append(a)
        a += stride
    return out


def windows(x, width, stride):
    """[(start, the window's bases)]"""
    x = np.asarray(x)
    return [(a, x[a:a + width].copy()) for a in starts(len(x), width, stride)]


def valid_windows(x, width, stride):
    """[bool]: the window holds only codes 0..3, base by base"""
    return [all(int(b) < 4 for b in w) for _, w in windows(x, width, stride)]


def self_profile(w, kernel_type, L, k, d, M=50, H=50.0):
    """the oracle's P_m(w, w), m = 0..d, as int64"""
    return R.profile(w, w, kernel_type, L, k, d, M, H).astype(np.int64)


def profiles(x, width, stride, kernel_type, L, k, d, M=50, H=50.0):
    """(windows, d + 1) int64: the oracle's self profile of every window of a sequence of valid bases"""
    return np.array([self_profile(w, kernel_type, L, k, d, M, H) for _, w in windows(x, width, stride)],
                    dtype=np.int64).reshape(-1, d + 1)


def scores(table, x, width, stride):
    """[(start, score)] of every window of x (codes >= 4 invalid): T(w) / sqrt(sum_m c_m P_m(w, w)) + rho from the table's
    weights and the oracle's profile, NaN where the window holds an invalid base"""
    out = []
    for (a, w), ok in zip(windows(x, width, stride), valid_windows(x, width, stride)):
        if not ok:
            out.append((a, float("nan")))
            continue
        sq = R.self_norm(w, table.kernel_type, table.L, table.k, table.d, table.M, table.H)
        out.append((a, LR.table_score(table, table.W, w) / sq + table.rho))
    return out


def stretch_profiles(x, width, stride, g, kernel_type, L, d, M=50, H=50.0):
    """The stretch formulation in numpy -> ((windows, d + 1) int64 profiles, comparisons made).  The windows are taken g at
    a time; in a stretch every pair (p, q = p + delta), 0 <= delta < n, q inside the stretch, is compared once per strand
    (m(f_p, f_q) and m(rc f_p, f_q)), and a pair within d mismatches adds (2 - [delta = 0]) wt[p - a] wt[q - a] to every
    window [a, a + n) of the stretch that holds both l-mers."""
    f = R.pack(x, L).astype(np.int64)
    n = width - L + 1
    wt = R.weights(kernel_type, n, M, H)
    a_all = starts(len(x), width, stride)
    out = np.zeros((len(a_all), d + 1), dtype=np.int64)
    comparisons = 0
    for w0 in range(0, len(a_all), g):
        a_s = a_all[w0:w0 + g]
        lo, hi = a_s[0], a_s[-1] + n
        for p in range(lo, hi):
            q = np.arange(p, min(p + n, hi))
            comparisons += 2 * len(q)
            mf = LR.mismatches(f[p:p + 1], f[q], L)[0]
            mr = LR.mismatches(LR.rc_codes(f[p:p + 1], L), f[q], L)[0]
            for m_all in (mf, mr):
                for j in np.nonzero(m_all <= d)[0]:
                    for i, a in enumerate(a_s):
                        if a <= p and q[j] < a + n:
                            out[w0 + i, m_all[j]] += (1 if q[j] == p else 2) * wt[p - a] * wt[q[j] - a]
    return out, comparisons
