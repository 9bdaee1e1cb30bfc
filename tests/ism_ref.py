"""CPU reference of in-silico mutagenesis, for the ism tests: plain numpy on packed l-mers, pair by pair,
nothing shared with the device code.  Test infrastructure; packing and positional weights as in tests/explain_ref.py."""
import numpy as np

from tests import explain_ref as E


def _pairs(x, s, kernel_type, L, M, H):
    """(u, v, w, mm, m) of every (forward l-mer p of x, forward or reverse-complement l-mer q of s): the packed l-mers, the
    pair weights w_x[p] w_s[q] (int64), the mismatch masks (one bit 2j per mismatched base, j = L - 1 - i) and counts"""
    x = np.asarray(x, dtype=np.uint8)
    s = np.asarray(s, dtype=np.uint8)
    u = E.pack(x, L)
    ns = len(s) - L + 1
    wx = E.weights(kernel_type, len(u), M, H)
    ws = E.weights(kernel_type, ns, M, H)
    v = np.concatenate((E.pack(s, L), E.pack((3 - s)[::-1], L)))
    wv = np.concatenate((ws, ws[::-1]))                    # wt_rc[q] = wt[ns - 1 - q]
    t = u[:, None] ^ v[None, :]
    mm = (t | (t >> np.uint32(1))) & np.uint32(0x55555555)
    m = np.bitwise_count(mm).astype(np.int64)
    return u, v, wx[:, None] * wv[None, :], mm, m


def tallies(x, s, kernel_type, L, d, M=50, H=50.0):
    """-> (U, B), int64.  U[t, m] (len(x) x (d + 1)): the sum of w_x[p] w_s[q] over the pairs with m <= d mismatches in
    which base t - p of the query l-mer is MATCHED.  B[t, m, b] (len(x) x (d + 2) x 4): the same over the pairs with
    1 <= m <= min(d + 1, L) mismatches in which base t - p is MISMATCHED and the support vector's base there is b."""
    _, v, w, mm, m = _pairs(x, s, kernel_type, L, M, H)
    p, q = np.nonzero(m <= min(d + 1, L))
    w, mpq, mmpq, vq = w[p, q], m[p, q], mm[p, q], v[q]
    U = np.zeros((len(x), d + 1), dtype=np.int64)
    B = np.zeros((len(x), d + 2, 4), dtype=np.int64)
    for i in range(L):
        sh = np.uint32(2 * (L - 1 - i))
        mis = ((mmpq >> sh) & np.uint32(1)) == 1
        vb = ((vq >> sh) & np.uint32(3)).astype(np.int64)
        matched = ~mis & (mpq <= d)
        np.add.at(U, (p[matched] + i, mpq[matched]), w[matched])
        np.add.at(B, (p[mis] + i, mpq[mis], vb[mis]), w[mis])
    return U, B


def profile_change(x, U, B, d):
    """dP[t, b, m] = P_m(y, s) - P_m(x, s), y = x with base t set to b (0 where b == x[t]), m = 0..d:
    U[t, m-1] - U[t, m] + B[t, m+1, b] - B[t, m, b]"""
    Um1 = np.concatenate((np.zeros((len(x), 1), np.int64), U[:, :-1]), axis=1)        # U[t, m - 1], 0 at m = 0
    dP = (Um1 - U)[:, None, :] + np.moveaxis(B[:, 1:d + 2, :] - B[:, 0:d + 1, :], 2, 1)
    dP[np.arange(len(x)), np.asarray(x, dtype=np.int64)] = 0
    return dP


def profile(x, y, kernel_type, L, d, M=50, H=50.0):
    """P_m(x, y), m = 0..d, int64 (no int32 limit, unlike the oracle's)"""
    _, _, w, _, m = _pairs(x, y, kernel_type, L, M, H)
    return np.array([w[m == k].sum() for k in range(d + 1)], dtype=np.int64)


def mutant(x, t, b):
    y = np.array(x, dtype=np.uint8)
    y[t] = b
    return y


def self_profiles(x, kernel_type, L, d, M=50, H=50.0, positions=None):
    """P[t, b, m] = P_m(y, y) of every single-base mutant y (b == x[t]: x itself), int64 (len(x) x 4 x (d + 1)); rows
    outside `positions` (default: all) are left at -1"""
    x = np.asarray(x, dtype=np.uint8)
    out = np.full((len(x), 4, d + 1), -1, dtype=np.int64)
    own = profile(x, x, kernel_type, L, d, M, H)
    for t in range(len(x)) if positions is None else positions:
        for b in range(4):
            out[t, b] = own if b == x[t] else profile(mutant(x, t, b), mutant(x, t, b), kernel_type, L, d, M, H)
    return out
