"""CPU reference of the per-base importance, for the explain tests: plain numpy on packed l-mers, pair by
pair, nothing shared with the device code.  Test infrastructure; the positional weights come from the oracle."""
import ctypes

import numpy as np


def pack(codes, L):
    """l-mers of a base-code array, first base in the highest pair (as the oracle and the device tables pack them)."""
    codes = np.asarray(codes, dtype=np.uint32)
    n = len(codes) - L + 1
    v = np.zeros(n, dtype=np.uint32)
    for i in range(L):
        v = (v << np.uint32(2)) | codes[i:i + n]
    return v


def weights(kernel_type, n, M=50, H=50.0):
    """positional weights of n l-mers: all 1, or the oracle's decay for types 4 / 5"""
    if kernel_type in (4, 5):
        from oracle import oracle as O
        return O.position_weights(kernel_type, n, M, H).astype(np.int64)
    return np.ones(n, dtype=np.int64)


def tallies(x, s, kernel_type, L, d, M=50, H=50.0):
    """H[t, m] (int64, len(x) x (d + 1)): the sum of w_x[p] w_s[q] over the pairs (forward l-mer p of x, forward or
    reverse-complement l-mer q of s) with m <= d mismatches in which base t - p of the l-mer is a matched base."""
    x = np.asarray(x, dtype=np.uint8)
    s = np.asarray(s, dtype=np.uint8)
    u = pack(x, L)
    nx, ns = len(u), len(s) - L + 1
    wx = weights(kernel_type, nx, M, H)
    ws = weights(kernel_type, ns, M, H)
    v = np.concatenate((pack(s, L), pack((3 - s)[::-1], L)))
    wv = np.concatenate((ws, ws[::-1]))                    # wt_rc[q] = wt[ns - 1 - q]
    t = u[:, None] ^ v[None, :]
    mm = (t | (t >> np.uint32(1))) & np.uint32(0x55555555)
    m = np.bitwise_count(mm).astype(np.int64)
    p, q = np.nonzero(m <= d)
    out = np.zeros((len(x), d + 1), dtype=np.int64)
    w = wx[p] * wv[q]
    for i in range(L):
        matched = ((mm[p, q] >> np.uint32(2 * (L - 1 - i))) & np.uint32(1)) == 0
        np.add.at(out, (p[matched] + i, m[p, q][matched]), w[matched])
    return out


def profile(x, s, kernel_type, L, k, d, M=50, H=50.0):
    """the oracle's P_m(x, s), m = 0..d"""
    from oracle import oracle as O
    opt = O.make_opt(kernel_type, L, k, d, M, H)
    x = np.ascontiguousarray(x, dtype=np.uint8)
    s = np.ascontiguousarray(s, dtype=np.uint8)
    prof = np.zeros(d + 1, dtype=np.int32)
    O.lib().gkmo_profile(ctypes.byref(opt), x.ctypes.data_as(ctypes.c_void_p), len(x), s.ctypes.data_as(ctypes.c_void_p),
                         len(s), prof.ctypes.data_as(ctypes.c_void_p))
    return prof


def shares(kernel_type, L, k, d):
    from oracle import oracle as O
    return O.mismatch_weights(kernel_type, L, k)[:d + 1] / (L - np.arange(d + 1))


def self_norm(x, kernel_type, L, k, d, M=50, H=50.0):
    """sqrt(sum_m c_m P_m(x, x)) in ascending m, as the oracle forms it"""
    from oracle import oracle as O
    c = O.mismatch_weights(kernel_type, L, k)
    prof = profile(x, x, kernel_type, L, k, d, M, H)
    g = 0.0
    for m in range(d + 1):
        g += c[m] * float(prof[m])
    return np.sqrt(g)


def sv_norms(model):
    return np.array([self_norm(s, model.kernel_type, model.L, model.k, model.d, model.M, model.H) for s in model.seqs])


def explanation(model, x, norms=None):
    """-> (E, bound): E(x)[t] = sum_s dual_coef_s A_s(x)[t] / (sq_s sq_x), and sum_s |dual_coef_s A_s(x)[t]| / (sq_s sq_x)
    (the scale of the rounding error any summation order makes)."""
    t_, L, k, d, M, H = model.kernel_type, model.L, model.k, model.d, model.M, model.H
    sh = shares(t_, L, k, d)
    sqx = self_norm(x, t_, L, k, d, M, H)
    E = np.zeros(len(x))
    bound = np.zeros(len(x))
    norms = sv_norms(model) if norms is None else norms
    for coef, s, sqs in zip(model.dual_coef(), model.seqs, norms):
        A = tallies(x, s, t_, L, d, M, H).astype(np.float64) @ sh
        scale = coef / (sqs * sqx)
        E += scale * A
        bound += np.abs(scale * A)
    return E, bound
