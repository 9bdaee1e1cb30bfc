"""CPU reference of the windowed kernel matrices, for the wsim tests: the windows of both records cut out
one by one, the oracle's profile per pair, and G, the norms and K formed in the order the definition states -- nothing
shared with the device code or gkmqc_amd/gkmwindows.py.  Also a plain numpy rendering of the tile and difference-array
formulation (every l-mer pair of a tile of window pairs compared once per strand and credited to the rectangle of window
pairs that hold it), which the host tests hold against the oracle.  Test infrastructure."""
import math

import numpy as np

from tests import explain_ref as R
from tests import lmer_ref as LR
from tests import scan_ref as SR

_PROFILES = {}


def pair_profile(wx, wy, kernel_type, L, k, d):
    """the oracle's P_m(wx, wy), m = 0..d, as int64 (identical pairs looked up once)"""
    key = (kernel_type, L, k, d, wx.tobytes(), wy.tobytes())
    if key not in _PROFILES:
        _PROFILES[key] = R.profile(wx, wy, kernel_type, L, k, d).astype(np.int64)
    return _PROFILES[key]


def forget():
    """drop the profiles looked up so far (a grid of shapes holds tens of thousands of window pairs)"""
    _PROFILES.clear()


def profiles(x, y, width, sx, sy, kernel_type, L, k, d):
    """(nA, nB, d + 1) int64: the oracle's profile of every window of x against every window of y (valid bases only)"""
    wx, wy = SR.windows(x, width, sx), SR.windows(y, width, sy)
    out = np.zeros((len(wx), len(wy), d + 1), dtype=np.int64)
    for i, (_, a) in enumerate(wx):
        for j, (_, b) in enumerate(wy):
            out[i, j] = pair_profile(a, b, kernel_type, L, k, d)
    return out


def coefficients(kernel_type, L, k, d):
    from oracle import oracle as O
    return O.mismatch_weights(kernel_type, L, k)[:d + 1]


def raw(prof, c):
    """G = ((0.0 + c_0 P_0) + c_1 P_1) + ... of one profile, in Python floats"""
    g = 0.0
    for m in range(len(c)):
        g = g + float(c[m]) * float(prof[m])
    return g


def kernel(x, y, width, sx, sy, kernel_type, L, k, d, gamma=1.0):
    """K (nA, nB) by the definition: G / (sq_x sq_y), the product first; exp(gamma (K - 1)) for type 3; NaN in the rows
    and columns of windows that hold a code >= 4.  No unit diagonal."""
    c = coefficients(kernel_type, L, k, d)
    wx, wy = SR.windows(x, width, sx), SR.windows(y, width, sy)
    okx, oky = SR.valid_windows(x, width, sx), SR.valid_windows(y, width, sy)
    sqx = [math.sqrt(raw(pair_profile(a, a, kernel_type, L, k, d), c)) if ok else math.nan for (_, a), ok in zip(wx, okx)]
    sqy = [math.sqrt(raw(pair_profile(b, b, kernel_type, L, k, d), c)) if ok else math.nan for (_, b), ok in zip(wy, oky)]
    K = np.full((len(wx), len(wy)), np.nan)
    for i, (_, a) in enumerate(wx):
        for j, (_, b) in enumerate(wy):
            if okx[i] and oky[j]:
                v = raw(pair_profile(a, b, kernel_type, L, k, d), c) / (sqx[i] * sqy[j])
                K[i, j] = math.exp(gamma * (v - 1)) if kernel_type == 3 else v
    return K


def best(K, x_starts, y_starts, min_separation=0):
    """per row the eligible column with the largest K, the lower one on a tie, by a plain loop -> (y_start, K); eligible:
    not a NaN and the starts at least min_separation apart; (-1, NaN) where none is"""
    out_j, out_k = [], []
    for i, a in enumerate(x_starts):
        bj, bv = -1, math.nan
        for j, b in enumerate(y_starts):
            v = K[i, j]
            if abs(int(a) - int(b)) < min_separation or v != v:
                continue
            if bj < 0 or v > bv:
                bj, bv = j, v
        out_j.append(-1 if bj < 0 else int(y_starts[bj]))
        out_k.append(bv)
    return np.array(out_j, dtype=np.int64), np.array(out_k, dtype=np.float64)


def tile_profiles(x, y, width, sx, sy, gx, gy, L, d):
    """The tile formulation in numpy -> ((nA, nB, d + 1) int64 profiles, comparisons made).  The windows are taken gx by gy
    at a time.  In a tile every forward l-mer p of x under its windows is compared with every forward l-mer q of y under
    its windows once per strand (m(f_p, g_q) and m(rc f_p, g_q)); a pair within d mismatches adds +1, -1, -1, +1 at the
    corners of the rectangle of the tile's window pairs that hold both l-mers in a difference array of its mismatch
    class, and an inclusive 2-D prefix sum per class gives the profiles."""
    f, g = R.pack(x, L).astype(np.int64), R.pack(y, L).astype(np.int64)
    n = width - L + 1
    ax, ay = SR.starts(len(x), width, sx), SR.starts(len(y), width, sy)
    out = np.zeros((len(ax), len(ay), d + 1), dtype=np.int64)
    comparisons = 0
    for i0 in range(0, len(ax), gx):
        tx = ax[i0:i0 + gx]
        for j0 in range(0, len(ay), gy):
            ty = ay[j0:j0 + gy]
            D = np.zeros((d + 1, len(tx) + 1, len(ty) + 1), dtype=np.int64)
            qs = np.arange(ty[0], ty[-1] + n)
            holds_q = [[j for j, b in enumerate(ty) if b <= q < b + n] for q in qs]
            for p in range(tx[0], tx[-1] + n):
                rows = [i for i, a in enumerate(tx) if a <= p < a + n]
                comparisons += 2 * len(qs)
                for mm in (LR.mismatches(f[p:p + 1], g[qs], L)[0], LR.mismatches(LR.rc_codes(f[p:p + 1], L), g[qs], L)[0]):
                    for t in np.nonzero(mm <= d)[0]:
                        cols = holds_q[t]
                        if not rows or not cols:
                            continue
                        assert rows == list(range(rows[0], rows[-1] + 1)) and cols == list(range(cols[0], cols[-1] + 1))
                        D[mm[t], rows[0], cols[0]] += 1
                        D[mm[t], rows[0], cols[-1] + 1] -= 1
                        D[mm[t], rows[-1] + 1, cols[0]] -= 1
                        D[mm[t], rows[-1] + 1, cols[-1] + 1] += 1
            P = D.cumsum(axis=1).cumsum(axis=2)[:, :len(tx), :len(ty)]
            out[i0:i0 + len(tx), j0:j0 + len(ty)] = np.moveaxis(P, 0, 2)
    return out, comparisons
