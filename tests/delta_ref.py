"""CPU reference of the variant effects, for the delta tests: the definition with Python loops of double
additions -- nothing shared with the device code or gkmpredict's delta.  Sequences are lists / arrays of base codes,
values >= 4 invalid; alleles are strings of A, C, G, T.  Test infrastructure."""
import numpy as np

NAN = float("nan")


def codes_of(text):
    return ["ACGT".index(ch) for ch in text]


def S(W, z, L):
    """((0.0 + W[u_0]) + W[u_1]) + ...: the l-mers of z in order, 0.0 when z is shorter than L"""
    acc = 0.0
    for p in range(len(z) - L + 1):
        u = 0
        for b in z[p:p + L]:
            u = u * 4 + int(b)
        acc = acc + float(W[u])
    return acc


def trim(pos, ref, alt):
    """the common suffix goes first, then the common prefix (which moves pos)"""
    while ref and alt and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    while ref and alt and ref[0] == alt[0]:
        pos, ref, alt = pos + 1, ref[1:], alt[1:]
    return pos, ref, alt


def delta(W, L, x, pos, ref, alt):
    """the delta of one variant of the record x"""
    x = [int(b) for b in x]
    assert all(b >= 4 or b == r for b, r in zip(x[pos:pos + len(ref)], codes_of(ref))) and pos + len(ref) <= len(x)
    pos, ref, alt = trim(pos, ref, alt)
    r = len(ref)
    a, e = max(0, pos - (L - 1)), min(len(x), pos + r + (L - 1))
    if any(b >= 4 for b in x[a:e]):
        return NAN
    return S(W, x[a:pos] + codes_of(alt) + x[pos + r:e], L) - S(W, x[a:e], L)


def saturation(W, L, x):
    """(T, 4): row t, column b = S(context with b at t) - S(context), the context being L - 1 bases on either side of
    t; a row of NaN where it holds an invalid base"""
    x = [int(b) for b in x]
    T = len(x)
    D = np.empty((T, 4))
    for t in range(T):
        a, e = max(0, t - (L - 1)), min(T, t + L)
        if any(b >= 4 for b in x[a:e]):
            D[t] = NAN
            continue
        base = S(W, x[a:e], L)
        for b in range(4):
            D[t, b] = S(W, x[a:t] + [b] + x[t + 1:e], L) - base
    return D


def total(W, x, L):
    """T(x): the plain sum of W over all l-mers of a whole record, and the sum of |W| over them"""
    x = [int(b) for b in x]
    return S(W, x, L), S(np.abs(W), x, L)


def edit(x, pos, ref, alt):
    x = [int(b) for b in x]
    return x[:pos] + codes_of(alt) + x[pos + len(ref):]
