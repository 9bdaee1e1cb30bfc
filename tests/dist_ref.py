"""The numpy reference of the score distributions of a scan, not a test: the order-preserving key,
order statistics, quantile ranks and tail counts of an array of window scores in which the unscored windows are NaN --
`scan`'s own output.  Everything sorts and selects on the uint64 keys, never on the doubles."""
import math

import numpy as np

_SIGN, _ALL = np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)


def key(values):
    """b ^ (b >> 63 ? ~0 : 1 << 63) of the bits b of each double"""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    out = b.copy()
    neg = (b >> np.uint64(63)) == 1
    out[neg] = ~b[neg]
    out[~neg] = b[~neg] | _SIGN
    return out


def unkey(keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    out = k.copy()
    pos = (k >> np.uint64(63)) == 1
    out[pos] = k[pos] & ~_SIGN
    out[~pos] = ~k[~pos]
    return out.view(np.float64)


def scored(scores):
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    return scores[~np.isnan(scores)]


def order_statistics(scores, ranks):
    """the ranks[i]-th smallest scored value by key, the very bits"""
    keys = np.sort(key(scored(scores)))
    return unkey(keys[np.asarray(ranks, dtype=np.int64)])


def quantile_ranks(n, q):
    return [min(n - 1, int(math.floor(float(x) * (n - 1)))) for x in q]


def tail_counts(scores, thresholds):
    """scored windows with score >= t, per threshold, by IEEE comparison"""
    v = scored(scores)
    return np.array([int((v >= t).sum()) for t in thresholds], dtype=np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
