"""CPU reference of the regions of a scan, for the region tests: the definition in a plain Python loop over
the windows, one at a time, written from the text of the definition and from nothing in gkmqc_amd.

Windows are indexed i = 0 .. nw - 1 and window i starts at base i * stride.  Window i passes when it has a score (NaN
marks a window without one, as `scan` returns it) and score[i] >= threshold by IEEE comparison.  Two consecutive passing
windows p < q belong to one region when q - p <= gap + 1.  A region reports start = p_first * stride, end = p_last *
stride + width, peak (the largest score among its passing windows), summit (the start of the first passing window that
attains the peak) and windows (how many passed)."""
import numpy as np

FIELDS = ("start", "end", "peak", "summit", "windows")


def regions(scores, width, stride, threshold, gap):
    """-> dict of start, end, summit, windows (int64) and peak (float64), one element per region, ascending."""
    scores = np.asarray(scores, dtype=np.float64)
    assert scores.ndim == 1 and int(gap) >= 0 and threshold == threshold
    rows = []            # [first, last, peak, summit, windows] in window indices
    for i, v in enumerate(scores.tolist()):
        if not v >= threshold:      # (False for a NaN)
            continue
        if rows and i - rows[-1][1] <= int(gap) + 1:
            r = rows[-1]
            r[1] = i
            r[4] += 1
            if v > r[2]:            # a later window replaces the summit only when it is strictly larger
                r[2], r[3] = v, i
        else:
            rows.append([i, i, v, i, 1])
    ints = lambda k: np.array([r[k] for r in rows], dtype=np.int64)
    return dict(start=ints(0) * int(stride), end=ints(1) * int(stride) + int(width),
                peak=np.array([r[2] for r in rows], dtype=np.float64), summit=ints(3) * int(stride), windows=ints(4))


def window_regions(scores, threshold, gap):
    """The same in window indices (stride 1, width 1: end = last + 1) -> dict of first, last, summit, windows, peak."""
    r = regions(scores, 1, 1, threshold, gap)
    return dict(first=r["start"], last=r["end"] - 1, summit=r["summit"], windows=r["windows"], peak=r["peak"])


def same(a, b, fields=FIELDS):
    """bit for bit, dtypes included"""
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in fields)
