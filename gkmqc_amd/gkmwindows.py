"""Windowed gkm kernel matrices between two long sequences and the best path through one (§5r).

    window_kernel(x, y, width, ...)   K(i, j): the gkm kernel between window i of x and window j of y, every pair
    window_best(x, y, width, ...)     per window of x the window of y with the largest K, reduced on the device
    window_align(x, y, width, ...)    the best local path through K (Smith-Waterman over the windows), found on the device

A window is `width` bases at starts 0, stride, 2 stride, ...; a pair's value is, bit for bit, the off-diagonal entry that
device.cross_kernel returns for the two windows cut out as sequences.  K covers both strands of y (the kernel compares an
l-mer with the other sequence's l-mers and their reverse complements), so it does NOT tell in which orientation two
windows resemble each other.  No unit diagonal is forced: K of two identical windows is what the division gives.
Kernel types 0..3 only.  The records never enter gkmhip_set_sequences: the device layer (gkm_wsim.hip) compares every
l-mer pair of a tile of window pairs once, not once per window pair that holds it.

Command line:
    python -m gkmqc_amd.gkmwindows matrix --width W [--stride-x S --stride-y S --chunk B] [-t -L -k -d -G] x.fa y.fa out.npz
    python -m gkmqc_amd.gkmwindows best   --width W [... --min-separation B]                             x.fa y.fa out.tsv
    python -m gkmqc_amd.gkmwindows align  --width W --offset o --gap g [--orientation forward|reverse|both ...]  x.fa y.fa out.tsv
"""
import argparse
import math
import os
import sys
import time

import numpy as np

from . import device as dv
from . import gkmpredict as gp
from .gkmquery import _norms_from_profiles

MAX_WIDTH = gp.SCAN_MAX_WIDTH
BLOCK_BYTES = gp.BLOCK_BYTES          # device memory one block of K (windows of x by windows of y, doubles) may take
MATRIX_FORMAT = "gkmqc-window-kernel-1"
_MATRIX_KEYS = ("format", "K", "x_starts", "y_starts", "x_valid", "y_valid", "width")


class WindowError(ValueError):
    pass


def _as_record(what, x):
    """A FASTA path with exactly one record, or an array of base codes (values >= 4 invalid) -> (codes, valid)."""
    if isinstance(x, (str, bytes, os.PathLike)):
        if not os.path.isfile(x):
            raise WindowError("cannot read %s" % x)
        recs = gp.read_long_fasta(x)
        if len(recs) != 1:
            raise WindowError("%s: %s holds %d records; one is needed" % (what, x, len(recs)))
        return recs[0][1], recs[0][2]
    x = np.asarray(x, dtype=np.uint8)
    if x.ndim != 1:
        raise WindowError("%s: a record is a one-dimensional array of base codes" % what)
    valid = x < 4
    return np.where(valid, x, 0).astype(np.uint8), valid


def windows_per_chunk(width, stride, chunk):
    """Windows of one chunk of `chunk` bases (scan_chunk_plan's count)."""
    return (max(int(chunk), int(width)) - int(width)) // int(stride) + 1


def default_chunks(width, stride_x, stride_y, budget=BLOCK_BYTES):
    """(bases per chunk of x, of y): the same number of windows on either axis, their block of doubles within `budget`."""
    per = max(1, math.isqrt(int(budget) // 8))
    return (per - 1) * int(stride_x) + int(width), (per - 1) * int(stride_y) + int(width)


def check_window_kernel(x_len, y_len, width, stride_x=1, stride_y=None, kernel_type=0, L=11, k=7, d=3, gamma=1.0,
                        chunk=None, min_separation=0, what="window_kernel"):
    """What window_kernel and window_best refuse, before the device is touched (x_len, y_len: the records' bases)."""
    stride_y = stride_x if stride_y is None else stride_y
    if int(kernel_type) in (4, 5):
        raise WindowError("%s: kernel type %d weights an l-mer by its position in the sequence; a pair of l-mers would "
                          "count differently in every window pair that holds it, and a centre weight belongs to a "
                          "summit-centred peak, not to a sliding window: use types 0..3" % (what, kernel_type))
    bad = dv.check_parameters(int(kernel_type), int(L), int(k), int(d))
    if bad:
        raise WindowError("%s: %s" % (what, bad))
    if int(width) < int(L):
        raise WindowError("%s: the width %d is below L = %d" % (what, width, L))
    if int(width) > MAX_WIDTH:
        raise WindowError("%s: the width %d is above %d, the longest sequence the kernel is defined for"
                          % (what, width, MAX_WIDTH))
    if int(stride_x) < 1 or int(stride_y) < 1:
        raise WindowError("%s: the strides must be at least 1" % what)
    if not math.isfinite(float(gamma)):
        raise WindowError("%s: gamma must be a finite number" % what)
    if int(min_separation) < 0:
        raise WindowError("%s: the minimum separation must not be negative" % what)
    for name, T in (("x", x_len), ("y", y_len)):
        if int(T) < int(width):
            raise WindowError("%s: the record %s (%d bases) holds no window of %d bases" % (what, name, T, width))
    if chunk is not None:
        if int(chunk) < int(width):
            raise WindowError("%s: a chunk must hold at least one window (%d bases)" % (what, width))
        cells = windows_per_chunk(width, stride_x, chunk) * windows_per_chunk(width, stride_y, chunk)
        if cells * 8 > BLOCK_BYTES:
            raise WindowError("%s: a chunk of %d bases makes blocks of %d window pairs; at most %d fit the device budget"
                              % (what, chunk, cells, BLOCK_BYTES // 8))


class _Axis:
    """One chunk of one record on the device: its windows [w0, w1), their first base b0, the chunk's nlm l-mer words
    (int32 tensor lm) and the windows' norms sq (float64 tensor, NaN where the window covers an invalid base)."""
    __slots__ = ("w0", "w1", "b0", "lm", "nlm", "sq")


def _axis_chunks(ctx, codes, valid, width, stride, chunk, c, dev, stream, ones):
    """The chunks of one record, a generator of _Axis: per chunk the upload, the l-mer words (k_scan_lmers) and the
    windows' self profiles with all-ones weights (k_scan_profiles), formed into norms exactly as `scan` forms them."""
    import torch
    L, d = ctx.L, ctx.d
    for w0, w1, b0, b1 in gp.scan_chunk_plan(len(codes), width, stride, chunk):
        ax = _Axis()
        ax.w0, ax.w1, ax.b0, ax.nlm = w0, w1, b0, b1 - b0 - L + 1
        d_codes = torch.from_numpy(np.ascontiguousarray(codes[b0:b1])).to(dev)
        d_valid = torch.from_numpy(np.ascontiguousarray(valid[b0:b1]).view(np.uint8)).to(dev)
        ax.lm = torch.empty(ax.nlm, dtype=torch.int32, device=dev)
        ctx.scan_lmers(d_codes.data_ptr(), d_valid.data_ptr(), b1 - b0, ax.lm.data_ptr(), stream)
        prof = torch.empty((w1 - w0, d + 1), dtype=torch.int64, device=dev)
        ctx.scan_profiles(ax.lm.data_ptr(), ax.nlm, ones.data_ptr(), width, stride, w1 - w0, prof.data_ptr(), stream)
        ax.sq = _norms_from_profiles(prof, c)
        ok = torch.from_numpy(gp.window_validity(valid[b0:b1], width, stride)).to(dev)
        ax.sq.masked_fill_(~ok, float("nan"))
        yield ax


def _blocks(what, x, y, width, stride_x, stride_y, kernel_type, L, k, d, gamma, device, chunk, min_separation, on_chunk,
            descending_y=False):
    """The chunk-pair loop the entry points share, a generator of (info, ax, ay, K, ctx, stream): K the finished block
    (windows of ax by windows of ay, a float64 device tensor).  The first item is the dict of the result's host arrays.
    The norms of a chunk are formed once: those of y before the loop, those of x once per chunk of x.  descending_y: per
    chunk of x the chunks of y from the last to the first (the blocks themselves are the same)."""
    import torch
    xc, xv = _as_record(what, x)
    yc, yv = _as_record(what, y)
    stride_y = stride_x if stride_y is None else stride_y
    check_window_kernel(len(xc), len(yc), width, stride_x, stride_y, kernel_type, L, k, d, gamma, chunk, min_separation, what)
    width, sx, sy = int(width), int(stride_x), int(stride_y)
    chunk_x, chunk_y = default_chunks(width, sx, sy) if chunk is None else (int(chunk), int(chunk))
    nA, nB = gp.scan_window_count(len(xc), width, sx), gp.scan_window_count(len(yc), width, sy)
    yield dict(x_starts=np.arange(nA, dtype=np.int64) * sx, y_starts=np.arange(nB, dtype=np.int64) * sy,
               x_valid=gp.window_validity(xv, width, sx), y_valid=gp.window_validity(yv, width, sy))
    ctx = dv.cached_context(int(kernel_type), int(L), int(k), int(d), gamma=float(gamma), device=device)
    dev = torch.device("cuda", device)
    c = dv.mismatch_weights(int(kernel_type), int(L), int(k))[:int(d) + 1]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        ones = torch.ones(width - int(L) + 1, dtype=torch.uint8, device=dev)
        y_chunks = list(_axis_chunks(ctx, yc, yv, width, sy, chunk_y, c, dev, stream, ones))
        for ax in _axis_chunks(ctx, xc, xv, width, sx, chunk_x, c, dev, stream, ones):
            for ay in (y_chunks[::-1] if descending_y else y_chunks):
                t0 = time.perf_counter()
                nwx, nwy = ax.w1 - ax.w0, ay.w1 - ay.w0
                K = torch.empty((nwx, nwy), dtype=torch.float64, device=dev)
                ctx.wsim_profiles(ax.lm.data_ptr(), ax.nlm, ay.lm.data_ptr(), ay.nlm, width, sx, sy, nwx, nwy, K.data_ptr(),
                                  nwy, None, stream)
                info = None
                if on_chunk is not None:
                    info = dict(x_windows=nwx, y_windows=nwy, profile_kernel_ms=ctx.last_kernel_ms(),
                                comparisons=ctx.last_comparisons(), kernel=ctx.last_kernel_name(), t0=t0)
                ctx.wsim_normalize(K.data_ptr(), nwy, nwx, nwy, ax.sq.data_ptr(), ay.sq.data_ptr(), stream)
                yield info, ax, ay, K, ctx, stream


def _report(on_chunk, info):
    if on_chunk is not None:
        info["wall_ms"] = (time.perf_counter() - info.pop("t0")) * 1e3
        on_chunk(info)


def window_kernel(x, y, width, stride_x=1, stride_y=None, kernel_type=0, L=11, k=7, d=3, gamma=1.0, device=0, chunk=None,
                  on_chunk=None):
    """The gkm kernel between every window of `width` bases of x (starts 0, stride_x, ...) and every window of y (stride_y,
    stride_x when None) -> dict(K float64 (nA, nB), x_starts, y_starts int64, x_valid, y_valid bool).  x, y: a FASTA path
    with one record, or an array of base codes (values >= 4 invalid), of any length.  K[i, j] is, bit for bit, the
    off-diagonal entry device.cross_kernel gives for the two windows cut out, whatever `chunk`; the rows and columns of
    windows over a non-ACGT character are NaN.  K covers both strands of y and does not tell orientation; no unit
    diagonal is forced.  Kernel types 0..3 (check_window_kernel).  chunk: bases per device chunk on either axis
    (default_chunks).  on_chunk(dict) (measurements): called after every pair of chunks with its windows,
    k_wsim_profiles' milliseconds (HIP events), its l-mer comparisons and the pair's wall time."""
    blocks = _blocks("window_kernel", x, y, width, stride_x, stride_y, kernel_type, L, k, d, gamma, device, chunk, 0, on_chunk)
    out = next(blocks)
    out["K"] = np.empty((len(out["x_starts"]), len(out["y_starts"])), dtype=np.float64)
    for info, ax, ay, K, _, _ in blocks:
        out["K"][ax.w0:ax.w1, ay.w0:ay.w1] = K.cpu().numpy()
        _report(on_chunk, info)
    return out


def better(v, j, bv, bj):
    """k_wsim_best's rule, elementwise on arrays: the candidate (v, j) replaces (bv, bj) when it names a column at all
    (j >= 0) and the other names none, or its value is larger, or the values are equal and its column is the lower one.
    Exact and associative; a candidate's value is never a NaN where j >= 0."""
    with np.errstate(invalid="ignore"):
        return (j >= 0) & ((bj < 0) | (v > bv) | ((v == bv) & (j < bj)))


def combine_best(parts):
    """[(best_j, best_k)] of the same rows over consecutive column ranges, columns already global -> (best_j, best_k)
    of the rows over all of them, by `better`."""
    bj, bv = np.array(parts[0][0], dtype=np.int64), np.array(parts[0][1], dtype=np.float64)
    for j, v in parts[1:]:
        j, v = np.asarray(j, dtype=np.int64), np.asarray(v, dtype=np.float64)
        take = better(v, j, bv, bj)
        bj[take], bv[take] = j[take], v[take]
    return bj, bv


def window_best(x, y, width, stride_x=1, stride_y=None, kernel_type=0, L=11, k=7, d=3, gamma=1.0, device=0, chunk=None,
                on_chunk=None, min_separation=0):
    """Per window of x the window of y with the largest K of window_kernel's matrix, the lower start on a tie, among the
    windows of y whose start lies at least `min_separation` bases from the window of x's start and whose K is not a NaN
    -> dict(x_starts int64, y_start int64 (-1: none), K float64 (NaN: none), x_valid, y_valid).  With y = x and
    min_separation = width the best non-overlapping window: internal repeats.  The matrix stays on the device: per pair
    of chunks one value and one index per window of x leave it, combined here by the same rule; the same bytes for
    every `chunk`."""
    import torch
    blocks = _blocks("window_best", x, y, width, stride_x, stride_y, kernel_type, L, k, d, gamma, device, chunk,
                     min_separation, on_chunk)
    out = next(blocks)
    nA = len(out["x_starts"])
    sx = int(stride_x)
    sy = sx if stride_y is None else int(stride_y)
    bj, bv = np.full(nA, -1, dtype=np.int64), np.full(nA, np.nan)
    for info, ax, ay, K, ctx, stream in blocks:
        nwx, nwy = ax.w1 - ax.w0, ay.w1 - ay.w0
        d_j = torch.empty(nwx, dtype=torch.int64, device=K.device)
        d_k = torch.empty(nwx, dtype=torch.float64, device=K.device)
        ctx.wsim_best(K.data_ptr(), nwy, nwx, nwy, ax.b0, sx, ay.b0, sy, int(min_separation), d_j.data_ptr(), d_k.data_ptr(),
                      stream)
        j, v = d_j.cpu().numpy(), d_k.cpu().numpy()
        j = np.where(j >= 0, j + ay.w0, -1)
        rows = slice(ax.w0, ax.w1)
        bj[rows], bv[rows] = combine_best([(bj[rows], bv[rows]), (j, v)])
        _report(on_chunk, info)
    out["y_start"] = np.where(bj >= 0, bj * sy, -1)
    out["K"] = bv
    return out


# ------------------------------------------------------------------ alignment
ORIENTATIONS = ("forward", "reverse", "both")
TRACE_BYTES = 1 << 32                 # device memory the direction bytes of window_align (one per window pair) may take


def check_window_align(x_len, y_len, width, stride_x=1, stride_y=None, kernel_type=0, L=11, k=7, d=3, gamma=1.0, offset=None,
                       gap=None, orientation="forward", chunk=None, path=True, trace_bytes=TRACE_BYTES, what="window_align"):
    """What window_align refuses, before the device is touched: everything check_window_kernel refuses, an offset that
    is missing or not finite, a gap penalty that is missing, negative or not finite, an unknown orientation, and with
    path=True more window pairs than `trace_bytes` direction bytes."""
    check_window_kernel(x_len, y_len, width, stride_x, stride_y, kernel_type, L, k, d, gamma, chunk, 0, what)
    stride_y = stride_x if stride_y is None else stride_y
    if offset is None or not math.isfinite(float(offset)):
        raise WindowError("%s: the offset (the K a window pair must exceed to gain) must be a finite number" % what)
    if gap is None or not math.isfinite(float(gap)) or float(gap) < 0:
        raise WindowError("%s: the gap penalty must be a finite number that is not negative" % what)
    if orientation not in ORIENTATIONS:
        raise WindowError("%s: the orientation must be one of %s" % (what, ", ".join(ORIENTATIONS)))
    nA, nB = gp.scan_window_count(int(x_len), int(width), int(stride_x)), gp.scan_window_count(int(y_len), int(width), int(stride_y))
    if path and nA * nB > int(trace_bytes):
        raise WindowError("%s: %d x %d windows need %d direction bytes on the device, above trace_bytes = %d: use larger "
                          "strides, path=False (the score and the end only) or a larger trace_bytes"
                          % (what, nA, nB, nA * nB, int(trace_bytes)))


def better_cell(a, b):
    """k_walign_tiles' rule for (H, i, c) triples: a replaces b when its H is larger, or the same positive H lies at a
    lower i, then a lower c.  Exact and associative; (0.0, -1, -1) stands for no cell."""
    return a[0] > b[0] or (a[0] == b[0] and a[0] > 0.0 and (a[1], a[2]) < (b[1], b[2]))


def _align_one(xa, ya, width, stride_x, stride_y, kernel_type, L, k, d, gamma, offset, gap, flip, device, chunk, path, on_chunk):
    """One orientation: the DP carried across _blocks' chunk pairs, then one trace -> (host arrays of _blocks, score,
    end (i, c), pairs (n, 2) int64 ascending, in DP coordinates).  On the device: a row vector over all windows of y
    (H of the last row done, per DP column), a column vector per chunk of x, the corner of the next block, D."""
    import torch
    blocks = _blocks("window_align", xa, ya, width, stride_x, stride_y, kernel_type, L, k, d, gamma, device, chunk, 0, on_chunk,
                     descending_y=flip)
    out = next(blocks)
    nA, nB = len(out["x_starts"]), len(out["y_starts"])
    row = D = col = corner = ctx = stream = None
    bests = []
    at = -1
    for info, ax, ay, K, ctx, stream in blocks:
        dev = K.device
        nwx, nwy = ax.w1 - ax.w0, ay.w1 - ay.w0
        if row is None:
            row = torch.zeros(nB, dtype=torch.float64, device=dev)
            D = torch.empty((nA, nB), dtype=torch.uint8, device=dev) if path else None
        if ax.w0 != at:                                        # a new row of blocks: H(., -1) = 0 and so is its corner
            at = ax.w0
            col = torch.zeros(nwx, dtype=torch.float64, device=dev)
            corner = torch.zeros(1, dtype=torch.float64, device=dev)
        c0 = nB - ay.w1 if flip else ay.w0                     # the block's first DP column
        saved = row[c0 + nwy - 1:c0 + nwy].clone()             # H(i0 - 1, c1 - 1): the corner of the block to the right
        need = dv.walign_scratch_bytes(nwx, nwy)
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        bh = torch.empty(1, dtype=torch.float64, device=dev)
        bic = torch.empty(2, dtype=torch.int64, device=dev)
        ctx.walign_block(K.data_ptr(), nwy, nwx, nwy, flip, offset, gap, row.data_ptr() + 8 * c0, col.data_ptr(),
                         corner.data_ptr(), None if D is None else D.data_ptr() + ax.w0 * nB + c0, nB, bh.data_ptr(),
                         bic.data_ptr(), scratch.data_ptr(), need, stream)
        corner = saved
        bests.append((bh, bic, ax.w0, c0))
        if on_chunk is not None:
            info["align_kernel_ms"] = ctx.last_kernel_ms()
        _report(on_chunk, info)
    best = (0.0, -1, -1)
    for bh, bic, i0, c0 in bests:                              # (the first read waits for the stream)
        i, c = bic.tolist()
        if i >= 0 and better_cell((bh.item(), i + i0, c + c0), best):
            best = (bh.item(), i + i0, c + c0)
    pairs = np.zeros((0, 2), dtype=np.int64)
    if path and best[1] >= 0:
        cap = min(nA, nB)
        d_path = torch.empty((cap, 2), dtype=torch.int32, device=D.device)
        d_count = torch.empty(3, dtype=torch.int64, device=D.device)
        ctx.walign_trace(D.data_ptr(), nB, nA, nB, best[1], best[2], d_path.data_ptr(), cap, d_count.data_ptr(), stream)
        n = int(d_count[0].item())
        pairs = d_path[:n].cpu().numpy().astype(np.int64)[::-1]
    return out, best[0], (best[1], best[2]), pairs


def window_align(x, y, width, stride_x=1, stride_y=None, kernel_type=0, L=11, k=7, d=3, gamma=1.0, offset=None, gap=None,
                 orientation="forward", device=0, chunk=None, path=True, trace_bytes=TRACE_BYTES, on_chunk=None):
    """The best local path through window_kernel's matrix: the chain of window pairs of x and y that resemble each other,
    with its insertions and deletions, found on the device beside the blocks of K (which never leave it).  Smith-Waterman
    with a linear gap penalty in doubles: a matched pair (i, j) gains K[i, j] - offset, a window skipped on either axis
    costs gap; offset and gap are required (with offset 0 every pair gains and the alignment is the whole matrix).  A
    pair whose K is NaN (a window over a non-ACGT character) is never matched but may be skipped at the gap's cost.
    orientation: "forward" (y ascending along the path), "reverse" (y descending: an inverted element; K itself covers
    both strands and does not tell) or "both" (the two runs one after the other -- K is computed twice -- and the larger
    score, forward on a tie).
    -> dict(score, orientation, end, start, x_index, y_index, x_start, y_start, x_valid, y_valid): the score is the
    largest H (0.0: no pair gains; the path is empty, end and start (-1, -1)); end = (i, j), the last matched pair in x's
    order, the best cell (the lower i, then the lower DP column on a tie); start = the first matched pair; the matched
    pairs as window indices and as base starts, ascending in x; j in y's own numbering whatever the orientation.  With
    path=False no direction bytes are kept: dict(score, orientation, end) only.  The same bytes for every `chunk`, and
    bit for bit what a plain loop over window_kernel's K gives.  trace_bytes: the most direction bytes (one per window
    pair) the device may hold.  on_chunk(dict): as window_kernel's, with align_kernel_ms, the DP's milliseconds for the
    block.  The K along the path is not returned (the blocks are gone when the path is known): window_kernel on the
    path's span gives it."""
    xc, xv = _as_record("window_align", x)
    yc, yv = _as_record("window_align", y)
    check_window_align(len(xc), len(yc), width, stride_x, stride_y, kernel_type, L, k, d, gamma, offset, gap, orientation, chunk,
                       path, trace_bytes)
    xa, ya = np.where(xv, xc, 4).astype(np.uint8), np.where(yv, yc, 4).astype(np.uint8)
    got = None
    for name in (("forward", "reverse") if orientation == "both" else (orientation,)):
        r = _align_one(xa, ya, width, stride_x, stride_y, kernel_type, L, k, d, gamma, float(offset), float(gap),
                       name == "reverse", device, chunk, path, on_chunk)
        if got is None or r[1] > got[1][1]:
            got = (name, r)
    name, (out, score, (ei, ec), pairs) = got
    nB = len(out["y_starts"])
    to_y = (lambda c: nB - 1 - c) if name == "reverse" else (lambda c: c)
    res = dict(score=score, orientation=name, end=(ei, to_y(ec) if ei >= 0 else -1))
    if not path:
        return res
    xi, yi = pairs[:, 0], to_y(pairs[:, 1])
    res.update(start=(int(xi[0]), int(yi[0])) if len(xi) else (-1, -1), x_index=xi, y_index=yi, x_start=out["x_starts"][xi],
               y_start=out["y_starts"][yi], x_valid=out["x_valid"], y_valid=out["y_valid"])
    return res


# ------------------------------------------------------------------ files
ALIGN_FORMAT = "#score\t%.17g\torientation\t%s\tend\t%d\t%d\tstart\t%d\t%d\tpairs\t%d\n"


def write_window_align(path, result):
    """The `align` output: a header line #score<TAB>score (%.17g)<TAB>orientation<TAB>name<TAB>end<TAB>i<TAB>j<TAB>start
    <TAB>i<TAB>j<TAB>pairs<TAB>n (window indices), then x_start<TAB>y_start (0-based bases) per matched pair, ascending
    in x."""
    with open(path, "w") as f:
        f.write(ALIGN_FORMAT % ((result["score"], result["orientation"]) + tuple(result["end"]) + tuple(result["start"])
                                + (len(result["x_start"]),)))
        f.write("".join("%d\t%d\n" % p for p in zip(result["x_start"].tolist(), result["y_start"].tolist())))


def read_window_align(path):
    """-> dict(score, orientation, end, start, x_start, y_start) from a file written by write_window_align."""
    with open(path) as f:
        lines = f.read().split("\n")[:-1]
    head = lines[0].split("\t") if lines else []
    if len(head) != 12 or [head[i] for i in (0, 2, 4, 7, 10)] != ["#score", "orientation", "end", "start", "pairs"] \
            or head[3] not in ORIENTATIONS[:2]:
        raise WindowError("%s: no window alignment header" % path)
    try:
        out = dict(score=float(head[1]), orientation=head[3], end=(int(head[5]), int(head[6])), start=(int(head[8]), int(head[9])))
        rows = [(int(a), int(b)) for a, b in (line.split("\t") for line in lines[1:])]
        count = int(head[11])
    except ValueError:
        raise WindowError("%s: expected a number, window indices and two integers per line" % path)
    if count != len(rows):
        raise WindowError("%s: the header announces %d pairs, %d follow" % (path, count, len(rows)))
    out["x_start"] = np.array([r[0] for r in rows], dtype=np.int64)
    out["y_start"] = np.array([r[1] for r in rows], dtype=np.int64)
    return out


def write_window_kernel(path, result, width):
    """The `matrix` output: an uncompressed .npz (np.savez) of K, the two start arrays, the two validity masks, the width
    and a format tag."""
    with open(path, "wb") as f:
        np.savez(f, format=np.array(MATRIX_FORMAT), K=np.asarray(result["K"], dtype=np.float64),
                 x_starts=np.asarray(result["x_starts"], dtype=np.int64), y_starts=np.asarray(result["y_starts"], dtype=np.int64),
                 x_valid=np.asarray(result["x_valid"], dtype=np.bool_), y_valid=np.asarray(result["y_valid"], dtype=np.bool_),
                 width=np.array(int(width), dtype=np.int64))


def read_window_kernel(path):
    """-> dict(K, x_starts, y_starts, x_valid, y_valid, width) from a file written by write_window_kernel."""
    with np.load(path, allow_pickle=False) as z:
        if sorted(z.files) != sorted(_MATRIX_KEYS) or str(z["format"]) != MATRIX_FORMAT:
            raise WindowError("%s is not a %s file" % (path, MATRIX_FORMAT))
        out = {key: z[key] for key in _MATRIX_KEYS[1:-1]}
        out["width"] = int(z["width"])
    if out["K"].shape != (len(out["x_starts"]), len(out["y_starts"])) or len(out["x_valid"]) != len(out["x_starts"]) \
            or len(out["y_valid"]) != len(out["y_starts"]):
        raise WindowError("%s: the arrays' shapes do not fit each other" % path)
    return out


def write_window_best(path, result):
    """The `best` output: one line per window of x, x_start<TAB>y_start<TAB>K (0-based starts; K at %.17g, which reads back
    to the same double); -1 and nan where no window of y was eligible."""
    with open(path, "w") as f:
        f.write("".join("%d\t%d\t%.17g\n" % row for row in
                        zip(result["x_starts"].tolist(), result["y_start"].tolist(), result["K"].tolist())))


def read_window_best(path):
    """-> dict(x_starts, y_start, K) from a file written by write_window_best."""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f.read().split("\n")[:-1], 1):
            fields = line.split("\t")
            if len(fields) != 3:
                raise WindowError("%s:%d: expected x_start, y_start and K" % (path, no))
            try:
                rows.append((int(fields[0]), int(fields[1]), float(fields[2])))
            except ValueError:
                raise WindowError("%s:%d: expected two integers and a number" % (path, no))
    return dict(x_starts=np.array([r[0] for r in rows], dtype=np.int64), y_start=np.array([r[1] for r in rows], dtype=np.int64),
                K=np.array([r[2] for r in rows], dtype=np.float64))


# ------------------------------------------------------------------ command line
def build_parser():
    p = argparse.ArgumentParser(prog="gkmwindows", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, text in (("matrix", "the kernel between every window of x and every window of y -> .npz"),
                       ("best", "per window of x the best window of y -> TSV"),
                       ("align", "the best local path through the matrix: the chain of matching window pairs -> TSV")):
        q = sub.add_parser(name, help=text)
        q.add_argument("--width", type=int, required=True, help="bases per window (L..%d)" % MAX_WIDTH)
        q.add_argument("--stride-x", type=int, default=1, help="bases between window starts of x (default 1)")
        q.add_argument("--stride-y", type=int, default=None, help="the same for y (default: --stride-x)")
        if name == "best":
            q.add_argument("--min-separation", type=int, default=0,
                           help="least distance in bases between the two windows' starts (default 0: any)")
        if name == "align":
            q.add_argument("--offset", type=float, required=True, help="the K a window pair must exceed to gain")
            q.add_argument("--gap", type=float, required=True, help="the cost of a window skipped on either axis (>= 0)")
            q.add_argument("--orientation", default="forward", help="forward, reverse or both (default forward)")
        q.add_argument("--chunk", type=int, default=None, help="bases per device chunk on either axis")
        q.add_argument("-t", "--kernel-type", type=int, default=0, help="0 gapped k-mer, 1 estimated l-mer with full "
                       "filter, 2 truncated filter, 3 gkm with RBF (default 0)")
        q.add_argument("-L", "--full-word-length", type=int, default=11)
        q.add_argument("-k", "--non-gap-length", type=int, default=7)
        q.add_argument("-d", "--max-num-gaps", type=int, default=3)
        q.add_argument("-G", "--rbf-gamma", type=float, default=1.0)
        q.add_argument("--device", type=int, default=0)
        q.add_argument("x_fa")
        q.add_argument("y_fa")
        q.add_argument("output")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        args = (a.x_fa, a.y_fa, a.width, a.stride_x, a.stride_y, a.kernel_type, a.full_word_length, a.non_gap_length,
                a.max_num_gaps, a.rbf_gamma, a.device, a.chunk)
        tmp = a.output + ".tmp"
        if a.cmd == "matrix":
            r = window_kernel(*args)
            write_window_kernel(tmp, r, a.width)
            os.replace(tmp, a.output)
            print("%d x %d windows, %d and %d over a non-ACGT character (nan) -> %s"
                  % (len(r["x_starts"]), len(r["y_starts"]), int((~r["x_valid"]).sum()), int((~r["y_valid"]).sum()), a.output),
                  file=sys.stderr)
        elif a.cmd == "align":
            r = window_align(*args[:-2], offset=a.offset, gap=a.gap, orientation=a.orientation, device=a.device, chunk=a.chunk)
            write_window_align(tmp, r)
            os.replace(tmp, a.output)
            print("score %.6g, %s, %d matched window pairs -> %s" % (r["score"], r["orientation"], len(r["x_start"]), a.output),
                  file=sys.stderr)
        else:
            r = window_best(*args, min_separation=a.min_separation)
            write_window_best(tmp, r)
            os.replace(tmp, a.output)
            print("%d windows of x, %d without an eligible window of y -> %s"
                  % (len(r["x_starts"]), int((r["y_start"] < 0).sum()), a.output), file=sys.stderr)
    except (WindowError, gp.ModelError, dv.GkmError, OSError) as e:
        print("gkmwindows: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
