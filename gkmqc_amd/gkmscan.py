"""Scanning sequences of any length with a weight table or a panel: every window's score, the regions
above a threshold (§5o) and the distribution of the scores (§5p).  Each panel form stands right after the single-table
form whose result it repeats per member, bit for bit."""
import math
import os
import time

import numpy as np

from . import device as dv
from .gkmmodel import _ACGT, ModelError
from .gkmquery import BLOCK_BYTES, _norms_from_profiles
from .gkmtables import LmerPanel, LmerTable, _check_folded, _models, _panel_row, _per_item, _rho_operand


# ------------------------------------------------------------------ scanning long sequences
SCAN_MAX_WIDTH = 2047     # a window is a query of its own: the longest sequence the kernels' norms are defined for
_WHITESPACE = np.array([9, 10, 11, 12, 13, 32], dtype=np.uint8)


def read_long_fasta(path):
    """A FASTA file -> [(name, codes, valid)] with records of any length, uncut: name is the header after '>', codes
    the uint8 base codes (A, C, G, T = 0..3 in either case; 0 at any other character) and valid the bool mask of the
    bases that are A, C, G or T.  Lines before the first header are ignored, as is white space inside a record."""
    with open(path, "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[_ACGT] = np.arange(4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    nls = np.flatnonzero(data == 10)
    starts = np.concatenate(([0], nls + 1))                                # where lines begin
    starts = starts[starts < len(data)]
    heads = starts[data[starts] == ord(">")]
    ends = np.append(nls, len(data))[np.searchsorted(nls, heads)]          # where the header lines end
    out = []
    for i, (h, end) in enumerate(zip(heads.tolist(), ends.tolist())):
        name = data[h + 1:end].tobytes().decode("utf-8", "replace").rstrip("\r")
        body = data[end + 1:heads[i + 1] if i + 1 < len(heads) else len(data)]
        body = body[~np.isin(body, _WHITESPACE)]
        codes = lut[body]
        valid = codes != 255
        codes[~valid] = 0
        out.append((name, codes, valid))
    return out


def _as_scan_records(fasta_or_sequences):
    if isinstance(fasta_or_sequences, (str, bytes, os.PathLike)):
        return read_long_fasta(fasta_or_sequences)
    out = []
    for i, x in enumerate(fasta_or_sequences):
        x = np.asarray(x, dtype=np.uint8)
        valid = x < 4
        out.append(("seq%d" % i, np.where(valid, x, 0).astype(np.uint8), valid))
    return out


def scan_window_count(T, width, stride):
    """Windows of `width` bases at starts 0, stride, 2 stride, ... that lie inside T bases."""
    return 0 if T < width else (int(T) - int(width)) // int(stride) + 1


def window_validity(valid, width, stride):
    """-> bool per window: the window covers no invalid base."""
    bad = np.zeros(len(valid) + 1, dtype=np.int64)
    np.cumsum(~np.asarray(valid, dtype=bool), out=bad[1:])
    a = np.arange(scan_window_count(len(valid), width, stride), dtype=np.int64) * int(stride)
    return bad[a + int(width)] == bad[a]


def scan_chunk_plan(T, width, stride, chunk):
    """The chunks of a record of T bases -> [(w0, w1, b0, b1)]: windows [w0, w1) from the bases [b0, b1), at most
    max(chunk, width) of them; every window in exactly one chunk.  Consecutive chunks share the bases between the next
    window's start and the last window's end (width - 1 of them at stride 1)."""
    nw = scan_window_count(T, width, stride)
    per = (max(int(chunk), int(width)) - int(width)) // int(stride) + 1
    return [(w0, min(nw, w0 + per), w0 * stride, (min(nw, w0 + per) - 1) * stride + width) for w0 in range(0, nw, per)]


def default_scan_chunk(d, budget=BLOCK_BYTES):
    """Bases per chunk: at stride 1 a base costs its code, mask and l-mer word, a window's d + 1 int64 profile counts and
    the doubles of the epilogue, within `budget` bytes of device memory."""
    return int(budget // (8 * (int(d) + 1) + 64))


def default_panel_scan_chunk(d, n_models, budget=BLOCK_BYTES):
    """Bases per chunk of scan_with_panel: default_scan_chunk's bytes per base and the window's n_models doubles."""
    return int(budget // (8 * (int(d) + 1) + 64 + 8 * int(n_models)))


def check_scan(table, width, stride, chunk=None):
    """What `scan` refuses before it reads anything or touches the device."""
    _check_scan(LmerTable, "scan", table, width, stride, chunk)


def check_panel_scan(panel, width, stride, chunk=None):
    """What `scan_with_panel` refuses before it reads anything or touches the device (check_scan's refusals)."""
    _check_scan(LmerPanel, "scan-panel", panel, width, stride, chunk)


def _check_scan(want, what, folded, width, stride, chunk):
    """check_scan's and check_panel_scan's refusals; what: the prefix of every message"""
    _check_folded(want, what, folded)
    if int(width) < folded.L:
        raise ModelError("%s: the width %d is below L = %d" % (what, width, folded.L))
    if int(width) > SCAN_MAX_WIDTH:
        raise ModelError("%s: the width %d is above %d, the longest sequence a score is defined for"
                         % (what, width, SCAN_MAX_WIDTH))
    if int(stride) < 1:
        raise ModelError("%s: the stride must be at least 1" % what)
    if chunk is not None and int(chunk) < int(width):
        raise ModelError("%s: a chunk must hold at least one window (%d bases)" % (what, width))


def scan(table, fasta_or_sequences, width, stride=1, device=0, chunk=None, on_chunk=None):
    """The score of every window of `width` bases at starts 0, stride, 2 stride, ... of each record of a FASTA file (or of
    each of a list of uint8 code arrays, values >= 4 invalid), records of any length -> [(name, starts, scores)], starts
    int64 and scores float64 per record.  A window's score is score_with_table's for the window cut out as a sequence,
    bit for bit, whatever `chunk` and whatever precedes the record; NaN where the window covers a character other than
    A, C, G, T (either case).  A record shorter than `width` has no windows; it is an error if none has any.
    chunk: bases per device chunk (default_scan_chunk).  on_chunk(dict) (measurements): called after every chunk with
    its windows, k_scan_profiles' milliseconds (HIP events), its l-mer comparisons and the chunk's wall time."""
    check_scan(table, width, stride, chunk)
    return _scan_folded(table, "scan", fasta_or_sequences, width, stride, device, chunk or default_scan_chunk(table.d),
                        on_chunk)


def scan_with_panel(panel, fasta_or_sequences, width, stride=1, device=0, chunk=None, on_chunk=None):
    """`scan` for every member of a panel -> [(name, starts, scores (windows, n_models))]: column m is scan's result for
    member m, bit for bit, whatever `chunk` and whatever precedes the record; a window over a character other than A, C,
    G, T is NaN in every column.  Per chunk the l-mer words and the windows' self profiles once (k_scan_profiles, the
    hot kernel of a scan, depends on the shared parameters only), then one k_panel_scan_score launch.
    chunk: bases per device chunk (default_panel_scan_chunk).  on_chunk(dict) (measurements): scan's keys, `models`,
    `score_kernel` and `score_kernel_ms`."""
    check_panel_scan(panel, width, stride, chunk)
    return _scan_folded(panel, "scan-panel", fasta_or_sequences, width, stride, device,
                        chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)


def _scan_folded(folded, what, fasta_or_sequences, width, stride, device, chunk, on_chunk):
    """The body `scan` and `scan_with_panel` share -> [(name, starts, scores (windows,) + folded.cols)].  folded: the
    table or panel (checked with width, stride and chunk); what: the prefix of the messages; chunk: bases per chunk."""
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    out = []
    for name, codes, valid in records:
        nw = scan_window_count(len(codes), width, stride)
        out.append((name, np.arange(nw, dtype=np.int64) * stride, np.empty((nw,) + folded.cols)))
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None):
        out[ch.record][2][ch.w0:ch.w1] = ch.scores.cpu().numpy()
        if on_chunk is not None:
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    for (_, _, valid), (_, _, scores) in zip(records, out):
        scores[~window_validity(valid, width, stride)] = np.nan
    return out


def _scan_records(what, fasta_or_sequences, width):
    """The records of a scan, or the refusal every scan shares: none of them holds a window."""
    records = _as_scan_records(fasta_or_sequences)
    if not any(len(codes) >= width for _, codes, _ in records):
        raise ModelError("%s: no record holds a window of %d bases" % (what, width))
    return records


class _ScanChunk:
    """What the chunk loop hands over per chunk, all of it on the device: the windows [w0, w1) of records[record], the
    chunk's nlm l-mer words (int32 tensor lm) and the windows' finished scores ((windows,) + folded.cols, rho included;
    whatever stands at a window over an invalid base is not a score).  ctx, stream: for further launches on the chunk;
    info: the measurements so far (None unless asked for); t0: when the chunk began."""
    __slots__ = ("record", "w0", "w1", "lm", "nlm", "scores", "ctx", "stream", "info", "t0")


def _scan_chunks(folded, records, width, stride, device, chunk, measure, score_ms=False):
    """The chunk loop of every scan, a generator of _ScanChunk: per chunk of each record the upload, the l-mer words, the
    windows' self profiles (k_scan_profiles), the table's or panel's score launch and the epilogue T / sq + rho.  The
    consumer runs between two chunks, on the loop's device and stream.  measure: fill info with scan's on_chunk keys;
    score_ms: a table reports its score kernel too."""
    import torch
    chunk = int(chunk)
    L, d, cols = folded.L, folded.d, folded.cols
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    c = dv.mismatch_weights(folded.kernel_type, L, folded.k)[:d + 1]
    wt = dv.position_weights(folded.kernel_type, width - L + 1, folded.M, folded.H)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        W = torch.from_numpy(folded.device_weights()).to(dev)
        rho = _rho_operand(folded, dev)
        d_wt = torch.from_numpy(wt).to(dev)
        launch = folded.launcher(ctx, "scan_score")
        for r, (name, codes, valid) in enumerate(records):
            for w0, w1, b0, b1 in scan_chunk_plan(len(codes), width, stride, chunk):
                ch = _ScanChunk()
                ch.record, ch.w0, ch.w1, ch.ctx, ch.stream, ch.info = r, w0, w1, ctx, stream, None
                ch.t0 = time.perf_counter()
                d_codes = torch.from_numpy(codes[b0:b1]).to(dev)
                d_valid = torch.from_numpy(valid[b0:b1].view(np.uint8)).to(dev)
                nlm, nwin = b1 - b0 - L + 1, w1 - w0
                lm = torch.empty(nlm, dtype=torch.int32, device=dev)
                ctx.scan_lmers(d_codes.data_ptr(), d_valid.data_ptr(), b1 - b0, lm.data_ptr(), stream)
                prof = torch.empty((nwin, d + 1), dtype=torch.int64, device=dev)
                ctx.scan_profiles(lm.data_ptr(), nlm, d_wt.data_ptr(), width, stride, nwin, prof.data_ptr(), stream)
                if measure:
                    ch.info = dict(windows=nwin, bases=b1 - b0, **_models(cols), profile_kernel_ms=ctx.last_kernel_ms(),
                                   comparisons=ctx.last_comparisons(), kernel=ctx.last_kernel_name())
                T = torch.empty((nwin,) + cols, dtype=torch.float64, device=dev)
                launch(lm.data_ptr(), nlm, d_wt.data_ptr(), width, stride, nwin, W.data_ptr(), T.data_ptr(), stream)
                if measure and (cols or score_ms):                         # (a panel reports its score kernel too)
                    ch.info.update(score_kernel=ctx.last_kernel_name(), score_kernel_ms=ctx.last_kernel_ms())
                sq = _norms_from_profiles(prof, c)
                ch.lm, ch.nlm, ch.scores = lm, nlm, T / _per_item(sq, cols) + rho
                yield ch


def write_scan(path, results, width):
    """The `scan` output: one line per scored window, name<TAB>start<TAB>end<TAB>score (0-based start, end = start +
    width, the score at %.17g, which reads back to the same double); windows without a score (NaN) are left out.
    -> how many were left out."""
    omitted = 0
    with open(path, "w") as f:
        for name, starts, scores in results:
            keep = ~np.isnan(scores)
            omitted += int((~keep).sum())
            for i in range(0, len(starts), 1 << 16):
                k = keep[i:i + (1 << 16)]
                f.write("".join("%s\t%d\t%d\t%.17g\n" % (name, a, a + width, v) for a, v in
                                zip(starts[i:i + (1 << 16)][k].tolist(), scores[i:i + (1 << 16)][k].tolist())))
    return omitted


def read_scan(path):
    """-> [(name, start, end, score)] from a file written by write_scan."""
    out = []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, a, b, v = line.rsplit("\t", 3)
            out.append((name, int(a), int(b), float(v)))
    return out


def write_panel_scan(path, panel_names, results, width):
    """The `scan-panel` output: the header #name<TAB>start<TAB>end<TAB>member names, then `scan`'s leading columns and
    one score per member at %.17g; windows without a score (NaN) are left out.  -> how many were left out."""
    omitted = 0
    with open(path, "w") as f:
        f.write("#" + "\t".join(["name", "start", "end"] + list(panel_names)) + "\n")
        for name, starts, scores in results:
            keep = ~np.isnan(scores).any(axis=1)
            omitted += int((~keep).sum())
            for i in range(0, len(starts), 1 << 14):
                k = keep[i:i + (1 << 14)]
                f.write("".join(_panel_row([name, "%d" % a, "%d" % (a + width)], row) for a, row in
                                zip(starts[i:i + (1 << 14)][k].tolist(), scores[i:i + (1 << 14)][k].tolist())))
    return omitted


# ------------------------------------------------------------------ regions of a scan
REGION_FIELDS = ("start", "end", "peak", "summit", "windows")   # the arrays of a `regions` dict, in file order
_REGION_KEYS = ("first", "last", "summit", "windows", "peak")   # of a region in window indices, as the device reports it
REGION_MAX_GAP = 1 << 40  # the largest gap the device layer takes (gkmhip_regions_count)


def _check_regions(what, threshold, gap, n_models=None):
    """The refusals `scan_regions` adds to `scan`'s -> the thresholds, one float per member (one in all for a table)."""
    if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)):
        raise ModelError("%s: the gap must be an integer, not %r" % (what, gap))
    if gap < 0:
        raise ModelError("%s: the gap must be at least 0" % what)
    if gap > REGION_MAX_GAP:
        raise ModelError("%s: the gap must be at most 2^40 windows" % what)
    if n_models is None or np.ndim(threshold) == 0:
        values = [threshold] * (n_models or 1)
    else:
        values = list(threshold)
        if len(values) != n_models:
            raise ModelError("%s: %d thresholds for the panel's %d members" % (what, len(values), n_models))
    try:
        values = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ModelError("%s: the threshold must be a number%s" % (what, "" if n_models is None else " or one per member"))
    if any(v != v for v in values):
        raise ModelError("%s: the threshold is NaN" % what)
    return values


def check_scan_regions(table, width, stride, threshold=0.0, gap=0, chunk=None):
    """What `scan_regions` refuses before it reads anything or touches the device: check_scan's refusals, a gap that is
    negative, above 2^40 or no integer, a NaN threshold.  -> the threshold as a float."""
    _check_scan(LmerTable, "scan-regions", table, width, stride, chunk)
    return _check_regions("scan-regions", threshold, gap)[0]


def check_panel_scan_regions(panel, width, stride, threshold=0.0, gap=0, chunk=None):
    """check_scan_regions for `scan_regions_with_panel`: check_panel_scan's refusals, the gap, and the thresholds -- one
    for all members or one per member, none of them NaN.  -> the thresholds, one float per member."""
    _check_scan(LmerPanel, "scan-regions-panel", panel, width, stride, chunk)
    return _check_regions("scan-regions-panel", threshold, gap, panel.n_models)


def _no_regions():
    return dict(first=np.empty(0, np.int64), last=np.empty(0, np.int64), summit=np.empty(0, np.int64),
                windows=np.empty(0, np.int64), peak=np.empty(0, np.float64))


def stitch_regions(per_chunk, gap):
    """The regions of a record's chunks, each found as if its chunk stood alone -> the record's.  per_chunk: one dict per
    chunk, in order, of the arrays first, last, summit, windows (integers) and peak (float64) in the RECORD's window
    indices, ascending.  A region merges with the one before it when its first window lies within gap + 1 of that one's
    last (inside a chunk none does; across chunk boundaries a merge may cascade): the merged region runs from the first
    one's `first` to the last one's `last`, its windows add up, and its peak and summit are those of the part with the
    largest peak, the earliest such part on a tie.  Only the order of the regions enters, not how they are divided among
    the dicts.  -> a dict of the same five arrays (int64, float64)."""
    parts = [c for c in per_chunk if len(c["first"])]
    if not parts:
        return _no_regions()
    first, last, summit, windows = (np.concatenate([np.asarray(c[key], dtype=np.int64) for c in parts])
                                    for key in _REGION_KEYS[:4])
    peak = np.concatenate([np.asarray(c["peak"], dtype=np.float64) for c in parts])
    begins = np.ones(len(first), dtype=bool)
    begins[1:] = first[1:] - last[:-1] > int(gap) + 1
    at = np.flatnonzero(begins)
    group = np.cumsum(begins) - 1
    top = np.flatnonzero(peak == np.maximum.reduceat(peak, at)[group])     # the parts that attain their region's peak
    top = top[np.concatenate(([True], group[top][1:] != group[top][:-1]))]  # the earliest of each region
    return dict(first=first[at], last=last[np.append(at[1:], len(first)) - 1], summit=summit[top],
                windows=np.add.reduceat(windows, at), peak=peak[top])


def _regions_in_bases(r, width, stride):
    """a region dict in window indices -> the `regions` dict of scan_regions, in bases"""
    return dict(start=r["first"] * stride, end=r["last"] * stride + width, peak=r["peak"], summit=r["summit"] * stride,
                windows=r["windows"])


def _chunk_regions(ch, col, ld, width, stride, threshold, gap, scratch):
    """The regions of column `col` of a chunk's scores, in the record's window indices -> (dict, bytes copied back,
    the region kernels' milliseconds).  Only the count and the regions themselves leave the device."""
    import torch
    ctx, nwin = ch.ctx, ch.w1 - ch.w0
    args = (ch.scores.data_ptr() + 8 * col, ld, ch.lm.data_ptr(), ch.nlm, width, stride, nwin, threshold, gap,
            scratch.data_ptr(), scratch.numel())
    n = ctx.regions_count(*args, ch.stream)
    ms = ctx.last_kernel_ms() if ch.info is not None else 0.0
    if n == 0:
        return _no_regions(), 8, ms
    ints = torch.empty((4, n), dtype=torch.int32, device=scratch.device)
    peak = torch.empty(n, dtype=torch.float64, device=scratch.device)
    ctx.regions_fill(*args, n, *(ints[k].data_ptr() for k in range(4)), peak.data_ptr(), ch.stream)
    if ch.info is not None:
        ms += ctx.last_kernel_ms()
    h = ints.cpu().numpy().astype(np.int64)
    out = dict(first=h[0] + ch.w0, last=h[1] + ch.w0, summit=h[2] + ch.w0, windows=h[3], peak=peak.cpu().numpy())
    return out, 8 + 64 + 24 * n, ms                                        # the count; fill's header; 4 int32 + 1 double


def _scan_regions_folded(folded, what, fasta_or_sequences, width, stride, thresholds, gap, device, chunk, on_chunk):
    """The body `scan_regions` and `scan_regions_with_panel` share -> [(name, [regions per member])]: the chunk loop of
    `scan`, then per chunk and member one count and one fill call on the member's column of the device scores."""
    import torch
    width, stride, gap = int(width), int(stride), int(gap)
    records = _scan_records(what, fasta_or_sequences, width)
    nm = len(thresholds)
    found = [[[] for _ in range(nm)] for _ in records]
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None, score_ms=True):
        scratch = torch.empty(ch.ctx.regions_scratch_bytes(ch.nlm, ch.w1 - ch.w0), dtype=torch.uint8,
                              device=ch.scores.device)
        got = [_chunk_regions(ch, m, nm, width, stride, thresholds[m], gap, scratch) for m in range(nm)]
        for m, (r, _, _) in enumerate(got):
            found[ch.record][m].append(r)
        if on_chunk is not None:
            counts = [len(r["first"]) for r, _, _ in got]
            ch.info.update(regions=counts if folded.cols else counts[0], copied_bytes=sum(b for _, b, _ in got),
                           region_kernels_ms=sum(ms for _, _, ms in got))
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    return [(name, [_regions_in_bases(stitch_regions(per_chunk, gap), width, stride) for per_chunk in members])
            for (name, _, _), members in zip(records, found)]


def scan_regions(table, fasta_or_sequences, width, stride=1, threshold=0.0, gap=0, device=0, chunk=None, on_chunk=None):
    """The regions of a scan -> [(name, regions)] per record, in file order.  A window passes when it has a score (it
    covers only A, C, G, T) and the score `scan` returns for it, rho included, is >= threshold (a NaN never passes;
    -inf passes every scored window).  Consecutive passing windows belong to one region when at most `gap` windows lie
    between them.  regions: a dict of arrays, one element per region in ascending order: start (the first passing
    window's start), end (the last one's start + width), summit (the start of the first passing window that attains the
    peak) and windows (how many passed), int64, and peak (the largest score among them), float64.  A record shorter than
    `width` or without a passing window has empty arrays.  Whatever `chunk` and whatever precedes the record, the result
    is bit for bit this definition applied to `scan`'s output.
    The reduction runs on the device (k_regions_summaries, k_regions_fill): per chunk only the region count and the
    regions are copied back, and no per-window array exists on the host.  on_chunk(dict) (measurements): scan's keys,
    `score_kernel` and `score_kernel_ms`, `regions`, `copied_bytes` (what the chunk brought back from the device) and
    `region_kernels_ms` (HIP events)."""
    threshold = check_scan_regions(table, width, stride, threshold, gap, chunk)
    res = _scan_regions_folded(table, "scan-regions", fasta_or_sequences, width, stride, [threshold], gap, device,
                               chunk or default_scan_chunk(table.d), on_chunk)
    return [(name, members[0]) for name, members in res]


def scan_regions_with_panel(panel, fasta_or_sequences, width, stride=1, threshold=0.0, gap=0, device=0, chunk=None,
                            on_chunk=None):
    """`scan_regions` for every member of a panel -> [(name, [regions of member 0, of member 1, ...])]: member m's regions
    are scan_regions' for panel.table(m), bit for bit.  threshold: one for all members or one per member.  Per chunk the
    profiles and k_panel_scan_score run once; the region calls run once per member on its column of the device result
    (leading dimension n_models, no copy).  on_chunk(dict): scan_with_panel's keys, `regions` (one count per member),
    `copied_bytes` and `region_kernels_ms` (both summed over the members)."""
    thresholds = check_panel_scan_regions(panel, width, stride, threshold, gap, chunk)
    return _scan_regions_folded(panel, "scan-regions-panel", fasta_or_sequences, width, stride, thresholds, gap, device,
                                chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)


def write_regions(path, results):
    """The `scan-regions` output: one line per region, name<TAB>start<TAB>end<TAB>peak<TAB>summit<TAB>windows (0-based
    start, end exclusive, the peak at %.17g, which reads back to the same double); a record without regions writes
    nothing.  -> the regions written."""
    n = 0
    with open(path, "w") as f:
        for name, r in results:
            f.write("".join("%s\t%d\t%d\t%.17g\t%d\t%d\n" % ((name,) + row)
                            for row in zip(*(r[key].tolist() for key in REGION_FIELDS))))
            n += len(r["start"])
    return n


def read_regions(path):
    """-> [(name, start, end, peak, summit, windows)] from a file written by write_regions."""
    out = []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, a, b, v, s, n = line.rsplit("\t", 5)
            out.append((name, int(a), int(b), float(v), int(s), int(n)))
    return out


def write_panel_regions(path, panel_names, results):
    """The `scan-regions-panel` output: write_regions' line with the member's name in front,
    member<TAB>name<TAB>start<TAB>end<TAB>peak<TAB>summit<TAB>windows; records in file order, the members of a record in
    panel order.  -> the regions written."""
    n = 0
    with open(path, "w") as f:
        for name, members in results:
            for member, r in zip(panel_names, members):
                f.write("".join("%s\t%s\t%d\t%d\t%.17g\t%d\t%d\n" % ((member, name) + row)
                                for row in zip(*(r[key].tolist() for key in REGION_FIELDS))))
                n += len(r["start"])
    return n


def read_panel_regions(path):
    """-> [(member, name, start, end, peak, summit, windows)] from a file written by write_panel_regions."""
    out = []
    for lead, a, b, v, s, n in read_regions(path):
        out.append(tuple(lead.split("\t", 1)) + (a, b, v, s, n))
    return out


# ------------------------------------------------------------------ score distributions of a scan
DIST_MAX_THRESHOLDS = 4096  # edges one gkmhip_dist_edges launch takes
DIST_MAX_RANKS = 64         # prefixes one gkmhip_dist_digits launch carries: one target per requested rank at most
DIST_DIGIT_BITS = 13        # gkmhip_dist_digit_bits of this build (the device's own value is what a scan uses)
_KEY_SIGN, _KEY_ALL = np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)


def score_keys(values):
    """float64 -> uint64 keys: b ^ (b >> 63 ? ~0 : 1 << 63) of the bits b.  Ascending keys are ascending non-NaN
    doubles, -0.0 just below +0.0; the map is a bijection of the 64-bit words."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), _KEY_ALL, _KEY_SIGN)


def keys_to_scores(keys):
    """The inverse of score_keys: the same bits back."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63), _KEY_SIGN, _KEY_ALL)).view(np.float64)


def dist_level_bits(digit_bits=DIST_DIGIT_BITS):
    """The key bits each refinement level resolves for B = digit_bits: ceil(64 / B) levels, the first of
    64 - B (levels - 1) bits, every later one of B."""
    B = int(digit_bits)
    if not 1 <= B <= 64:
        raise ModelError("a level resolves 1..64 bits, not %d" % B)
    levels = -(-64 // B)
    return [64 - B * (levels - 1)] + [B] * (levels - 1)


def dist_boundaries(digit_bits=DIST_DIGIT_BITS):
    """The bits resolved after each level; the last is 64."""
    return np.cumsum(dist_level_bits(digit_bits)).tolist()


def quantile_ranks(n, q):
    """The order statistic a quantile q in [0, 1] of n values names: min(n - 1, floor(q (n - 1))) in Python floats."""
    return [min(int(n) - 1, int(math.floor(float(x) * (int(n) - 1)))) for x in q]


class _RankSearch:
    """Radix selection of order statistics from histograms of a multiset of keys that is never held: a state machine.
    `request` is what it needs next -- ("hist", prefixes, prefix_bits) or ("collect", prefixes, prefix_bits, total), or
    None when `values` holds the answer -- and feed(result) hands it over: for "hist" the counts (len(prefixes) or 1,
    2^bits of the level) of the keys that begin with each prefix by their next digit, for "collect" the `total` values
    whose keys begin with one of the prefixes, in any order.  want(n) -> the ranks, once the first histogram has given
    n.  All targets (the distinct prefixes the ranks fall under, each with the count of keys below it) descend one level
    per pass in lockstep; they are collected as soon as they hold at most collect_cap keys together, and decoded when
    all 64 bits are resolved, which ends the search whatever the values are."""

    def __init__(self, want, collect_cap, digit_bits):
        self.want, self.cap, self.bits = want, int(collect_cap), dist_level_bits(digit_bits)
        self.level, self.prefix_bits = 0, 0
        self.prefixes = np.empty(0, dtype=np.uint64)
        self.request = ("hist", self.prefixes, 0)
        self.n = self.ranks = self.values = None

    def feed(self, result):
        if self.request[0] == "collect":
            self.values, self.request = self._read_off(result), None
            return
        bits = self.bits[self.level]
        counts = np.asarray(result, dtype=np.int64).reshape(max(len(self.prefixes), 1), 1 << bits)
        if self.level == 0:
            self.n = int(counts.sum())
            self.ranks = np.asarray(self.want(self.n), dtype=np.int64).reshape(-1)
            self.target = np.zeros(len(self.ranks), dtype=np.int64)       # the row of each rank's target
            self.below = np.zeros(1, dtype=np.int64)                      # per target: the keys below it
            self.prefixes = np.zeros(1, dtype=np.uint64)
        cum = np.cumsum(counts, axis=1)
        local = self.ranks - self.below[self.target]
        digit = np.array([np.searchsorted(cum[t], r, side="right") for t, r in zip(self.target, local)], dtype=np.int64)
        if (digit >> bits).any():
            raise ModelError("the histogram of a refinement pass does not hold the windows of the pass before it")
        count = counts[self.target, digit]
        below = self.below[self.target] + cum[self.target, digit] - count
        prefix = (self.prefixes[self.target] << np.uint64(bits)) | digit.astype(np.uint64)
        self.level, self.prefix_bits = self.level + 1, self.prefix_bits + bits
        self.prefixes, first, self.target = np.unique(prefix, return_index=True, return_inverse=True)
        self.target = self.target.reshape(-1)
        self.below, self.count = below[first], count[first]
        if self.prefix_bits == 64:                                         # the prefix is the key
            self.values, self.request = keys_to_scores(self.prefixes)[self.target], None
        elif int(self.count.sum()) <= self.cap:
            self.request = ("collect", self.prefixes, self.prefix_bits, int(self.count.sum()))
        else:
            self.request = ("hist", self.prefixes, self.prefix_bits)

    def _read_off(self, values):
        keys = np.sort(score_keys(np.asarray(values, dtype=np.float64).reshape(-1)))
        run = np.repeat(self.prefixes, self.count)
        if len(keys) != len(run) or not np.array_equal(keys >> np.uint64(64 - self.prefix_bits), run):
            raise ModelError("the collected values are not the ones the histograms counted")
        start = np.cumsum(self.count) - self.count
        return keys_to_scores(keys[start[self.target] + self.ranks - self.below[self.target]])


def select_order_statistics(hist_pass, collect_pass, want, collect_cap=1 << 20, digit_bits=DIST_DIGIT_BITS, on_pass=None):
    """Order statistics of a multiset of doubles that only two callables can see -> (n, ranks, values, passes).
    hist_pass(prefixes, prefix_bits) -> counts and collect_pass(prefixes, prefix_bits, total) -> values as _RankSearch
    describes them (prefix_bits 0 and no prefix: the first level over everything); want(n) -> the ranks in 0..n-1.
    values[i] is the ranks[i]-th smallest by key, the very bits.  passes: one dict per call made, in order -- kind
    ("hist" or "collect"), prefix_bits and targets -- at most levels + 1 of them; on_pass(dict) sees each after its
    call."""
    search, passes = _RankSearch(want, collect_cap, digit_bits), []
    while search.request is not None:
        kind, prefixes, prefix_bits = search.request[:3]
        passes.append(dict(kind=kind, prefix_bits=prefix_bits, targets=len(prefixes)))
        search.feed(hist_pass(prefixes, prefix_bits) if kind == "hist" else collect_pass(*search.request[1:]))
        if on_pass is not None:
            on_pass(passes[-1])
    return search.n, search.ranks, search.values, passes


def _check_quantiles(what, q, ranks, collect_cap):
    """The refusals `scan_quantiles` adds to `scan`'s -> (q as floats or None, want): want(n) -> the ranks of a call with
    n scored windows, or the refusals that need n."""
    if (q is None) == (ranks is None):
        raise ModelError("%s: give either q or ranks" % what)
    if isinstance(collect_cap, bool) or not isinstance(collect_cap, (int, np.integer)) or collect_cap < 1:
        raise ModelError("%s: collect_cap must be an integer of at least 1" % what)
    given = np.atleast_1d(np.asarray(q if ranks is None else ranks)).reshape(-1).tolist()
    if not 1 <= len(given) <= DIST_MAX_RANKS:
        raise ModelError("%s: 1..%d %s per call, not %d" % (what, DIST_MAX_RANKS, "quantiles" if ranks is None else "ranks",
                                                           len(given)))
    if ranks is None:
        try:
            qs = [float(x) for x in given]
        except (TypeError, ValueError):
            raise ModelError("%s: a quantile must be a number" % what)
        if any(not 0.0 <= x <= 1.0 for x in qs):                           # (a NaN fails both comparisons)
            raise ModelError("%s: a quantile must lie in 0..1 (and be no NaN)" % what)
    else:
        qs = None
        if any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) for r in given):
            raise ModelError("%s: a rank must be an integer" % what)
        if any(r < 0 for r in given):
            raise ModelError("%s: a rank must lie in 0..n-1" % what)

    def want(n):
        if n == 0:
            raise ModelError("%s: no window has a score" % what)
        if qs is not None:
            return quantile_ranks(n, qs)
        if any(r >= n for r in given):
            raise ModelError("%s: a rank must lie in 0..n-1; %d windows have a score" % (what, n))
        return given
    return qs, want


def _check_thresholds(what, thresholds):
    """The refusals `scan_tail_counts` adds to `scan`'s -> the thresholds as a float64 array, in the caller's order."""
    try:
        values = np.atleast_1d(np.asarray(thresholds, dtype=np.float64)).reshape(-1)
    except (TypeError, ValueError):
        raise ModelError("%s: a threshold must be a number" % what)
    if not 1 <= len(values) <= DIST_MAX_THRESHOLDS:
        raise ModelError("%s: 1..%d thresholds per call, not %d" % (what, DIST_MAX_THRESHOLDS, len(values)))
    if np.isnan(values).any():
        raise ModelError("%s: a threshold is NaN" % what)
    return values


def check_scan_tail_counts(table, width, stride, thresholds=(), chunk=None):
    """What `scan_tail_counts` refuses before it reads anything or touches the device: check_scan's refusals, no
    threshold, more than 4096 of them, a NaN among them.  -> the thresholds, float64."""
    _check_scan(LmerTable, "scan-tail", table, width, stride, chunk)
    return _check_thresholds("scan-tail", thresholds)


def check_panel_scan_tail_counts(panel, width, stride, thresholds=(), chunk=None):
    """check_scan_tail_counts for `scan_tail_counts_with_panel` -> the thresholds, float64."""
    _check_scan(LmerPanel, "scan-tail-panel", panel, width, stride, chunk)
    return _check_thresholds("scan-tail-panel", thresholds)


def check_scan_quantiles(table, width, stride, q=None, ranks=None, chunk=None, collect_cap=1 << 20):
    """What `scan_quantiles` refuses before it reads anything or touches the device: check_scan's refusals, both or
    neither of q and ranks, none or more than 64 of them, a q that is NaN or outside 0..1, a rank that is negative or no
    integer, a collect_cap below 1.  (A rank of n or more is refused once the first pass has counted n.)
    -> (q as floats, or None where ranks were given; want: n -> the ranks of a call with n scored windows)."""
    _check_scan(LmerTable, "scan-quantiles", table, width, stride, chunk)
    return _check_quantiles("scan-quantiles", q, ranks, collect_cap)


def check_panel_scan_quantiles(panel, width, stride, q=None, ranks=None, chunk=None, collect_cap=1 << 20):
    """check_scan_quantiles for `scan_quantiles_with_panel`."""
    _check_scan(LmerPanel, "scan-quantiles-panel", panel, width, stride, chunk)
    return _check_quantiles("scan-quantiles-panel", q, ranks, collect_cap)


def _dist_windows(records, width, stride):
    return sum(scan_window_count(len(codes), width, stride) for _, codes, _ in records)


def _chunk_dist_args(ch, col, ld, width, stride):
    return (ch.scores.data_ptr() + 8 * col, ld, ch.lm.data_ptr(), ch.nlm, width, stride, ch.w1 - ch.w0)


def _scan_tail_folded(folded, what, fasta_or_sequences, width, stride, thresholds, device, chunk, on_chunk):
    """The body `scan_tail_counts` and `scan_tail_counts_with_panel` share -> (windows, scored (members,), counts
    (members, thresholds)): one scan, per chunk and member one k_dist_edges launch on the member's column; the
    histograms come back once, after the last chunk."""
    import torch
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    nm, order = folded.cols[0] if folded.cols else 1, np.argsort(thresholds, kind="stable")
    dev = torch.device("cuda", device)
    edges = torch.from_numpy(thresholds[order]).to(dev)
    hist = torch.zeros((nm, len(thresholds) + 1), dtype=torch.int64, device=dev)
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None, score_ms=True):
        nbytes = ch.ctx.dist_scratch_bytes(ch.nlm, ch.w1 - ch.w0)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = 0.0
        for m in range(nm):
            ch.ctx.dist_edges(*_chunk_dist_args(ch, m, nm, width, stride), edges.data_ptr(), len(thresholds),
                              hist[m].data_ptr(), scratch.data_ptr(), nbytes, ch.stream)
            if on_chunk is not None:
                ms += ch.ctx.last_kernel_ms()
        if on_chunk is not None:
            ch.info.update(dist_kernels_ms=ms, copied_bytes=0)
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    suffix = np.cumsum(hist.cpu().numpy()[:, ::-1], axis=1)[:, ::-1]       # [m, b]: scores with at least b edges <= them
    counts = np.empty((nm, len(thresholds)), dtype=np.int64)
    counts[:, order] = suffix[:, 1:]
    return _dist_windows(records, width, stride), suffix[:, 0].copy(), counts


def scan_tail_counts(table, fasta_or_sequences, width, stride=1, thresholds=(), device=0, chunk=None, on_chunk=None):
    """How many scored windows of a scan reach each threshold, all records pooled -> dict(scored, unscored, thresholds,
    counts).  A window is scored when it covers only A, C, G, T and `scan`'s score for it is no NaN; counts[i] (int64, the
    caller's order) is the number of scored windows with score >= thresholds[i], `scan_regions`' own pass rule: the sum
    of `windows` over scan_regions(threshold=thresholds[i], gap=0).  -inf counts every scored window, +inf only +inf
    scores.  One scan: the host sorts the thresholds, k_dist_edges bins every chunk's scores by them on the device, and
    only the histogram of len(thresholds) + 1 counters comes back, once.  on_chunk(dict) (measurements): scan's keys,
    `score_kernel`, `score_kernel_ms`, `dist_kernels_ms` (HIP events) and `copied_bytes` (0: nothing per chunk)."""
    thresholds = check_scan_tail_counts(table, width, stride, thresholds, chunk)
    windows, scored, counts = _scan_tail_folded(table, "scan-tail", fasta_or_sequences, width, stride, thresholds, device,
                                                chunk or default_scan_chunk(table.d), on_chunk)
    return dict(scored=int(scored[0]), unscored=windows - int(scored[0]), thresholds=thresholds, counts=counts[0])


def scan_tail_counts_with_panel(panel, fasta_or_sequences, width, stride=1, thresholds=(), device=0, chunk=None,
                                on_chunk=None):
    """`scan_tail_counts` for every member of a panel, the same thresholds for all -> dict(scored, unscored (int64, one
    per member), thresholds, counts (n_models, thresholds)): row m is scan_tail_counts' result for panel.table(m), bit
    for bit.  One scan serves all members: k_panel_scan_score once per chunk, then one k_dist_edges launch per member on
    its column of the device result.  on_chunk(dict): scan_with_panel's keys, `dist_kernels_ms` and `copied_bytes`."""
    thresholds = check_panel_scan_tail_counts(panel, width, stride, thresholds, chunk)
    windows, scored, counts = _scan_tail_folded(panel, "scan-tail-panel", fasta_or_sequences, width, stride, thresholds,
                                                device, chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)
    return dict(scored=scored, unscored=windows - scored, thresholds=thresholds, counts=counts)


def _scan_quantiles_folded(folded, what, fasta_or_sequences, width, stride, wants, collect_cap, device, chunk, on_pass):
    """The body `scan_quantiles` and `scan_quantiles_with_panel` share -> (windows, [the finished _RankSearch of each
    member], passes).  Every pass is one chunk loop of `scan` that serves all members still searching, each with its
    own request: per chunk and member one k_dist_digits or k_dist_collect launch on the member's column."""
    import torch
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    nm = len(wants)
    dev = torch.device("cuda", device)
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    searches = [_RankSearch(want, collect_cap, ctx.dist_digit_bits()) for want in wants]
    passes = []
    while any(s.request is not None for s in searches):
        active = [(m, s) for m, s in enumerate(searches) if s.request is not None]
        bufs = {}
        for m, s in active:
            if s.request[0] == "hist":
                bufs[m] = (torch.zeros(max(len(s.prefixes), 1) << s.bits[s.level], dtype=torch.int64, device=dev),)
            else:
                bufs[m] = (torch.empty(s.request[3], dtype=torch.float64, device=dev),
                           torch.zeros(1, dtype=torch.int64, device=dev))
        ms = scan_ms = 0.0
        for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_pass is not None, score_ms=True):
            nbytes = ctx.dist_scratch_bytes(ch.nlm, ch.w1 - ch.w0)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if on_pass is not None:
                scan_ms += ch.info["profile_kernel_ms"] + ch.info["score_kernel_ms"]
            for m, s in active:
                args = _chunk_dist_args(ch, m, nm, width, stride) + (s.request[1], s.request[2])
                if s.request[0] == "hist":
                    ctx.dist_digits(*args, bufs[m][0].data_ptr(), scratch.data_ptr(), nbytes, ch.stream)
                else:
                    ctx.dist_collect(*args, bufs[m][0].data_ptr(), s.request[3], bufs[m][1].data_ptr(), scratch.data_ptr(),
                                     nbytes, ch.stream)
                if on_pass is not None:
                    ms += ctx.last_kernel_ms()
        info = dict(kind=[s.request[0] for _, s in active], prefix_bits=[s.request[2] for _, s in active],
                    targets=[len(s.request[1]) for _, s in active], copied_bytes=0)
        if on_pass is not None:
            info.update(dist_kernels_ms=ms, scan_kernels_ms=scan_ms)
        for m, s in active:
            if s.request[0] == "collect":
                found = int(bufs[m][1].item())
                if found != s.request[3]:
                    raise dv.GkmError("%s: k_dist_collect found %d values where the histograms counted %d"
                                      % (what, found, s.request[3]))
                info["copied_bytes"] += 8
            info["copied_bytes"] += 8 * bufs[m][0].numel()
            s.feed(bufs[m][0].cpu().numpy())
        if not folded.cols:
            info.update(kind=info["kind"][0], prefix_bits=info["prefix_bits"][0], targets=info["targets"][0])
        passes.append(info)
        if on_pass is not None:
            on_pass(info)
    return _dist_windows(records, width, stride), searches, passes


def scan_quantiles(table, fasta_or_sequences, width, stride=1, q=None, ranks=None, device=0, chunk=None,
                   collect_cap=1 << 20, on_pass=None):
    """Exact order statistics of a scan's scores, all records pooled -> dict(scored, unscored, q, ranks, values, passes).
    Give either q (quantiles in 0..1) or ranks (0..n-1), at most 64, in any order, duplicates allowed.  With n the scored
    windows of the call (see scan_tail_counts), order statistic r is the r-th smallest score by key (score_keys:
    numerical order, -0.0 below +0.0) and a quantile q is order statistic min(n - 1, floor(q (n - 1))) -- not
    np.quantile, which interpolates.  values[i] is bit for bit that element of `scan`'s own output, whatever `chunk`,
    `collect_cap` and the order of the requests.  It is an error if no window has a score.
    The scores are never kept: radix selection over the keys re-scans instead.  Pass 0 counts every scored window by its
    key's first digit (k_dist_digits), which gives n and places each rank in a bin; the distinct bins are the targets,
    refined in lockstep one level per pass until they hold at most collect_cap windows together -- then one more pass
    gathers exactly those scores (k_dist_collect) and the host sorts them -- or until all 64 bits are resolved and the
    prefix is the value.  At most levels + 1 passes, each a full scan; only histograms and the collected values leave the
    device.  passes / on_pass(dict): per pass its kind ("hist" or "collect"), prefix_bits, targets, and what it brought
    back (copied_bytes); with on_pass also dist_kernels_ms and scan_kernels_ms (k_scan_profiles + k_scan_score), HIP
    events summed over the pass's chunks."""
    qs, want = check_scan_quantiles(table, width, stride, q, ranks, chunk, collect_cap)
    windows, (s,), passes = _scan_quantiles_folded(table, "scan-quantiles", fasta_or_sequences, width, stride, [want],
                                                   int(collect_cap), device, chunk or default_scan_chunk(table.d), on_pass)
    return dict(scored=s.n, unscored=windows - s.n, q=qs, ranks=s.ranks, values=s.values, passes=passes)


def scan_quantiles_with_panel(panel, fasta_or_sequences, width, stride=1, q=None, ranks=None, device=0, chunk=None,
                              collect_cap=1 << 20, on_pass=None):
    """`scan_quantiles` for every member of a panel, the same requests for all -> dict(scored, unscored (int64, one per
    member), q, ranks, values (both (n_models, requests)), passes): row m is scan_quantiles' result for panel.table(m), bit
    for bit.  One chunk loop per pass serves all members; each carries its own targets and collects when ITS targets fit
    collect_cap, so a pass may count for one member and collect for another.  passes / on_pass(dict): kind, prefix_bits
    and targets are lists, one entry per member still searching; the other keys are summed over them."""
    qs, want = check_panel_scan_quantiles(panel, width, stride, q, ranks, chunk, collect_cap)
    windows, found, passes = _scan_quantiles_folded(panel, "scan-quantiles-panel", fasta_or_sequences, width, stride,
                                                    [want] * panel.n_models, int(collect_cap), device,
                                                    chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_pass)
    scored = np.array([s.n for s in found], dtype=np.int64)
    return dict(scored=scored, unscored=windows - scored, q=qs, ranks=np.stack([s.ranks for s in found]),
                values=np.stack([s.values for s in found]), passes=passes)


def write_tail_counts(path, result):
    """The `scan-tail` output: #scored<TAB>n<TAB>unscored<TAB>m, then threshold<TAB>count per threshold in the caller's
    order, the threshold at %.17g, which reads back to the same double."""
    with open(path, "w") as f:
        f.write("#scored\t%d\tunscored\t%d\n" % (result["scored"], result["unscored"]))
        f.write("".join("%.17g\t%d\n" % row for row in zip(result["thresholds"].tolist(), result["counts"].tolist())))


def _read_dist(path, nlead, convert):
    """-> ([the fields of the #scored lines], [the converted fields of the other lines]); nlead: names in front"""
    heads, rows = [], []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            fields = line.split("\t")
            if fields[nlead] == "#scored":
                heads.append(tuple(fields[:nlead]) + (int(fields[nlead + 1]), int(fields[nlead + 3])))
            else:
                rows.append(tuple(fields[:nlead]) + tuple(c(x) for c, x in zip(convert, fields[nlead:])))
    return heads, rows


def read_tail_counts(path):
    """-> dict(scored, unscored, thresholds, counts) from a file written by write_tail_counts."""
    (head,), rows = _read_dist(path, 0, (float, int))
    return dict(scored=head[0], unscored=head[1], thresholds=np.array([r[0] for r in rows], dtype=np.float64),
                counts=np.array([r[1] for r in rows], dtype=np.int64))


def write_panel_tail_counts(path, panel_names, result):
    """The `scan-tail-panel` output: write_tail_counts' lines per member in panel order, the member's name in front."""
    with open(path, "w") as f:
        for m, member in enumerate(panel_names):
            f.write("%s\t#scored\t%d\tunscored\t%d\n" % (member, result["scored"][m], result["unscored"][m]))
            f.write("".join("%s\t%.17g\t%d\n" % ((member,) + row)
                            for row in zip(result["thresholds"].tolist(), result["counts"][m].tolist())))


def read_panel_tail_counts(path):
    """-> ([(member, scored, unscored)], [(member, threshold, count)]) from a file written by write_panel_tail_counts."""
    return _read_dist(path, 1, (float, int))


def _q_text(q, i):
    return "-" if q is None else "%.17g" % q[i]


def _q_value(text):
    return None if text == "-" else float(text)


def write_quantiles(path, result):
    """The `scan-quantiles` output: #scored<TAB>n<TAB>unscored<TAB>m, then q<TAB>rank<TAB>value per request in the
    caller's order, q ("-" when ranks were asked for) and the value at %.17g."""
    with open(path, "w") as f:
        f.write("#scored\t%d\tunscored\t%d\n" % (result["scored"], result["unscored"]))
        for i, (r, v) in enumerate(zip(result["ranks"].tolist(), result["values"].tolist())):
            f.write("%s\t%d\t%.17g\n" % (_q_text(result["q"], i), r, v))


def read_quantiles(path):
    """-> dict(scored, unscored, q, ranks, values) from a file written by write_quantiles (q: None where "-")."""
    (head,), rows = _read_dist(path, 0, (_q_value, int, float))
    q = [r[0] for r in rows]
    return dict(scored=head[0], unscored=head[1], q=None if None in q else q,
                ranks=np.array([r[1] for r in rows], dtype=np.int64), values=np.array([r[2] for r in rows], dtype=np.float64))


def write_panel_quantiles(path, panel_names, result):
    """The `scan-quantiles-panel` output: write_quantiles' lines per member in panel order, the member's name in front."""
    with open(path, "w") as f:
        for m, member in enumerate(panel_names):
            f.write("%s\t#scored\t%d\tunscored\t%d\n" % (member, result["scored"][m], result["unscored"][m]))
            for i, (r, v) in enumerate(zip(result["ranks"][m].tolist(), result["values"][m].tolist())):
                f.write("%s\t%s\t%d\t%.17g\n" % (member, _q_text(result["q"], i), r, v))


def read_panel_quantiles(path):
    """-> ([(member, scored, unscored)], [(member, q or None, rank, value)]) from a file written by
    write_panel_quantiles."""
    return _read_dist(path, 1, (_q_value, int, float))
