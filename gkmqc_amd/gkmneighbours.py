"""Which sequences of a set are near-copies of one another, or of a second set, by the gkm kernel itself: the k nearest
neighbours of every sequence, every pair at or above a threshold, redundancy groups, a de-duplicated set and
cross-validation folds that never split a group.

The kernel values are computed in blocks on the device as `score` computes them (gram_block + normalize_block) and reduced
there (device.knn_merge, pairs_count, pairs_fill): only the lists come back, never a block of the matrix."""
import argparse
import math
import os
import sys

import numpy as np

from . import device as dv
from .gkmmodel import ModelError
from .gkmquery import BLOCK_BYTES, _as_queries

MAX_NEIGHBOURS = 64       # entries of a row's list: one per lane of the wave that keeps it (gkmhip_knn_merge's kcap)
ROW_CHUNK = 16384         # sequences on the rows of one Gram launch at the most


# ------------------------------------------------------------------ the block loop
def _check_sets(what, rows, cols, kernel_type, L, k, d, block):
    bad = dv.check_parameters(kernel_type, L, k, d)
    if bad:
        raise ModelError("%s: %s" % (what, bad))
    if block is not None and int(block) < 1:
        raise ModelError("%s: block must be at least 1" % what)
    for name, s in (("sequence", rows), ("pool sequence", cols)):
        if len(s) == 0:
            raise ModelError("%s: no %ss" % (what, name))
        short = np.nonzero(np.diff(s.off) < L)[0]
        if len(short):
            raise ModelError("%s: %s %d is shorter than L = %d" % (what, name, int(short[0]), L))
    if len(rows) + len(cols) >= 2 ** 31:
        raise ModelError("%s: too many sequences" % what)


def default_block(n_rows, n_cols, budget=BLOCK_BYTES):
    """Pool sequences per column block: the rows' chunk (at most ROW_CHUNK) times the block, as kernel values and as the
    Gram kernel's tile-transposed output (about as big), within `budget` bytes of device memory."""
    rows = max(64, min(int(n_rows), ROW_CHUNK))
    return int(max(1, min(int(n_cols), budget // (16 * rows))))


def _row_chunk(n_rows, block, budget=BLOCK_BYTES):
    return int(max(1, min(int(n_rows), ROW_CHUNK, budget // (16 * max(int(block), 64)))))


class _Tiles:
    """The kernel between the sequences `rows` and the sequences `cols` (FlatSequences) as device blocks.  Iterating
    uploads, per (chunk of rows, block of cols), [the chunk; the block] into the cached context, takes that set's self
    norms, runs gram_block and normalize_block with the chunk on the launch's rows and the block on its column range into
    the one buffer G (leading dimension `ld`), and yields (r0, r1, c0, c1): G[i * ld + j] = K(rows[r0 + i], cols[c0 + j]).
    No cell is a sequence against its own uploaded copy, so no value is forced to 1.0.  skip(r0, r1, c0, c1): tiles
    for which it returns true are not computed.  gram_ms: the Gram kernels' HIP-event milliseconds so far (timed=True)."""

    def __init__(self, rows, cols, kernel_type, L, k, d, M, H, gamma, device, block, skip=None, timed=False):
        import torch
        self.rows, self.cols = rows, cols
        self.pb = min(len(cols), int(block) if block else default_block(len(rows), len(cols)))
        self.rc = _row_chunk(len(rows), self.pb)
        self.ld = self.pb
        self.ctx = dv.cached_context(kernel_type, L, k, d, M, H, gamma, device=device)
        self.device = device
        self.dev = torch.device("cuda", device)
        self.skip, self.timed, self.gram_ms = skip, timed, 0.0

    def __iter__(self):
        import torch
        R, C, rc, pb, ctx = len(self.rows), len(self.cols), self.rc, self.pb, self.ctx
        with torch.cuda.device(self.dev):
            self.stream = stream = torch.cuda.current_stream().cuda_stream
            ctx.set_kernel(dv.KERNEL_AUTO)
            self.G = torch.empty((rc, pb), dtype=torch.float64, device=self.dev)
            sq = torch.empty(rc + pb, dtype=torch.float64, device=self.dev)
            for r0 in range(0, R, rc):
                r1 = min(R, r0 + rc)
                nr = r1 - r0
                launch_rows = np.arange(nr, dtype=np.int32)
                roff = self.rows.off[r0:r1 + 1]
                rcodes = self.rows.codes[roff[0]:roff[-1]]
                for c0 in range(0, C, pb):
                    c1 = min(C, c0 + pb)
                    if self.skip is not None and self.skip(r0, r1, c0, c1):
                        continue
                    coff = self.cols.off[c0:c1 + 1]
                    codes = np.concatenate((rcodes, self.cols.codes[coff[0]:coff[-1]]))
                    off = np.concatenate((roff - roff[0], (roff[-1] - roff[0]) + (coff[1:] - coff[0])))
                    ctx.set_sequences(dv.FlatSequences(codes, off), stream)     # (complete on return)
                    ctx.self_norms(sq.data_ptr(), stream)
                    ctx.gram_block(launch_rows, nr, nr + (c1 - c0), self.G.data_ptr(), self.ld, stream)
                    if self.timed:
                        torch.cuda.current_stream().synchronize()
                        self.gram_ms += ctx.last_kernel_ms()
                    ctx.normalize_block(launch_rows, nr, nr + (c1 - c0), self.G.data_ptr(), self.ld, sq.data_ptr(), stream)
                    yield r0, r1, c0, c1


class _Timer:
    """HIP-event milliseconds of the reduce kernels of a run (timed=True), the events on the stream the calls take."""

    def __init__(self, timed):
        self.timed, self.ms = timed, 0.0

    def run(self, call):
        if not self.timed:
            return call()
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        self.ms += e0.elapsed_time(e1)


def _empty_lists(n, k_nn, dev):
    import torch
    idx = torch.full((n, k_nn), -1, dtype=torch.int32, device=dev)
    val = torch.full((n, k_nn), float("nan"), dtype=torch.float64, device=dev)
    return idx, val


def _check_k(what, k_nn):
    if not 1 <= int(k_nn) <= MAX_NEIGHBOURS:
        raise ModelError("%s: k_nn must lie in 1..%d, not %d" % (what, MAX_NEIGHBOURS, int(k_nn)))
    return int(k_nn)


# ------------------------------------------------------------------ nearest neighbours
def nearest(queries, pool=None, k_nn=10, kernel_type=4, L=10, k=6, d=3, M=50, H=50.0, gamma=1.0, device=0, block=None,
            on_block=None):
    """The k_nn pool sequences with the largest kernel value for every query -> (idx (Q, k_nn) int32, val (Q, k_nn)
    float64): larger value first, on equal values the lower pool index first; -1 and nan behind the last neighbour where
    the pool holds fewer than k_nn eligible sequences.  A NaN kernel value (a type with negative weights can give a
    negative squared norm) is never a neighbour.  pool=None: the queries against themselves, and a sequence is never its
    own neighbour.  queries, pool: a FASTA file, a list of base-code arrays or a FlatSequences.

    The queries go on the Gram launch's rows, the pool in blocks of `block` sequences (default_block) on its column range,
    so that a query's candidates lie along a row of the block; queries beyond ROW_CHUNK, or beyond what
    fits beside the block, are served chunk after chunk.  The lists are the same bytes for every block size.
    on_block(dict) (measurements): called after every tile with its shape and the HIP-event milliseconds of the Gram and
    the merge kernel so far."""
    import torch
    k_nn = _check_k("nearest", k_nn)
    rows, _ = _as_queries(queries)
    cols = rows if pool is None else _as_queries(pool)[0]
    _check_sets("nearest", rows, cols, kernel_type, L, k, d, block)
    timed = on_block is not None
    tiles = _Tiles(rows, cols, kernel_type, L, k, d, M, H, gamma, device, block, timed=timed)
    timer = _Timer(timed)
    out_idx = np.empty((len(rows), k_nn), dtype=np.int32)
    out_val = np.empty((len(rows), k_nn), dtype=np.float64)
    lists, at = None, None
    with torch.cuda.device(tiles.dev):
        def flush():
            if lists is not None:
                out_idx[at[0]:at[1]] = lists[0][:at[1] - at[0]].cpu().numpy()
                out_val[at[0]:at[1]] = lists[1][:at[1] - at[0]].cpu().numpy()

        for r0, r1, c0, c1 in tiles:
            if at is None or at[0] != r0:
                flush()
                lists, at = _empty_lists(tiles.rc, k_nn, tiles.dev), (r0, r1)
                ids = (torch.arange(r0, r1, dtype=torch.int32, device=tiles.dev) if pool is None
                       else torch.full((r1 - r0,), -1, dtype=torch.int32, device=tiles.dev))
            timer.run(lambda: dv.knn_merge(device, tiles.G.data_ptr(), tiles.ld, r1 - r0, c1 - c0, ids.data_ptr(), c0, 0,
                                           k_nn, lists[0].data_ptr(), lists[1].data_ptr(), tiles.stream))
            if on_block is not None:
                on_block(dict(rows=r1 - r0, cols=c1 - c0, gram_kernel_ms=tiles.gram_ms, merge_kernel_ms=timer.ms,
                              kernel=tiles.ctx.last_kernel_name()))
        flush()
    return out_idx, out_val


def _as_matrix(what, K):
    import torch
    if not (isinstance(K, torch.Tensor) and K.is_cuda and K.dtype == torch.float64 and K.dim() == 2
            and K.shape[0] > 0 and K.shape[1] > 0 and K.stride(1) == 1 and K.stride(0) >= K.shape[1]):
        raise ModelError("%s: K must be a non-empty two-dimensional float64 CUDA tensor with contiguous rows" % what)
    return K.device.index or 0


def nearest_in_matrix(K, k_nn, exclude_self=True):
    """`nearest` for a matrix that is already on the device (gram_matrix(symmetric=True)["K"], a cross_kernel block):
    row i's k_nn best columns -> (idx, val) as `nearest` returns them.  exclude_self: column i is not row i's."""
    import torch
    k_nn = _check_k("nearest_in_matrix", k_nn)
    device = _as_matrix("nearest_in_matrix", K)
    n, m = K.shape
    with torch.cuda.device(K.device):
        idx, val = _empty_lists(n, k_nn, K.device)
        ids = (torch.arange(n, dtype=torch.int32, device=K.device) if exclude_self
               else torch.full((n,), -1, dtype=torch.int32, device=K.device))
        dv.knn_merge(device, K.data_ptr(), K.stride(0), n, m, ids.data_ptr(), 0, 0, k_nn, idx.data_ptr(), val.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        return idx.cpu().numpy(), val.cpu().numpy()


# ------------------------------------------------------------------ pairs at or above a threshold
class _PairSink:
    """The pairs of the tiles of a run, counted first: once the total passes max_pairs nothing more is filled, the
    counting goes on, and finish() raises with the whole count."""

    def __init__(self, what, device, threshold, max_pairs, timer):
        self.what, self.device, self.threshold, self.max_pairs, self.timer = what, device, float(threshold), int(max_pairs), timer
        self.total, self.parts = 0, []

    def take(self, K_ptr, ld, nrows, ncols, ids, col_base, mode, stream):
        import torch
        dev = ids.device
        count = torch.empty(nrows, dtype=torch.int64, device=dev)
        self.timer.run(lambda: dv.pairs_count(self.device, K_ptr, ld, nrows, ncols, ids.data_ptr(), col_base, mode,
                                              self.threshold, count.data_ptr(), stream))
        here = int(count.sum().item())
        self.total += here
        if here == 0 or self.total > self.max_pairs:
            return
        offset = torch.cumsum(count, 0) - count
        oi = torch.empty(here, dtype=torch.int32, device=dev)
        oj = torch.empty(here, dtype=torch.int32, device=dev)
        ov = torch.empty(here, dtype=torch.float64, device=dev)
        self.timer.run(lambda: dv.pairs_fill(self.device, K_ptr, ld, nrows, ncols, ids.data_ptr(), col_base, mode,
                                             self.threshold, offset.data_ptr(), here, oi.data_ptr(), oj.data_ptr(),
                                             ov.data_ptr(), stream))
        self.parts.append((oi.cpu().numpy(), oj.cpu().numpy(), ov.cpu().numpy()))

    def finish(self, i_base=0):
        if self.total > self.max_pairs:
            raise ModelError("%s: %d pairs at or above the threshold, more than max_pairs = %d"
                             % (self.what, self.total, self.max_pairs))
        if not self.parts:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
        i = np.concatenate([p[0] for p in self.parts]) - np.int32(i_base)
        j = np.concatenate([p[1] for p in self.parts])
        v = np.concatenate([p[2] for p in self.parts])
        order = np.lexsort((j, i))
        return i[order], j[order], v[order]


def _check_pairs(what, threshold, max_pairs):
    if math.isnan(float(threshold)):
        raise ModelError("%s: the threshold is not a number" % what)
    if int(max_pairs) < 0:
        raise ModelError("%s: max_pairs must not be negative" % what)


def pairs_above(seqs, threshold, other=None, max_pairs=1 << 24, kernel_type=4, L=10, k=6, d=3, M=50, H=50.0, gamma=1.0,
                device=0, block=None, on_block=None):
    """Every pair with a kernel value >= threshold -> (i int32, j int32, value float64), sorted by (i, j).  other=None:
    the pairs i < j within `seqs`; otherwise i indexes `seqs` and j indexes `other`.  A NaN kernel value is no pair.
    More than max_pairs pairs: ModelError naming their number, nothing returned.  seqs, other, block, on_block: as `nearest`
    takes its queries and pool (on_block's reduce time is pairs_kernel_ms)."""
    import torch
    _check_pairs("pairs_above", threshold, max_pairs)
    rows, _ = _as_queries(seqs)
    cols = rows if other is None else _as_queries(other)[0]
    _check_sets("pairs_above", rows, cols, kernel_type, L, k, d, block)
    timed = on_block is not None
    # within one set only the tiles that reach above the diagonal hold a pair i < j
    skip = (lambda r0, r1, c0, c1: c1 <= r0 + 1) if other is None else None
    tiles = _Tiles(rows, cols, kernel_type, L, k, d, M, H, gamma, device, block, skip=skip, timed=timed)
    timer = _Timer(timed)
    sink = _PairSink("pairs_above", device, threshold, max_pairs, timer)
    # a row of a second set has no own column: its id lies behind every column, and comes back as the pair's i
    base = 0 if other is None else len(cols)
    with torch.cuda.device(tiles.dev):
        for r0, r1, c0, c1 in tiles:
            ids = torch.arange(base + r0, base + r1, dtype=torch.int32, device=tiles.dev)
            sink.take(tiles.G.data_ptr(), tiles.ld, r1 - r0, c1 - c0, ids, c0, 1 if other is None else 0, tiles.stream)
            if on_block is not None:
                on_block(dict(rows=r1 - r0, cols=c1 - c0, gram_kernel_ms=tiles.gram_ms, pairs_kernel_ms=timer.ms,
                              pairs=sink.total, kernel=tiles.ctx.last_kernel_name()))
    return sink.finish(base)


def pairs_in_matrix(K, threshold, upper=True, max_pairs=1 << 24):
    """`pairs_above` for a matrix that is already on the device.  upper=True: the pairs i < j of a square matrix, read
    from its upper triangle (gram_matrix(symmetric=True)); upper=False: every cell of K, whatever its shape."""
    import torch
    _check_pairs("pairs_in_matrix", threshold, max_pairs)
    device = _as_matrix("pairs_in_matrix", K)
    n, m = K.shape
    if upper and n != m:
        raise ModelError("pairs_in_matrix: the upper triangle needs a square matrix, not %d x %d" % (n, m))
    sink = _PairSink("pairs_in_matrix", device, threshold, max_pairs, _Timer(False))
    base = 0 if upper else m
    with torch.cuda.device(K.device):
        ids = torch.arange(base, base + n, dtype=torch.int32, device=K.device)
        sink.take(K.data_ptr(), K.stride(0), n, m, ids, 0, 1 if upper else 0, torch.cuda.current_stream().cuda_stream)
    return sink.finish(base)


# ------------------------------------------------------------------ groups, representatives, folds (host)
def redundancy_groups(n, i, j):
    """The connected components of the graph on 0..n-1 with the edges (i[e], j[e]) -> labels int64[n]: a sequence's
    label is the lowest member of its component (union-find, the lower root kept)."""
    n = int(n)
    i, j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
    if n < 0 or len(i) != len(j):
        raise ModelError("redundancy_groups: i and j must hold one entry per edge")
    if len(i) and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n):
        raise ModelError("redundancy_groups: an edge names a sequence outside 0..%d" % (n - 1))
    parent = list(range(n))

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n)], dtype=np.int64)


def _check_labels(what, labels, n=None):
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if n is not None and len(labels) != n:
        raise ModelError("%s: %d labels for %d sequences" % (what, len(labels), n))
    at = np.arange(len(labels))
    if len(labels) and (labels.min() < 0 or (labels > at).any() or (labels[labels] != labels).any()):
        raise ModelError("%s: a label must be the lowest member of its group" % what)
    return labels


def representatives(labels):
    """The lowest member of each group, ascending: what a de-duplicated set keeps."""
    labels = _check_labels("representatives", labels)
    return np.nonzero(labels == np.arange(len(labels)))[0].astype(np.int64)


def grouped_plan(n_pseqs, n_nseqs, labels, ncv=5, seed=1):
    """Cross-validation folds that never split a redundancy group, as a plan in svmcv.plan_folds' format (sizes, y,
    n_folds, which, u_trains, u_tests) for crossValidate(plan=...): the n_pseqs positives come first, `labels` as
    redundancy_groups gives them for all n_pseqs + n_nseqs sequences.

    The groups are dealt largest first; groups of one size in the order of a permutation of the ascending labels drawn
    from numpy's RandomState(seed).  A group goes to the fold that holds the fewest sequences of the group's majority
    class (positive on a tie) so far, then the fewest sequences, then the lowest number.  One repeat of ncv folds, each
    sequence tested once.  Refused: a grouping that leaves a fold's test part or training part without both classes."""
    n_pseqs, n_nseqs, ncv = int(n_pseqs), int(n_nseqs), int(ncv)
    n = n_pseqs + n_nseqs
    if ncv < 2:
        raise ModelError("grouped_plan: ncv must be at least 2, not %d" % ncv)
    if n_pseqs < 1 or n_nseqs < 1:
        raise ModelError("grouped_plan: both classes need at least one sequence")
    labels = _check_labels("grouped_plan", labels, n)
    y = np.concatenate((np.repeat(1, n_pseqs), np.repeat(0, n_nseqs)))
    uniq, inverse, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    pos = np.bincount(inverse, weights=y, minlength=len(uniq)).astype(np.int64)
    key = np.random.RandomState(int(seed)).permutation(len(uniq))
    order = np.lexsort((key, -sizes))
    fold_of_group = np.empty(len(uniq), dtype=np.int64)
    held = np.zeros((ncv, 2), dtype=np.int64)     # per fold: negatives, positives
    for g in order.tolist():
        p, q = int(pos[g]), int(sizes[g] - pos[g])
        cls = 1 if p >= q else 0
        f = min(range(ncv), key=lambda f: (held[f, cls], held[f, 0] + held[f, 1], f))
        fold_of_group[g] = f
        held[f, 1] += p
        held[f, 0] += q
    fold = fold_of_group[inverse]
    u_trains, u_tests = [], []
    for f in range(ncv):
        test = np.nonzero(fold == f)[0].astype(np.int64)
        train = np.nonzero(fold != f)[0].astype(np.int64)
        for part, name in ((test, "test"), (train, "training")):
            if len(part) == 0 or y[part].min() == y[part].max():
                raise ModelError("grouped_plan: the %s part of fold %d does not hold both classes (the groups are too few "
                                 "or too large for %d folds)" % (name, f, ncv))
        u_trains.append(train)
        u_tests.append(test)
    return dict(sizes=(n_pseqs, n_nseqs), y=y, n_folds=ncv, which=list(range(ncv)), u_trains=u_trains, u_tests=u_tests)


def plan_fold_of(plan):
    """fold[s] = the fold that tests sequence s, from a plan."""
    fold = np.full(len(plan["y"]), -1, dtype=np.int64)
    for f, test in enumerate(plan["u_tests"]):
        fold[test] = f
    return fold


def dedupe(seqs, threshold, max_pairs=1 << 24, **kernel):
    """-> (keep, labels): the redundancy groups of `seqs` under kernel value >= threshold (pairs_above's arguments) and
    the lowest member of each."""
    flat, _ = _as_queries(seqs)
    i, j, _v = pairs_above(flat, threshold, max_pairs=max_pairs, **kernel)
    labels = redundancy_groups(len(flat), i, j)
    return representatives(labels), labels


# ------------------------------------------------------------------ files
def _fields(path, no, line, count):
    fields = line.split("\t")
    if len(fields) != count:
        raise ModelError("%s:%d: expected %d tab-separated fields" % (path, no, count))
    return fields


def _lines(path):
    with open(path) as f:
        return list(enumerate(f.read().split("\n")[:-1], 1))


def write_nearest(path, names, idx, val):
    """The `nearest` output: one line per query, name<TAB>i0,i1,...<TAB>v0,v1,... (pool indices, -1 where there is no
    further neighbour; repr() floats, which read back to the same doubles, nan beside a -1)."""
    with open(path, "w") as f:
        for name, ii, vv in zip(names, idx.tolist(), val.tolist()):
            f.write("%s\t%s\t%s\n" % (name, ",".join("%d" % e for e in ii), ",".join(repr(float(e)) for e in vv)))


def read_nearest(path):
    """-> (names, idx int32 (Q, k_nn), val float64 (Q, k_nn)) from a file written by write_nearest."""
    names, idx, val = [], [], []
    for no, line in _lines(path):
        name, ii, vv = _fields(path, no, line, 3)
        try:
            idx.append([int(e) for e in ii.split(",")])
            val.append([float(e) for e in vv.split(",")])
        except ValueError:
            raise ModelError("%s:%d: expected integers and numbers" % (path, no))
        if len(idx[-1]) != len(val[-1]) or len(idx[-1]) != len(idx[0]):
            raise ModelError("%s:%d: the lists' lengths do not fit" % (path, no))
        names.append(name)
    k_nn = len(idx[0]) if idx else 0
    return names, np.array(idx, dtype=np.int32).reshape(-1, k_nn), np.array(val, dtype=np.float64).reshape(-1, k_nn)


def write_pairs(path, i, j, v, names_i, names_j):
    """The `pairs` output: one line per pair, i<TAB>j<TAB>name_i<TAB>name_j<TAB>K (0-based indices; K at %.17g)."""
    with open(path, "w") as f:
        for a, b, x in zip(i.tolist(), j.tolist(), v.tolist()):
            f.write("%d\t%d\t%s\t%s\t%.17g\n" % (a, b, names_i[a], names_j[b], x))


def read_pairs(path):
    """-> (i int32, j int32, value float64) from a file written by write_pairs."""
    rows = []
    for no, line in _lines(path):
        f = _fields(path, no, line, 5)
        try:
            rows.append((int(f[0]), int(f[1]), float(f[4])))
        except ValueError:
            raise ModelError("%s:%d: expected two integers, two names and a number" % (path, no))
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
            np.array([r[2] for r in rows], dtype=np.float64))


def write_groups(path, names, labels):
    """The groups table of `dedupe`: one line per sequence, index<TAB>name<TAB>group (the group's lowest member)<TAB>1 if
    the sequence is kept, else 0."""
    with open(path, "w") as f:
        for s, (name, g) in enumerate(zip(names, np.asarray(labels).tolist())):
            f.write("%d\t%s\t%d\t%d\n" % (s, name, g, int(g == s)))


def read_groups(path):
    """-> (names, labels int64) from a file written by write_groups."""
    names, labels = [], []
    for no, line in _lines(path):
        f = _fields(path, no, line, 4)
        try:
            if int(f[0]) != len(names):
                raise ValueError
            labels.append(int(f[2]))
        except ValueError:
            raise ModelError("%s:%d: expected the running index, a name, a group and a flag" % (path, no))
        names.append(f[1])
    return names, _check_labels(path, labels)


def write_folds(path, names, plan, labels):
    """The `folds` output: one line per sequence, index<TAB>name<TAB>class (1 positive, 0 negative)<TAB>group<TAB>fold."""
    fold = plan_fold_of(plan)
    with open(path, "w") as f:
        for s, name in enumerate(names):
            f.write("%d\t%s\t%d\t%d\t%d\n" % (s, name, int(plan["y"][s]), int(labels[s]), int(fold[s])))


def read_folds(path):
    """-> (names, labels, plan) from a file written by write_folds: the plan as grouped_plan returned it."""
    names, y, labels, fold = [], [], [], []
    for no, line in _lines(path):
        f = _fields(path, no, line, 5)
        try:
            if int(f[0]) != len(names):
                raise ValueError
            y.append(int(f[2]))
            labels.append(int(f[3]))
            fold.append(int(f[4]))
        except ValueError:
            raise ModelError("%s:%d: expected the running index, a name, a class, a group and a fold" % (path, no))
        names.append(f[1])
    y, fold = np.array(y, dtype=np.int64), np.array(fold, dtype=np.int64)
    n_p = int(y.sum())
    if len(y) == 0 or not ((y[:n_p] == 1).all() and (y[n_p:] == 0).all()) or fold.min() < 0:
        raise ModelError("%s: the positives must come first and every sequence needs a fold" % path)
    ncv = int(fold.max()) + 1
    at = np.arange(len(y), dtype=np.int64)
    plan = dict(sizes=(n_p, len(y) - n_p), y=y, n_folds=ncv, which=list(range(ncv)),
                u_trains=[at[fold != f] for f in range(ncv)], u_tests=[at[fold == f] for f in range(ncv)])
    return names, _check_labels(path, labels), plan


_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_fasta(path, seqs, names, keep):
    """The records `keep` of a FlatSequences as FASTA, the bases as the kernel read them (ACGT)."""
    with open(path, "wb") as f:
        for s in np.asarray(keep).tolist():
            f.write(b">" + names[s].encode() + b"\n" + _LETTERS[seqs[s]].tobytes() + b"\n")


# ------------------------------------------------------------------ command line
def build_parser():
    p = argparse.ArgumentParser(prog="gkmneighbours", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, text in (("nearest", "the nearest pool sequences of every query -> TSV"),
                       ("pairs", "every pair at or above a kernel value -> TSV"),
                       ("dedupe", "one sequence per redundancy group -> PREFIX.pos.fa (PREFIX.neg.fa) and PREFIX.groups.tsv"),
                       ("folds", "cross-validation folds that split no redundancy group -> TSV")):
        q = sub.add_parser(name, help=text)
        if name == "nearest":
            q.add_argument("-K", "--neighbours", type=int, default=10, help="neighbours per query (1..%d, default 10)"
                           % MAX_NEIGHBOURS)
            q.add_argument("--pool", default=None, help="FASTA file of the pool (default: the queries themselves)")
        else:
            q.add_argument("--threshold", type=float, required=True, help="the kernel value a pair must reach")
            q.add_argument("--max-pairs", type=int, default=1 << 24, help="refuse more pairs than this (default 2^24)")
        if name == "pairs":
            q.add_argument("--other", default=None, help="FASTA file of a second set (default: pairs within the one set)")
        if name == "dedupe":
            q.add_argument("-n", "--negatives", default=None, help="FASTA file of the negative set, de-duplicated with the "
                           "first as one set")
        if name == "folds":
            q.add_argument("-x", "--ncv", type=int, default=5, help="folds (default 5)")
            q.add_argument("-s", "--seed", type=int, default=1, help="seed of the groups' order (default 1)")
        q.add_argument("--block", type=int, default=None, help="pool sequences per device block")
        q.add_argument("-t", "--kernel-type", type=int, default=4, help="0 gkm, 1 full filter, 2 truncated filter, 3 gkm "
                       "with RBF, 4 wgkm, 5 wgkm with RBF (default 4)")
        q.add_argument("-L", "--full-word-length", type=int, default=10)
        q.add_argument("-k", "--non-gap-length", type=int, default=6)
        q.add_argument("-d", "--max-num-gaps", type=int, default=3)
        q.add_argument("-M", "--pos-weight-max", type=int, default=50)
        q.add_argument("-H", "--pos-weight-half", type=float, default=50.0)
        q.add_argument("-G", "--rbf-gamma", type=float, default=1.0)
        q.add_argument("--device", type=int, default=0)
        q.add_argument("fasta", help="the sequences" if name != "folds" else "the positive set")
        if name == "folds":
            q.add_argument("negatives", help="the negative set")
        q.add_argument("output", help="the output file" if name != "dedupe" else "the prefix of the output files")
    return p


def _join(a, b):
    codes = np.concatenate((a.codes, b.codes))
    return dv.FlatSequences(codes, np.concatenate((a.off, a.off[-1] + b.off[1:])))


def _replace_all(pairs):
    for tmp, path in pairs:
        os.replace(tmp, path)


def main(argv=None):
    a = build_parser().parse_args(argv)
    kernel = dict(kernel_type=a.kernel_type, L=a.full_word_length, k=a.non_gap_length, d=a.max_num_gaps,
                  M=a.pos_weight_max, H=a.pos_weight_half, gamma=a.rbf_gamma, device=a.device, block=a.block)
    tmp = a.output + ".tmp"
    try:
        if a.cmd == "nearest":
            _check_k("nearest", a.neighbours)
            seqs, names, _, _ = dv.read_fasta(a.fasta)
            pool = dv.read_fasta(a.pool)[0] if a.pool else None
            idx, val = nearest(seqs, pool, a.neighbours, **kernel)
            write_nearest(tmp, names, idx, val)
            os.replace(tmp, a.output)
            print("%d queries, %d neighbours each -> %s" % (len(names), a.neighbours, a.output), file=sys.stderr)
            return 0
        _check_pairs(a.cmd, a.threshold, a.max_pairs)
        if a.cmd == "folds" and a.ncv < 2:
            raise ModelError("folds: ncv must be at least 2, not %d" % a.ncv)
        seqs, names, _, _ = dv.read_fasta(a.fasta)
        if a.cmd == "pairs":
            other, other_names = (dv.read_fasta(a.other)[:2] if a.other else (None, names))
            i, j, v = pairs_above(seqs, a.threshold, other, a.max_pairs, **kernel)
            write_pairs(tmp, i, j, v, names, other_names)
            os.replace(tmp, a.output)
            print("%d pairs at or above %g -> %s" % (len(i), a.threshold, a.output), file=sys.stderr)
            return 0
        n_p = len(seqs)
        second = a.negatives
        if second:
            neg, neg_names, _, _ = dv.read_fasta(second)
            seqs, names = _join(seqs, neg), names + neg_names
        keep, labels = dedupe(seqs, a.threshold, a.max_pairs, **kernel)
        if a.cmd == "dedupe":
            done = [(tmp + ".pos", a.output + ".pos.fa"), (tmp + ".groups", a.output + ".groups.tsv")]
            write_fasta(done[0][0], seqs, names, keep[keep < n_p])
            write_groups(done[1][0], names, labels)
            if second:
                done.append((tmp + ".neg", a.output + ".neg.fa"))
                write_fasta(done[2][0], seqs, names, keep[keep >= n_p])
            _replace_all(done)
            print("%d of %d sequences kept -> %s.*" % (len(keep), len(names), a.output), file=sys.stderr)
        else:
            plan = grouped_plan(n_p, len(names) - n_p, labels, a.ncv, a.seed)
            write_folds(tmp, names, plan, labels)
            os.replace(tmp, a.output)
            print("%d sequences in %d groups, %d folds -> %s" % (len(names), len(keep), a.ncv, a.output), file=sys.stderr)
    except (ModelError, dv.GkmError, OSError) as e:
        print("gkmneighbours: error: %s" % e, file=sys.stderr)
        for name in (tmp, tmp + ".pos", tmp + ".neg", tmp + ".groups"):
            if os.path.exists(name):
                os.remove(name)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
