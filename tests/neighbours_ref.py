"""Plain numpy / Python restatement of what gkmqc_amd/csrc/gkm_knn.hip and gkmqc_amd/gkmneighbours.py promise (include/
gkm_hip.h): the eligibility rule, the order of a row's list, the pair listing, the connected components and
grouped_plan's dealing rule.  Written from the documents, one cell at a time; nothing here is shared with the product."""
import numpy as np


def eligible(v, c, rid, mode):
    """Cell with value v in global column c of a row whose own column is rid (-1: none)."""
    if v != v:
        return False
    return c > rid if mode == 1 else c != rid


def stands_before(v, c, w, e):
    """(v, c) before (w, e): larger value first, then the lower column; -0.0 == 0.0 as floats compare."""
    return v > w or (v == w and c < e)


def merge(K, ncols, row_id, col_base, mode, kcap, best_idx, best_val):
    """The block K[:, :ncols] merged into the running lists -> (best_idx, best_val), new arrays.  An insertion sort with
    stands_before, so that nothing but the documented order decides."""
    K = np.asarray(K, dtype=np.float64)
    out_i, out_v = np.array(best_idx, dtype=np.int32).copy(), np.array(best_val, dtype=np.float64).copy()
    for i in range(K.shape[0]):
        entries = [(out_v[i, s], int(out_i[i, s])) for s in range(kcap) if out_i[i, s] >= 0]
        for j in range(ncols):
            v, c = K[i, j], col_base + j
            if not eligible(v, c, int(row_id[i]), mode):
                continue
            at = 0
            while at < len(entries) and not stands_before(v, c, entries[at][0], entries[at][1]):
                at += 1
            entries.insert(at, (v, c))
            del entries[kcap:]
        for s in range(kcap):
            if s < len(entries):
                out_v[i, s], out_i[i, s] = entries[s]
            else:
                out_v[i, s], out_i[i, s] = np.nan, -1
    return out_i, out_v


def empty_lists(nrows, kcap):
    return np.full((nrows, kcap), -1, dtype=np.int32), np.full((nrows, kcap), np.nan, dtype=np.float64)


def topk(K, row_id, mode, kcap, col_base=0):
    K = np.asarray(K, dtype=np.float64)
    bi, bv = empty_lists(K.shape[0], kcap)
    return merge(K, K.shape[1], row_id, col_base, mode, kcap, bi, bv)


def pairs(K, ncols, row_id, col_base, mode, threshold):
    """-> per row the list of (row_id, column, value) with value >= threshold, ascending column."""
    K = np.asarray(K, dtype=np.float64)
    out = []
    for i in range(K.shape[0]):
        rid = int(row_id[i])
        out.append([(rid, col_base + j, K[i, j]) for j in range(ncols)
                    if eligible(K[i, j], col_base + j, rid, mode) and K[i, j] >= threshold])
    return out


def pairs_flat(K, row_id, mode, threshold):
    """-> (i, j, v) arrays of a whole matrix, sorted by (i, j); i is the ROW of the matrix (which is row_id[i] within one
    set; a row of a second set has no own column, row_id -1, and is still named by its row)."""
    K = np.asarray(K, dtype=np.float64)
    flat = sorted((i, c, v) for i, row in enumerate(pairs(K, K.shape[1], row_id, 0, mode, threshold)) for _, c, v in row)
    return (np.array([t[0] for t in flat], dtype=np.int32), np.array([t[1] for t in flat], dtype=np.int32),
            np.array([t[2] for t in flat], dtype=np.float64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_lists(got, want):
    """(idx, val) pairs equal: idx exactly, val bit for bit where it is a number, NaN in the same places."""
    gi, gv = got
    wi, wv = want
    nan = np.isnan(wv)
    return (np.array_equal(gi, wi) and gv.shape == wv.shape and np.array_equal(np.isnan(gv), nan)
            and same_bits(gv[~nan], wv[~nan]))


def components(n, i, j):
    """labels[s] = the lowest sequence reachable from s over the edges (flood fill from every unlabelled sequence in
    ascending order)."""
    near = [[] for _ in range(n)]
    for a, b in zip(i, j):
        near[int(a)].append(int(b))
        near[int(b)].append(int(a))
    labels = [-1] * n
    for s in range(n):
        if labels[s] >= 0:
            continue
        todo = [s]
        labels[s] = s
        while todo:
            a = todo.pop()
            for b in near[a]:
                if labels[b] < 0:
                    labels[b] = s
                    todo.append(b)
    return np.array(labels, dtype=np.int64)


def deal_groups(n_pos, n_neg, labels, ncv, seed):
    """fold[s] by grouped_plan's rule: groups largest first, equal sizes in the order of a RandomState(seed) permutation
    of the ascending labels; each to the fold with the fewest of the group's majority class (positive on a tie), then the
    fewest sequences, then the lowest number."""
    labels = [int(g) for g in labels]
    names = sorted(set(labels))
    key = np.random.RandomState(seed).permutation(len(names)).tolist()
    members = {g: [s for s in range(n_pos + n_neg) if labels[s] == g] for g in names}
    order = sorted(range(len(names)), key=lambda u: (-len(members[names[u]]), key[u]))
    held = [[0, 0] for _ in range(ncv)]
    fold = [-1] * (n_pos + n_neg)
    for u in order:
        mem = members[names[u]]
        p = sum(1 for s in mem if s < n_pos)
        q = len(mem) - p
        cls = 1 if p >= q else 0
        best = None
        for f in range(ncv):
            cand = (held[f][cls], held[f][0] + held[f][1], f)
            if best is None or cand < best:
                best = cand
        f = best[2]
        held[f][1] += p
        held[f][0] += q
        for s in mem:
            fold[s] = f
    return np.array(fold, dtype=np.int64)
