"""CPU reference of the window alignment, for the walign tests: the recurrence, the best cell and the
traceback as plain loops over a numpy K in Python floats -- nothing shared with the device code or
gkmqc_amd/gkmwindows.py.  Also a block-wise rendering of the carry protocol (a row vector and a column vector updated in
place, the saved corner, the blocks of y visited in descending order for the reverse orientation), which the host tests
hold against the whole-matrix DP.  Test infrastructure."""
import numpy as np

STOP, DIAG, UP, LEFT = 0, 1, 2, 3


def cell(v, diag, up, left, offset, gap):
    """one cell of the recurrence -> (h, dir): strict comparisons in the order DIAG, UP, LEFT"""
    h, d = 0.0, STOP
    if v == v:
        t = diag + (v - offset)
        if t > h:
            h, d = t, DIAG
    t = up - gap
    if t > h:
        h, d = t, UP
    t = left - gap
    if t > h:
        h, d = t, LEFT
    return h, d


def dp_block(K, flip, offset, gap, top, left, corner):
    """The DP over one block in DP coordinates (column c reads K[i, n - 1 - c] with flip): top (n floats) = H(-1, c),
    left (m floats) = H(i, -1), corner = H(-1, -1) -> (H (m, n) float64, D (m, n) uint8).  top and left are not changed."""
    m, n = K.shape
    offset, gap = float(offset), float(gap)
    rows = K.tolist()
    above = [float(corner)] + [float(t) for t in top]          # H(i - 1, -1 .. n - 1), Python floats throughout
    edge = [float(t) for t in left]
    H, D = [], []
    for i in range(m):
        cur, dirs = [edge[i]], []                              # H(i, -1 .. )
        kr = rows[i][::-1] if flip else rows[i]
        for c in range(n):
            h, d = cell(kr[c], above[c], above[c + 1], cur[c], offset, gap)
            cur.append(h)
            dirs.append(d)
        H.append(cur[1:])
        D.append(dirs)
        above = cur
    return np.array(H, dtype=np.float64).reshape(m, n), np.array(D, dtype=np.uint8).reshape(m, n)


def best_cell(H):
    """the largest H, the lower i and then the lower c on a tie -> (h, i, c); (0.0, -1, -1) where no cell is positive"""
    bh, bi, bc = 0.0, -1, -1
    for i, row in enumerate(H.tolist()):
        for c, h in enumerate(row):
            if h > bh:
                bh, bi, bc = h, i, c
    return bh, bi, bc


def better(a, b):
    """(h, i, c) a replaces b under the total order (as the host combines the blocks' best cells)"""
    return a[0] > b[0] or (a[0] == b[0] and a[0] > 0.0 and (a[1], a[2]) < (b[1], b[2]))


def trace(D, i, c):
    """walks D back from (i, c) -> (the DIAG cells [(i, c)] from the end backwards, the cell at which the walk stopped:
    a STOP cell (any byte but 1, 2, 3), or the first cell outside the matrix)"""
    pairs = []
    while i >= 0 and c >= 0:
        d = int(D[i, c])
        if d == DIAG:
            pairs.append((i, c))
            i, c = i - 1, c - 1
        elif d == UP:
            i -= 1
        elif d == LEFT:
            c -= 1
        else:
            break
    return pairs, (i, c)


def align(K, offset, gap, orientation="forward"):
    """The whole-matrix alignment of one orientation -> dict(score, end (i, c), pairs [(i, c)] ascending, stop, H, D), in
    DP coordinates; the column of y of DP column c is c forward and nB - 1 - c reverse."""
    m, n = K.shape
    H, D = dp_block(K, orientation == "reverse", offset, gap, [0.0] * n, [0.0] * m, 0.0)
    h, i, c = best_cell(H)
    pairs, stop = trace(D, i, c) if i >= 0 else ([], (i, c))
    return dict(score=h, end=(i, c), pairs=pairs[::-1], stop=stop, H=H, D=D)


def align_both(K, offset, gap):
    """forward and reverse; the larger score, forward on a tie -> (orientation, align(...))"""
    f, r = align(K, offset, gap, "forward"), align(K, offset, gap, "reverse")
    return ("reverse", r) if r["score"] > f["score"] else ("forward", f)


def y_index(c, nB, orientation):
    return nB - 1 - c if orientation == "reverse" else c


def align_blocks(K, offset, gap, orientation, bx, by):
    """The carry protocol: K cut into blocks of bx rows by by columns OF y; the blocks of a row of blocks are visited in
    ascending DP column (descending y for reverse).  One row vector of nB floats for the whole matrix and one column
    vector per row of blocks, both overwritten in place by every block with its last row and column; before a block
    runs, row[c1 - 1] is saved as the corner of the block to its right.  -> (score, end, D) as `align` gives them."""
    m, n = K.shape
    flip = orientation == "reverse"
    row = np.zeros(n)
    D = np.zeros((m, n), dtype=np.uint8)
    best = (0.0, -1, -1)
    ycuts = [(j0, min(j0 + by, n)) for j0 in range(0, n, by)]
    if flip:
        ycuts = ycuts[::-1]
    for i0 in range(0, m, bx):
        i1 = min(i0 + bx, m)
        col = np.zeros(i1 - i0)
        corner = 0.0
        for j0, j1 in ycuts:
            c0, c1 = (n - j1, n - j0) if flip else (j0, j1)
            saved = float(row[c1 - 1])
            H, Db = dp_block(K[i0:i1, j0:j1], flip, offset, gap, row[c0:c1], col, corner)
            row[c0:c1] = H[-1]
            col[:] = H[:, -1]
            corner = saved
            D[i0:i1, c0:c1] = Db
            h, i, c = best_cell(H)
            if i >= 0 and better((h, i + i0, c + c0), best):
                best = (h, i + i0, c + c0)
    return best[0], (best[1], best[2]), D


# ------------------------------------------------------------------ the planted case the host and GPU tests share
PLANT = dict(kernel_type=0, L=8, k=5, d=2, width=60, stride=10, offset=0.25, gap=0.2)


def complement_reverse(x):
    x = np.asarray(x)
    return np.where(x < 4, 3 - x, x)[::-1].astype(np.uint8)


def planted(reverse=False, n_run=None):
    """default_rng(7): x 700 iid bases; x[200:500] with 8 % substitutions and the 20 bases [340:360) deleted (280 bases)
    planted at y[100:380] of 600 iid bases -- its reverse complement instead with `reverse`; n_run = (a, b): y[a:b] made N
    afterwards -> (x, y)"""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 4, size=700, dtype=np.uint8)
    y = rng.integers(0, 4, size=600, dtype=np.uint8)
    seg = x[200:500].copy()
    hit = rng.random(300) < 0.08
    seg[hit] = (seg[hit] + rng.integers(1, 4, size=int(hit.sum()))) % 4
    seg = np.concatenate((seg[:140], seg[160:])).astype(np.uint8)
    assert len(seg) == 280
    y[100:380] = complement_reverse(seg) if reverse else seg
    if n_run is not None:
        y[n_run[0]:n_run[1]] = 4
    return x, y


# forward plant: x base 200 + u <-> y base 100 + u before the deletion (u < 140), x base 200 + u <-> y base 80 + u after
# it (u >= 160): window starts on the diagonals x_start - y_start = 100 and 120
PLANT_DIAGONALS = (100, 120)
