"""The neighbour entry points of include/gkm_hip.h on the GPU (gkm_knn.hip: gkmhip_knn_merge, gkmhip_pairs_count,
gkmhip_pairs_fill) driven with synthetic matrices against tests/neighbours_ref.py, byte for byte: sizes around the wave,
dense ties, sorted rows, NaN, infinities and signed zeros, short lists, own columns inside and outside the block, the
independence of the cut into column blocks, untouched memory, offsets and capacity of the pair listing, refusals."""
import numpy as np
import pytest

from tests import neighbours_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinels either side of every output
SENT_I, SENT_F, PAD = 0x5A5A5A5A, 12345.678, 7e77     # PAD: a padding cell beyond ncols, which would win every list
ALPHABET = np.array([-1.0, 0.0, 0.5, 2.0])


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def lib(dv):
    return dv._knn_lib()


class Guarded:
    """A device array of `count` elements between two runs of GUARD sentinels."""

    def __init__(self, count, dtype, init, sentinel):
        import torch
        self.count, self.sentinel = count, sentinel
        self.buf = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
        self.buf[GUARD:GUARD + count] = init

    def ptr(self):
        return self.buf[GUARD:].data_ptr()

    def set(self, host):
        import torch
        self.buf[GUARD:GUARD + self.count] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()

    def host(self):
        return self.buf[GUARD:GUARD + self.count].cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:GUARD] == self.sentinel).all() and (b[GUARD + self.count:] == self.sentinel).all())


class Block:
    """A matrix on the device with leading dimension ld > ncols, the padding holding PAD, and its row ids."""

    def __init__(self, K, row_id, pad=3):
        import torch
        self.K = np.asarray(K, dtype=np.float64)
        self.nrows, self.ncols = self.K.shape
        self.ld = self.ncols + pad
        host = np.full((self.nrows, self.ld), PAD)
        host[:, :self.ncols] = self.K
        self.host = host
        self.dK = torch.from_numpy(host).cuda()
        self.row_id = np.asarray(row_id, dtype=np.int32)
        self.d_id = torch.from_numpy(self.row_id).cuda()

    def ptr(self, c0=0):
        return self.dK.data_ptr() + 8 * c0

    def unchanged(self):
        return R.same_bits(self.dK.cpu().numpy(), self.host)


def gpu_merge(dv, blk, mode, kcap, cuts=None, col_base=0):
    """gkmhip_knn_merge over the column blocks `cuts` (pairs of columns; default: one call) -> (idx, val), after checking
    the guards and the input."""
    import torch
    bi = Guarded(blk.nrows * kcap, torch.int32, -1, SENT_I)
    bv = Guarded(blk.nrows * kcap, torch.float64, float("nan"), SENT_F)
    for c0, c1 in cuts or [(0, blk.ncols)]:
        dv.knn_merge(0, blk.ptr(c0), blk.ld, blk.nrows, c1 - c0, blk.d_id.data_ptr(), col_base + c0, mode, kcap, bi.ptr(),
                     bv.ptr())
    torch.cuda.synchronize()
    assert bi.guards_intact() and bv.guards_intact() and blk.unchanged()
    return bi.host().reshape(blk.nrows, kcap), bv.host().reshape(blk.nrows, kcap)


def same_bytes(got, want):
    return R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])


def row_ids(rng, nrows, ncols, col_base=0):
    """inside the block's columns, outside them, and -1, mixed"""
    ids = rng.integers(col_base, col_base + ncols, size=nrows)
    kind = rng.integers(0, 4, size=nrows)
    ids[kind == 1] = col_base + ncols + rng.integers(0, 5, size=int((kind == 1).sum()))
    ids[kind == 2] = -1
    return ids.astype(np.int32)


# ------------------------------------------------------------------ gkmhip_knn_merge
@pytest.mark.parametrize("kcap", [1, 5, 64])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_size_edges_with_dense_ties(dv, mode, kcap):
    rng = np.random.default_rng(100 * kcap + mode)
    for nrows in (1, 3, 65):
        for ncols in (1, 63, 64, 65, 200):
            K = ALPHABET[rng.integers(0, 4, size=(nrows, ncols))]
            K[rng.random(K.shape) < 0.05] = np.nan
            blk = Block(K, row_ids(rng, nrows, ncols, 1000))
            got = gpu_merge(dv, blk, mode, kcap, col_base=1000)
            assert same_bytes(got, R.topk(K, blk.row_id, mode, kcap, col_base=1000)), (nrows, ncols)


@pytest.mark.parametrize("kcap", [1, 5, 64])
def test_merge_sorted_rows_and_value_edges(dv, kcap):
    rng = np.random.default_rng(kcap)
    asc = np.sort(rng.random((3, 200)), axis=1)                 # every cell enters the list
    special = np.array([[0.0, -0.0, np.inf, -np.inf, -0.0, np.nan, 0.0, np.inf, 5e-324, -5e-324] * 7,
                        [np.nan] * 70,                          # no eligible cell at all
                        [-np.inf] * 69 + [np.nan]])
    few = np.full((2, 130), np.nan)                             # fewer eligible cells than kcap: trailing -1 / NaN
    few[0, [3, 64, 129]] = [0.5, 0.5, -0.0]
    few[1, 100] = 1.0
    for K, ids in ((asc, [-1, 5, 300]), (asc[:, ::-1].copy(), [-1, 5, 300]), (special, [2, -1, 68]), (few, [64, 100])):
        for mode in (0, 1):
            blk = Block(K, ids)
            got = gpu_merge(dv, blk, mode, kcap)
            want = R.topk(K, blk.row_id, mode, kcap)
            assert same_bytes(got, want), (K.shape, mode)
    got = gpu_merge(dv, Block(few, [64, 100]), 0, kcap)
    assert got[0][1].tolist() == [-1] * kcap and np.isnan(got[1][1]).all()      # its one number is its own column
    assert got[0][0, :2].tolist() == [3, 129][:min(2, kcap)]


@pytest.mark.parametrize("kcap", [1, 5, 64])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_is_independent_of_the_cut(dv, mode, kcap):
    rng = np.random.default_rng(7 + kcap)
    nrows, ncols = 5, 200
    K = ALPHABET[rng.integers(0, 4, size=(nrows, ncols))]
    K[rng.random(K.shape) < 0.05] = np.nan
    blk = Block(K, [0, 77, 199, -1, 450])
    whole = gpu_merge(dv, blk, mode, kcap)
    assert same_bytes(whole, R.topk(K, blk.row_id, mode, kcap))
    for width in (1, 7, 64):
        cuts = [(c0, min(ncols, c0 + width)) for c0 in range(0, ncols, width)]
        assert same_bytes(gpu_merge(dv, blk, mode, kcap, cuts), whole), width
        assert same_bytes(gpu_merge(dv, blk, mode, kcap, cuts[::-1]), whole), -width
    assert same_bytes(gpu_merge(dv, blk, mode, kcap), whole)                    # and two runs give the same bytes


def test_merge_carries_a_list_the_caller_filled(dv):
    """The running list is input as much as output: entries from columns of an earlier block the call never sees."""
    import torch
    K = np.array([[0.5, 0.25, 0.75, 0.5]])
    blk = Block(K, [-1])
    bi = Guarded(3, torch.int32, -1, SENT_I)
    bv = Guarded(3, torch.float64, float("nan"), SENT_F)
    bi.set(np.array([2, 9, -1], np.int32))
    bv.set(np.array([0.5, 0.5, np.nan]))
    dv.knn_merge(0, blk.ptr(), blk.ld, 1, 4, blk.d_id.data_ptr(), 10, 0, 3, bi.ptr(), bv.ptr())
    assert bi.host().tolist() == [12, 2, 9] and bv.host().tolist() == [0.75, 0.5, 0.5]
    assert bi.guards_intact() and bv.guards_intact()


# ------------------------------------------------------------------ gkmhip_pairs_count, gkmhip_pairs_fill
def gpu_pairs(dv, blk, mode, threshold, cuts=None, capacity=None, col_base=0):
    """count + fill over the column blocks -> (i, j, v, counts per block); the offsets carried from block to block the
    way the Python layer carries them: row-major within a block, blocks one behind the other."""
    import torch
    cuts = cuts or [(0, blk.ncols)]
    counts = []
    for c0, c1 in cuts:
        cnt = Guarded(blk.nrows, torch.int64, -5, -77)
        dv.pairs_count(0, blk.ptr(c0), blk.ld, blk.nrows, c1 - c0, blk.d_id.data_ptr(), col_base + c0, mode, threshold,
                       cnt.ptr())
        assert cnt.guards_intact()
        counts.append(cnt.host().copy())
    total = int(sum(c.sum() for c in counts))
    cap = total if capacity is None else capacity
    oi = Guarded(total, torch.int32, SENT_I, SENT_I)
    oj = Guarded(total, torch.int32, SENT_I, SENT_I)
    ov = Guarded(total, torch.float64, SENT_F, SENT_F)
    done = 0
    for (c0, c1), cnt in zip(cuts, counts):
        off = torch.from_numpy(done + np.cumsum(cnt) - cnt).cuda()
        dv.pairs_fill(0, blk.ptr(c0), blk.ld, blk.nrows, c1 - c0, blk.d_id.data_ptr(), col_base + c0, mode, threshold,
                      off.data_ptr(), cap, oi.ptr(), oj.ptr(), ov.ptr())
        done += int(cnt.sum())
    torch.cuda.synchronize()
    assert oi.guards_intact() and oj.guards_intact() and ov.guards_intact() and blk.unchanged()
    return oi.host(), oj.host(), ov.host(), counts


def ref_pairs(blk, mode, threshold, cuts=None, col_base=0):
    cuts = cuts or [(0, blk.ncols)]
    flat, counts = [], []
    for c0, c1 in cuts:
        rows = R.pairs(blk.K[:, c0:c1], c1 - c0, blk.row_id, col_base + c0, mode, threshold)
        counts.append(np.array([len(r) for r in rows], dtype=np.int64))
        flat.extend(t for r in rows for t in r)
    return (np.array([t[0] for t in flat], dtype=np.int32), np.array([t[1] for t in flat], dtype=np.int32),
            np.array([t[2] for t in flat], dtype=np.float64), counts)


def same_pairs(got, want):
    return (all(R.same_bits(g, w) for g, w in zip(got[:3], want[:3]))
            and all(np.array_equal(g, w) for g, w in zip(got[3], want[3])))


@pytest.mark.parametrize("mode", [0, 1])
def test_pairs_against_the_restatement(dv, mode):
    rng = np.random.default_rng(31 + mode)
    for nrows in (1, 3, 65):
        for ncols in (1, 63, 64, 65, 200):
            K = ALPHABET[rng.integers(0, 4, size=(nrows, ncols))]      # many values exactly at the threshold 0.5
            K[rng.random(K.shape) < 0.05] = np.nan
            if nrows > 2:
                K[1] = -1.0                                            # a row with no pair
                K[2] = 2.0                                             # a row with only pairs
            blk = Block(K, row_ids(rng, nrows, ncols, 50))
            got = gpu_pairs(dv, blk, mode, 0.5, col_base=50)
            want = ref_pairs(blk, mode, 0.5, col_base=50)
            assert same_pairs(got, want), (nrows, ncols)
            assert (got[2] >= 0.5).all()
    # two runs give the same bytes
    assert same_pairs(gpu_pairs(dv, blk, mode, 0.5, col_base=50), got)


def test_pairs_threshold_edges(dv):
    K = np.array([[0.5, np.nextafter(0.5, 0), np.nan, np.inf, -np.inf, -0.0, 0.0, np.nextafter(0.5, 1)]])
    blk = Block(K, [-1])
    assert gpu_pairs(dv, blk, 0, 0.5)[1].tolist() == [0, 3, 7]             # exactly at the threshold passes
    assert gpu_pairs(dv, blk, 0, 0.0)[1].tolist() == [0, 1, 3, 5, 6, 7]    # -0.0 >= 0.0
    assert gpu_pairs(dv, blk, 0, -np.inf)[1].tolist() == [0, 1, 3, 4, 5, 6, 7]   # NaN never passes
    assert gpu_pairs(dv, blk, 0, np.inf)[1].tolist() == [3]
    assert gpu_pairs(dv, blk, 0, np.nan)[1].tolist() == []


@pytest.mark.parametrize("mode", [0, 1])
def test_pairs_offsets_across_column_blocks_and_capacity(dv, mode):
    rng = np.random.default_rng(5)
    K = ALPHABET[rng.integers(0, 4, size=(9, 150))]
    blk = Block(K, [0, 10, 149, -1, 300, 70, 71, 72, 5])
    cuts = [(0, 70), (70, 150)]
    got = gpu_pairs(dv, blk, mode, 0.5, cuts)
    want = ref_pairs(blk, mode, 0.5, cuts)
    assert same_pairs(got, want) and len(got[0]) > 100
    # nothing at or beyond the capacity: the slots below it as before, the rest untouched
    cap = len(got[0]) // 2 + 1
    oi, oj, ov, _ = gpu_pairs(dv, blk, mode, 0.5, cuts, capacity=cap)
    assert R.same_bits(oi[:cap], want[0][:cap]) and R.same_bits(oj[:cap], want[1][:cap]) and R.same_bits(ov[:cap], want[2][:cap])
    assert (oi[cap:] == SENT_I).all() and (oj[cap:] == SENT_I).all() and (ov[cap:] == SENT_F).all()
    oi, _, _, _ = gpu_pairs(dv, blk, mode, 0.5, cuts, capacity=0)
    assert (oi == SENT_I).all()


# ------------------------------------------------------------------ refusals
def test_refusals_return_2_and_write_nothing(dv, lib):
    import torch
    K = np.full((4, 10), 2.0)
    blk = Block(K, [0, 1, 2, 3])
    bi = Guarded(4 * 5, torch.int32, -1, SENT_I)
    bv = Guarded(4 * 5, torch.float64, float("nan"), SENT_F)
    cnt = Guarded(4, torch.int64, -5, -77)
    off = torch.zeros(4, dtype=torch.int64, device="cuda")
    oi = Guarded(40, torch.int32, SENT_I, SENT_I)
    oj = Guarded(40, torch.int32, SENT_I, SENT_I)
    ov = Guarded(40, torch.float64, SENT_F, SENT_F)
    good = dict(K=blk.ptr(), ld=blk.ld, nrows=4, ncols=10, row_id=blk.d_id.data_ptr(), col_base=0, mode=0)
    bad = [("K", None, "NULL"), ("row_id", None, "NULL"), ("ld", 9, "ld must be at least ncols"),
           ("nrows", -1, "must not be negative"), ("ncols", -1, "must not be negative"), ("mode", 2, "mode must be 0"),
           ("mode", -1, "mode must be 0"), ("col_base", -1, "global columns"), ("col_base", 2 ** 31 - 5, "global columns"),
           ("nrows", 2 ** 25, "rows per call")]

    def merge(a, kcap=5, idx=bi.ptr(), val=bv.ptr()):
        return lib.gkmhip_knn_merge(0, a["K"], a["ld"], a["nrows"], a["ncols"], a["row_id"], a["col_base"], a["mode"], kcap,
                                    idx, val, None)

    def count(a, out=cnt.ptr()):
        return lib.gkmhip_pairs_count(0, a["K"], a["ld"], a["nrows"], a["ncols"], a["row_id"], a["col_base"], a["mode"], 0.5,
                                      out, None)

    def fill(a, offset=off.data_ptr(), cap=40, i=oi.ptr(), j=oj.ptr(), v=ov.ptr()):
        return lib.gkmhip_pairs_fill(0, a["K"], a["ld"], a["nrows"], a["ncols"], a["row_id"], a["col_base"], a["mode"], 0.5,
                                     offset, cap, i, j, v, None)

    def refused(rc, name, text):
        msg = lib.gkmhip_last_error().decode()
        assert rc == 2 and msg.startswith(name + ": ") and text in msg, (rc, msg)

    for key, value, text in bad:
        a = dict(good, **{key: value})
        refused(merge(a), "gkmhip_knn_merge", text)
        refused(count(a), "gkmhip_pairs_count", text)
        refused(fill(a), "gkmhip_pairs_fill", text)
    for kcap in (0, -1, 65):
        refused(merge(good, kcap=kcap), "gkmhip_knn_merge", "kcap must lie in 1..64")
    refused(merge(good, idx=None), "gkmhip_knn_merge", "NULL")
    refused(merge(good, val=None), "gkmhip_knn_merge", "NULL")
    refused(count(good, out=None), "gkmhip_pairs_count", "NULL")
    for kw in (dict(offset=None), dict(i=None), dict(j=None), dict(v=None)):
        refused(fill(good, **kw), "gkmhip_pairs_fill", "NULL")
    refused(fill(good, cap=-1), "gkmhip_pairs_fill", "capacity must not be negative")
    torch.cuda.synchronize()
    assert (bi.host() == -1).all() and np.isnan(bv.host()).all() and (cnt.host() == -5).all()
    assert (oi.host() == SENT_I).all() and (oj.host() == SENT_I).all() and (ov.host() == SENT_F).all()
    for g in (bi, bv, cnt, oi, oj, ov):
        assert g.guards_intact()
    assert blk.unchanged()
    # nothing to do is no error and writes nothing either
    assert merge(dict(good, nrows=0)) == 0 and merge(dict(good, ncols=0)) == 0 and fill(dict(good, nrows=0)) == 0
    assert count(dict(good, nrows=0)) == 0
    torch.cuda.synchronize()
    assert (bi.host() == -1).all() and (cnt.host() == -5).all() and (oi.host() == SENT_I).all()
    # the Python wrappers raise with the same message
    with pytest.raises(dv.GkmError, match="gkmhip_knn_merge failed \\(2\\): gkmhip_knn_merge: kcap must lie in 1..64"):
        dv.knn_merge(0, blk.ptr(), blk.ld, 4, 10, blk.d_id.data_ptr(), 0, 0, 65, bi.ptr(), bv.ptr())
