"""Riders of the same-length Gram kernel on the GPU (k_gram_bitslice PK = 5, gkm_pack.h RIDER_B0) against the CPU oracle:
the lower triangle of the integer profiles, of the raw values and of the normalised matrix, bit for bit.  The shapes are
the smallest at which the path can go wrong: 64 residents + 2 riders + a short second tile (n = 70), one row left over
(n = 67), 600-bp rows that take two lanes each and leave no room for riders, row subsets with a jump in both output
placements and as packed slabs, 330-bp rows (which share lanes: the several-pieces variant), and one ragged problem that
must stay on the several-pieces variant.  Whether a launch carried riders is asserted from `last_riders()` / the result's
`riders`: the kernel's name is the same either way and so is the matrix."""
import ctypes

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


_ORACLE = {}


def _oracle(seqs, key, t, L, k, d, rows=None, threads=1):
    """Profiles, raw values (sum_m c_m P_m in ascending m from 0.0, libgkm.c:576-582) and K = G / (sq_a sq_j) of the lower
    triangle (of the given rows only: K then stays unset), computed once per (sequences, parameters) and shared.
    threads > 1: that many rows at a time."""
    if (key, t, L, k, d) in _ORACLE:
        return _ORACLE[(key, t, L, k, d)]
    from oracle import oracle as O
    n = len(seqs)
    opt = O.make_opt(t, L, k, d)
    c = O.mismatch_weights(t, L, k)[: d + 1]
    P = np.zeros((n, n, d + 1), dtype=np.int32)
    vp = ctypes.c_void_p
    lib = O.lib()

    def one_row(a):
        prof = np.zeros(d + 1, dtype=np.int32)
        for j in range(a + 1):
            lib.gkmo_profile(ctypes.byref(opt), seqs[a].ctypes.data_as(vp), len(seqs[a]), seqs[j].ctypes.data_as(vp),
                             len(seqs[j]), prof.ctypes.data_as(vp))
            P[a, j] = prof

    todo = list(range(n) if rows is None else rows)
    if threads > 1:      # (gkmo_profile keeps no state between calls, and the call releases the interpreter lock)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one_row, todo[::-1]))
    else:
        for a in todo:
            one_row(a)
    G = np.zeros((n, n))
    for m in range(d + 1):
        G += c[m] * P[:, :, m].astype(np.float64)
    G = np.tril(G)
    K = None
    if rows is None:
        sq = np.sqrt(np.diag(G))
        K = np.tril(G / (sq[:, None] * sq[None, :]))
        np.fill_diagonal(K, 1.0)
    for x in (P, G, K):
        if x is not None:
            x.setflags(write=False)
    _ORACLE[(key, t, L, k, d)] = (P, G, K)
    return P, G, K


def _seqs(n, length, seed):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, 4, length).astype(np.uint8) for _ in range(n)]
    seqs[n - 2] = seqs[1].copy()           # a duplicate and a poly-A row among the last rows (the riders at n = 70, 67)
    seqs[n - 3][:] = 0
    return seqs


def _raw(dev, seqs, t, L, k, d, rows=None, local=False, packed=False):
    import torch
    n = len(seqs)
    ctx = dev.GramContext(t, L, k, d)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(seqs, stream)
        rows = np.arange(n, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
        if packed:
            off = np.zeros(len(rows), dtype=np.int64)
            np.cumsum(rows[:-1] + 1, out=off[1:])
            G = torch.zeros(int(off[-1] + rows[-1] + 1), dtype=torch.float64, device="cuda")
            ctx.gram_rows_packed(rows, G.data_ptr(), off, stream)
            torch.cuda.synchronize()
            G = G.cpu().numpy()
            return [G[off[i]:off[i] + rows[i] + 1] for i in range(len(rows))], ctx.last_riders()
        G = torch.zeros((len(rows) if local else n, n), dtype=torch.float64, device="cuda")
        ctx.gram_rows(rows, G.data_ptr(), n, None, 0, local, stream)
        torch.cuda.synchronize()
        return G.cpu().numpy(), ctx.last_riders()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [70, 67])
@pytest.mark.parametrize("t,L,k,d", [(4, 11, 7, 3), (2, 11, 7, 3), (4, 10, 6, 3), (2, 10, 6, 3)])
def test_riders_300_bp(dev, n, t, L, k, d):
    seqs = _seqs(n, 300, 1000 + n)
    P, G, K = _oracle(seqs, ("u300", n), t, L, k, d)
    res = dev.gram_matrix(seqs, t, L, k, d, want_profiles=True, kernel=dev.KERNEL_BITSLICE)
    assert res["kernel"] == "k_gram_bitslice<same length>" and res["riders"] == 2      # rows 64 and 65
    il = np.tril_indices(n)
    assert (res["P"].cpu().numpy()[il] == P[il]).all()
    raw, riders = _raw(dev, seqs, t, L, k, d)
    assert riders == 2
    assert (raw[il] == G[il]).all() and (np.triu(raw, 1) == 0).all()
    Kd = res["K"].cpu().numpy()
    assert (Kd[il] == K[il]).all() and (np.triu(Kd, 1) == 0).all()


def test_two_lane_residents_600_bp(dev):
    n, (t, L, k, d) = 35, (4, 10, 6, 3)
    seqs = _seqs(n, 600, 600)
    P, G, K = _oracle(seqs, ("u600", n), t, L, k, d)
    res = dev.gram_matrix(seqs, t, L, k, d, want_profiles=True, kernel=dev.KERNEL_BITSLICE)
    assert res["kernel"] == "k_gram_bitslice<same length>" and res["riders"] == 0
    il = np.tril_indices(n)
    assert (res["P"].cpu().numpy()[il] == P[il]).all() and (res["K"].cpu().numpy()[il] == K[il]).all()


def test_330_bp_rows_share_lanes_and_take_no_riders(dev):
    """330 bp at L = 11: 310 windows in a row's first lane, 10 in its second -- and the next row's first piece behind them
    in the same lane: several pieces per lane, so the several-pieces variant serves it and nothing rides."""
    n, (t, L, k, d) = 40, (4, 11, 7, 3)
    seqs = _seqs(n, 330, 330)
    P, G, K = _oracle(seqs, ("u330", n), t, L, k, d)
    res = dev.gram_matrix(seqs, t, L, k, d, want_profiles=True, kernel=dev.KERNEL_BITSLICE)
    assert res["kernel"].startswith("k_gram_bitslice<packed") and res["riders"] == 0
    il = np.tril_indices(n)
    assert (res["P"].cpu().numpy()[il] == P[il]).all() and (res["K"].cpu().numpy()[il] == K[il]).all()


def test_row_subset_with_a_jump(dev):
    """Rows 0..39 and 100..129 of 130 (70 rows; a jump of 61 closes no tile: 64 residents, rows 124 and 125 ride, 4 left),
    rows 0..69 and 100..129 (riders 64 and 65, the next tile reaches across the jump), and rows 0..9 and 100..129 (no tile
    fills up: nothing rides): both output placements and the packed slabs give the reference values and touch nothing
    else.  Reference: the oracle for the first list, the general kernel k_gram_direct for the others (5 950 pairs on the
    CPU would take longer than the rest of this file)."""
    n, (t, L, k, d) = 130, (4, 11, 7, 3)
    seqs = _seqs(n, 300, 130)
    rows = np.concatenate([np.arange(0, 40), np.arange(100, 130)]).astype(np.int32)
    _, G, _ = _oracle(seqs, ("u300", n), t, L, k, d, rows)
    loc, r0 = _raw(dev, seqs, t, L, k, d, rows, local=True)
    glob, r1 = _raw(dev, seqs, t, L, k, d, rows, local=False)
    slabs, r2 = _raw(dev, seqs, t, L, k, d, rows, packed=True)
    assert (r0, r1, r2) == (2, 2, 2)
    for i, a in enumerate(rows):
        assert (loc[i, :a + 1] == G[a, :a + 1]).all() and (loc[i, a + 1:] == 0).all()
        assert (glob[a, :a + 1] == G[a, :a + 1]).all() and (glob[a, a + 1:] == 0).all()
        assert (slabs[i] == G[a, :a + 1]).all()
    assert (glob[np.setdiff1d(np.arange(n), rows)] == 0).all()
    import torch
    ctx = dev.GramContext(t, L, k, d)
    ctx.set_kernel(dev.KERNEL_DIRECT)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.set_sequences(seqs, stream)
    Gd = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    ctx.gram_rows(np.arange(n), Gd.data_ptr(), n, None, 0, False, stream)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_gram_direct" and ctx.last_riders() == 0
    ctx.close()
    Gd = Gd.cpu().numpy()
    assert (Gd[rows][:, :40] == G[rows][:, :40]).all()      # (the two references agree where both exist)
    for rows, riders in ((np.concatenate([np.arange(0, 70), np.arange(100, 130)]), 2),
                         (np.concatenate([np.arange(0, 10), np.arange(100, 130)]), 0)):
        rows = rows.astype(np.int32)
        loc, r0 = _raw(dev, seqs, t, L, k, d, rows, local=True)
        glob, r1 = _raw(dev, seqs, t, L, k, d, rows, local=False)
        slabs, r2 = _raw(dev, seqs, t, L, k, d, rows, packed=True)
        assert (r0, r1, r2) == (riders, riders, riders)
        for i, a in enumerate(rows):
            assert (loc[i, :a + 1] == Gd[a, :a + 1]).all() and (loc[i, a + 1:] == 0).all()
            assert (glob[a, :a + 1] == Gd[a, :a + 1]).all() and (glob[a, a + 1:] == 0).all()
            assert (slabs[i] == Gd[a, :a + 1]).all()
        assert (glob[np.setdiff1d(np.arange(n), rows)] == 0).all()


def test_ragged_lengths_stay_on_the_several_pieces_variant(dev):
    t, L, k, d = 4, 11, 7, 3
    seqs = helpers.synth_codes(35, 35, 300, (150, 600))
    n = len(seqs)
    P, G, K = _oracle(seqs, ("ragged", n), t, L, k, d)
    res = dev.gram_matrix(seqs, t, L, k, d, want_profiles=True, kernel=dev.KERNEL_BITSLICE)
    assert res["kernel"].startswith("k_gram_bitslice<packed") and res["riders"] == 0
    il = np.tril_indices(n)
    assert (res["P"].cpu().numpy()[il] == P[il]).all() and (res["K"].cpu().numpy()[il] == K[il]).all()
