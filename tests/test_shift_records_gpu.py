"""Shift records on the GPU (k_gram_bitslice PK = 6 and 7: one hit compaction per shift, three-word records, the group taken
by the trip -- gkm_bitslice.h shift_record_visit) against the CPU oracle and against the explicit group-record kernel
(device.KERNEL_BITSLICE_GROUPS: PK = 4 and 5, untouched): the integer profiles and the raw Gram values of the lower
triangle, bit for bit.

Shapes, the smallest at which the path can go wrong: 70 rows of 300 bp (64 residents, 2 riders, a short second tile: PK = 7),
40 rows of 600 bp (two lanes per row, two profile copies, no riders: PK = 6), 5 rows of T = L and of T = L + 1 (one window,
two windows: every shift wraps; such rows share lanes and stay on the several-pieces variant under either kernel code).  Dense-hit sets -- homopolymers, two-letter and short-period repeats, copies -- make both
groups of a lane hit in the same shift, give records many bit rows and fill the list of 128 records, so that the re-push of
all three words and the trip check that now runs once per shift are exercised; a two-letter set is repeated through the
column-range launch that scoring uses."""
import numpy as np
import pytest

from tests import dense_inputs as D
from tests.test_rider_parity_gpu import _oracle, _seqs

pytestmark = pytest.mark.gpu

SHAPES = [(4, 11, 7, 3), (2, 11, 7, 3), (4, 10, 6, 3), (2, 10, 6, 3)]       # (11,3) and (10,3), weighted and unweighted
NAME = "k_gram_bitslice<same length>"


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def _launch(dev, seqs, params, kernel, block=None, want_k=False):
    """One Gram launch with the given kernel code -> (profiles or None, raw values, riders, kernel name, variant: the
    kernel's PK, 0 for the general kernel).  block = (rows, c0, c1): the column-range launch, raw values [len(rows),
    c1 - c0] and no profiles.  want_k (triangle only): a sixth value, the normalised matrix of the raw values."""
    import torch
    t, L, k, d = params
    n = len(seqs)
    ctx = dev.GramContext(t, L, k, d)
    try:
        ctx.set_kernel(kernel)
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(seqs, stream)
        if block is not None:
            rows, c0, c1 = block
            G = torch.full((len(rows), c1 - c0), -7.25, dtype=torch.float64, device="cuda")
            ctx.gram_block(rows, c0, c1, G.data_ptr(), c1 - c0, stream)
            torch.cuda.synchronize()
            return None, G.cpu().numpy(), ctx.last_riders(), ctx.last_kernel_name(), ctx.last_variant()
        G = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        P = torch.zeros((n, n, d + 1), dtype=torch.int32, device="cuda")
        ctx.gram_rows(np.arange(n), G.data_ptr(), n, P.data_ptr(), n, False, stream)
        torch.cuda.synchronize()
        out = (P.cpu().numpy(), G.cpu().numpy(), ctx.last_riders(), ctx.last_kernel_name(), ctx.last_variant())
        if want_k:
            sq = torch.zeros(n, dtype=torch.float64, device="cuda")
            ctx.normalize(G.data_ptr(), n, sq.data_ptr(), False, stream)
            torch.cuda.synchronize()
            out += (G.cpu().numpy(),)
        return out
    finally:
        ctx.close()


def _check(dev, seqs, key, params, riders, name=NAME):
    """shift records == oracle == group records on the lower triangle; -> nothing"""
    P, G, _ = _oracle(seqs, key, *params)
    n = len(seqs)
    il = np.tril_indices(n)
    Ps, Gs, rs, name_s, pk_s = _launch(dev, seqs, params, dev.KERNEL_BITSLICE)
    Pg, Gg, rg, name_g, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS)
    assert name_s == name and name_g == name
    assert (pk_s, pk_g) == ((1, 1) if name != NAME else (7, 5) if riders else (6, 4))
    assert (rs > 0) == riders and rs == rg
    assert (Ps[il] == P[il]).all() and (Gs[il] == G[il]).all() and (np.triu(Gs, 1) == 0).all()
    assert (Pg[il] == P[il]).all() and (Gg[il] == G[il]).all()
    assert np.array_equal(Ps[il], Pg[il]) and np.array_equal(Gs, Gg)


def _dense(n, length, L, seed):
    """n sequences of one length on which most window pairs are hits: homopolymers, two-letter and period-3 repeats (a
    lane's windows then hit in both groups of a shift and in many bit rows at once), spliced low-complexity stretches,
    copies of earlier rows; the same kinds again among the last rows, where the riders of a 300-bp tile are."""
    kinds = [D.homopolymer(D.A, length), D.repeat((D.A, D.T), length), D.repeat((D.A, D.C), length),
             D.repeat((D.C, D.G), length), D.repeat(D.unit_of(3, seed), length), D.homopolymer(D.C, length),
             D.repeat(D.unit_of(L, seed), length)]
    out = []
    for i in range(n):
        if i % 3 == 0:
            out.append(kinds[(i // 3) % len(kinds)].copy())
        elif i % 3 == 1:
            out.append(D.spliced(length, L, seed + i))
        else:
            out.append(D.substituted(out[i - 2], 1 + i % 3, L, seed + i))
    return [np.ascontiguousarray(x, dtype=np.uint8) for x in out]


@pytest.mark.parametrize("t,L,k,d", SHAPES)
def test_300_bp_with_riders(dev, t, L, k, d):
    _check(dev, _seqs(70, 300, 1070), ("u300", 70), (t, L, k, d), riders=True)


@pytest.mark.parametrize("t,L,k,d", SHAPES)
def test_600_bp_without_riders(dev, t, L, k, d):
    _check(dev, _seqs(40, 600, 640), ("u600s", 40), (t, L, k, d), riders=False)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("t,L,k,d", SHAPES)
def test_shortest_sequences(dev, t, L, k, d, extra):
    """Rows of one or two windows share lanes, so the several-pieces variant serves both kernel codes: the launch choice
    must not send such a same-length problem to the shift-record variants, which want one resident piece per lane."""
    seqs = _seqs(5, L + extra, 50 + L + extra)
    _check(dev, seqs, ("short", L + extra), (t, L, k, d), riders=False, name="k_gram_bitslice<packed>")


@pytest.mark.parametrize("t,L,k,d", SHAPES)
def test_dense_hits_300_bp_with_riders(dev, t, L, k, d):
    _check(dev, _dense(70, 300, L, 7), ("dense300", L), (t, L, k, d), riders=True)


@pytest.mark.parametrize("t,L,k,d", [(4, 11, 7, 3), (2, 10, 6, 3)])
def test_dense_hits_600_bp(dev, t, L, k, d):
    _check(dev, _dense(40, 600, L, 11), ("dense600", L), (t, L, k, d), riders=False)


@pytest.mark.parametrize("t,L,k,d", [(4, 11, 7, 3), (2, 10, 6, 3)])
def test_dense_hits_through_the_column_range_launch(dev, t, L, k, d):
    """Rows 0 .. 69 (riders) against the columns [3, 70) and rows 5 .. 30 (no tile fills up) against [0, 41): every
    cell of the block, upper triangle included, equals the oracle's symmetric value and the group-record kernel's."""
    seqs = _dense(70, 300, L, 7)
    P, G, _ = _oracle(seqs, ("dense300", L), t, L, k, d)
    full = np.tril(G) + np.tril(G, -1).T
    for rows, c0, c1, riders in ((np.arange(70, dtype=np.int32), 3, 70, True), (np.arange(5, 31, dtype=np.int32), 0, 41, False)):
        _, Bs, rs, name, pk_s = _launch(dev, seqs, (t, L, k, d), dev.KERNEL_BITSLICE, (rows, c0, c1))
        _, Bg, rg, _, pk_g = _launch(dev, seqs, (t, L, k, d), dev.KERNEL_BITSLICE_GROUPS, (rows, c0, c1))
        assert name == NAME and (rs > 0) == riders and rs == rg and (pk_s, pk_g) == ((7, 5) if riders else (6, 4))
        assert np.array_equal(Bs, full[rows][:, c0:c1]) and np.array_equal(Bs, Bg)
