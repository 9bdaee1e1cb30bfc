"""Every same-length variant of k_gram_bitslice (PK = 4, 5 group records, 6, 7 shift records) on the GPU, over the table
of tests/same_length_cases.py: all 43 instantiated (L, d) pairs at 300 bp, the (11, 5) and multi-lane launches where the
LDS budget sends plain KERNEL_BITSLICE back to group records, rows of one to six lanes at both edges of their length band,
and the first length outside a band, which must take the several-pieces variants.  tests/test_same_length_plan_host.py
proves on the CPU that each row reaches the variant it names; here `last_variant()` must say the same.

Per case and weighting (t = 4, 2) three launches -- KERNEL_BITSLICE, KERNEL_BITSLICE_GROUPS, KERNEL_DIRECT -- must agree
bit for bit in the integer profiles of the lower triangle, the raw values (upper triangle untouched) and, bit-sliced
against general, the normalised matrix.  The independent reference is the CPU oracle: for one-lane rows (n = 70) on rows
31 (a resident of the first tile), 64 and 65 (the riders where there are any), 67 (a resident of the short second tile)
and 69 (the last) against all their columns, for multi-lane rows (n <= 35) on the whole triangle.  Oracle time per case on
the CPU, measured on one core: 0.25-0.5 s for the five rows of a 70 x 300 bp case, 2.3-3.4 s for a whole multi-lane
triangle (35 x 629 bp ... 12 x 2 047 bp); the rows are dealt to eight threads.

Dense-hit inputs (tests/test_shift_records_gpu.py _dense) repeat the multi-lane and fallback cases with records that carry
both groups and many bit rows; four cases go through the column-range launch and the cross kernel (full rows plus the
diagonal band) as well."""
import numpy as np
import pytest

from tests import same_length_cases as S
from tests.test_rider_parity_gpu import _oracle, _seqs
from tests.test_shift_records_gpu import _dense, _launch

pytestmark = pytest.mark.gpu

SAME, PACKED, PACKED128 = "k_gram_bitslice<same length>", "k_gram_bitslice<packed>", "k_gram_bitslice<packed,128>"
GROUPS_OF = {6: 4, 7: 5}      # what KERNEL_BITSLICE_GROUPS runs where plain KERNEL_BITSLICE takes shift records


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def _name(pk):
    return PACKED if pk == 1 else PACKED128 if pk == 2 else SAME


def _input(case, kind):
    seed = 1000 * case.L + 100 * case.d + case.length
    return _seqs(case.n, case.length, seed) if kind == "iid" else _dense(case.n, case.length, case.L, seed)


def _oracle_rows(case):
    """The rows whose oracle profiles a case is checked against (None: all)"""
    return None if case.length > 320 else [31, 64, 65, 67, 69]


def _reference(case, seqs, kind, t):
    """(rows, P, G): the oracle's profiles and raw values under kernel type t on the chosen rows, all their columns"""
    L, d = case.L, case.d
    rows = _oracle_rows(case)
    P, G, _ = _oracle(seqs, ("sweep", kind, case.length, case.n), t, L, L - d, d, rows, threads=8)
    return (np.arange(case.n) if rows is None else np.asarray(rows)), P, G


def _sweep(dev, case, t, kind):
    L, d, n = case.L, case.d, case.n
    params = (t, L, L - d, d)
    seqs = _input(case, kind)
    Ps, Gs, rs, name_s, pk_s, Ks = _launch(dev, seqs, params, dev.KERNEL_BITSLICE, want_k=True)
    Pg, Gg, rg, name_g, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS)
    Pd, Gd, rd, name_d, pk_d, Kd = _launch(dev, seqs, params, dev.KERNEL_DIRECT, want_k=True)
    print("%s t=%d %s: KERNEL_BITSLICE -> %s PK %d riders %d, KERNEL_BITSLICE_GROUPS -> PK %d" %
          (S.case_id(case), t, kind, name_s, pk_s, rs, pk_g))
    assert (name_s, pk_s, rs > 0) == (_name(case.pk), case.pk, case.riders)
    assert (name_g, pk_g, rg) == (name_s, GROUPS_OF.get(case.pk, case.pk), rs)
    assert (name_d, pk_d, rd) == ("k_gram_direct", 0, 0)
    if case.riders:
        assert rs == 2                                               # rows 64 and 65
    il = np.tril_indices(n)
    assert np.array_equal(Ps[il], Pd[il]) and np.array_equal(Pg[il], Pd[il])
    assert np.array_equal(Gs, Gd) and np.array_equal(Gg, Gd)
    assert (np.triu(Gs, 1) == 0).all()
    assert (np.diag(Ks) == 1.0).all() and np.array_equal(Ks, Kd) and (np.triu(Ks, 1) == 0).all()
    rows, P, G = _reference(case, seqs, kind, t)
    for a in rows:
        assert np.array_equal(Ps[a, :a + 1], P[a, :a + 1]), a
        assert np.array_equal(Gs[a, :a + 1], G[a, :a + 1]), a
    return seqs, Gd, Kd


@pytest.mark.parametrize("t", [4, 2])
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_sweep(dev, case, t):
    _sweep(dev, case, t, "iid")


@pytest.mark.parametrize("t", [4, 2])
@pytest.mark.parametrize("case", S.DENSE_CASES, ids=S.case_id)
def test_sweep_dense_hits(dev, case, t):
    _sweep(dev, case, t, "dense")


@pytest.mark.parametrize("t", [4, 2])
@pytest.mark.parametrize("case", S.MODE_CASES, ids=S.case_id)
def test_launch_modes(dev, case, t):
    """The column-range launch over a column window that ends inside the first tile's rows and one that starts inside them,
    and the cross kernel (every column for a row list with a jump, self norms from the diagonal band): every cell against
    the symmetric completion of the full run, which _sweep has just held against the oracle."""
    L, d, n = case.L, case.d, case.n
    params = (t, L, L - d, d)
    kind = "dense" if case in S.DENSE_CASES else "iid"
    seqs, G, K = _sweep(dev, case, t, kind)
    full = np.tril(G) + np.tril(G, -1).T
    Ksym = np.tril(K) + np.tril(K, -1).T
    first = 64 if n == 70 else 64 // S.lanes_of(L, case.length)      # residents of the first tile
    every = np.arange(n, dtype=np.int32)
    for rows, c0, c1 in ((every, 3, first - 5), (every, first - 3, n), (every[2:n - 1], 1, n - 1)):
        _, Bs, rs, name, pk = _launch(dev, seqs, params, dev.KERNEL_BITSLICE, (rows, c0, c1))
        _, Bg, rg, _, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS, (rows, c0, c1))
        assert name == SAME and pk_g == GROUPS_OF.get(pk, pk) and rs == rg
        if len(rows) == n:      # (the same rows as the triangle: the same packing, whatever the columns)
            assert (pk, rs > 0) == (case.pk, case.riders)
        assert np.array_equal(Bs, full[rows][:, c0:c1]) and np.array_equal(Bs, Bg)
    rows = np.delete(every, [0, n // 2])      # still more rows than a tile holds: riders where the triangle has them
    for kern in (dev.KERNEL_BITSLICE, dev.KERNEL_BITSLICE_GROUPS):
        x = dev.cross_kernel(seqs, rows, *params, kernel=kern)
        want = case.pk if kern == dev.KERNEL_BITSLICE else GROUPS_OF.get(case.pk, case.pk)
        assert (x["kernel"], x["variant"]) == (SAME, want)
        got = x["K"].cpu().numpy()
        for i, a in enumerate(x["rows"]):
            assert np.array_equal(got[i], Ksym[a]), a
