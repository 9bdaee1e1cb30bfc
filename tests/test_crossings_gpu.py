"""The shift-record kernels' counting loop that groups hits from top-plane crossings (gkm_bitslice.h
window_group_any_crossings; k_gram_bitslice PK = 6, 7) on the GPU, at the shapes where that loop can go wrong and
tests/test_same_length_sweep_gpu.py is thin:

    (L, d)   length  rows  variant
    (11, 3)  300 bp  70    PK 7: riders, two tiles (the headline's kernel)
    (10, 3)  600 bp  35    PK 6: two lanes per row, bias beta = 1 (the carry-in of the first window's column sum)
    (12, 4)  300 bp  70    PK 6
    (5, 1)   300 bp  70    PK 7: three count planes (one step is four ops, not six)
    (8, 0)   300 bp  70    PK 7: d = 0, the threshold is "every base matches"

on iid input and on dense-hit input (tests/test_shift_records_gpu.py _dense), which makes the top plane cross up and down
repeatedly inside one group of five words and carries a set top plane over the group boundary -- the two places where an OR
built from crossings differs from an OR of per-word planes if a crossing is dropped or taken twice.

Per case, input and weighting (t = 4, 2): KERNEL_BITSLICE (the new loop) against KERNEL_BITSLICE_GROUPS (kernel code 3:
PK = 4 / 5, window_group_any_grouped as before) and KERNEL_DIRECT, bit for bit in the integer profiles of the lower triangle
and in the raw values; and against the CPU oracle, on the rows tests/test_same_length_sweep_gpu.py's _oracle_rows uses for
one-lane cases (31, 64, 65, 67, 69) and on the whole triangle for the 35-row case."""
import numpy as np
import pytest

from tests import same_length_cases as S
from tests.test_rider_parity_gpu import _oracle, _seqs
from tests.test_same_length_sweep_gpu import GROUPS_OF, SAME, _oracle_rows
from tests.test_shift_records_gpu import _dense, _launch

pytestmark = pytest.mark.gpu

CASES = [S.Case(11, 3, 300, 70, 7, True), S.Case(10, 3, 600, 35, 6, False), S.Case(12, 4, 300, 70, 6, False),
         S.Case(5, 1, 300, 70, 7, True), S.Case(8, 0, 300, 70, 7, True)]


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


@pytest.mark.parametrize("t", [4, 2])
@pytest.mark.parametrize("kind", ["dense", "iid"])
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_crossings_loop_against_group_records_direct_and_oracle(dev, case, kind, t):
    L, d, n = case.L, case.d, case.n
    params = (t, L, L - d, d)
    seed = 7000 + 100 * L + 10 * d + case.length
    seqs = _seqs(n, case.length, seed) if kind == "iid" else _dense(n, case.length, L, seed)
    Ps, Gs, rs, name_s, pk_s = _launch(dev, seqs, params, dev.KERNEL_BITSLICE)
    Pg, Gg, rg, name_g, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS)
    Pd, Gd, rd, name_d, pk_d = _launch(dev, seqs, params, dev.KERNEL_DIRECT)
    # the launches took the variants this file is about: the new loop, and the loop it is held against
    assert (name_s, pk_s, rs > 0) == (SAME, case.pk, case.riders)
    assert (name_g, pk_g, rg) == (SAME, GROUPS_OF[case.pk], rs)
    assert (name_d, pk_d, rd) == ("k_gram_direct", 0, 0)
    il = np.tril_indices(n)
    assert np.array_equal(Ps[il], Pg[il]) and np.array_equal(Ps[il], Pd[il])
    assert np.array_equal(Gs, Gg) and np.array_equal(Gs, Gd) and (np.triu(Gs, 1) == 0).all()
    rows = _oracle_rows(case)
    P, G, _ = _oracle(seqs, ("crossings", kind, L, d, case.length), t, L, L - d, d, rows, threads=8)
    assert P.any()
    for a in (range(n) if rows is None else rows):
        assert np.array_equal(Ps[a, :a + 1], P[a, :a + 1]), a
        assert np.array_equal(Gs[a, :a + 1], G[a, :a + 1]), a
