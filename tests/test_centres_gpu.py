"""The shift-record kernels' counter-free counting loop (gkm_bitslice.h window_group_any_centres; k_gram_bitslice PK = 6, 7) on
the GPU, at the pairs the existing GPU files leave thin for this form.  tests/test_crossings_gpu.py,
tests/test_shift_records_gpu.py, tests/test_same_length_sweep_gpu.py and tests/test_rider_parity_gpu.py already run the new
loop against kernel code 3, k_gram_direct and the oracle for (11,3), (10,3), (12,4), (5,1) and (8,0); added here:

    (L, d)   length  rows  variant
    (6, 3)   300 bp  70    PK 7: THREE count planes with bias beta = 1 -- the comparison's AND over the planes between plane 0 and
                           the top one is a single plane, and the carry-in of one enters each group's own column sum
    (12, 5)  300 bp  70    PK 6: the d = 5 instantiation (bias 1 at four planes; one wave per SIMD by its launch bounds)

on iid input and on dense-hit input (tests/test_shift_records_gpu.py _dense).  Dense input is where this form differs from a
stepped counter: centre windows one and two below the threshold whose group is flagged only through an off-centre window.

Per case, input and weighting (t = 4, 2), as tests/test_crossings_gpu.py: KERNEL_BITSLICE (the new loop) against
KERNEL_BITSLICE_GROUPS (kernel code 3: PK = 4 / 5, window_group_any_grouped with its stepped counter) and KERNEL_DIRECT, bit
for bit in the integer profiles of the lower triangle and in the raw values; and against the CPU oracle on rows 31, 64, 65,
67, 69.  The variant that ran is read back (gkmhip_last_variant through _launch)."""
import numpy as np
import pytest

from tests import same_length_cases as S
from tests.test_rider_parity_gpu import _oracle, _seqs
from tests.test_same_length_sweep_gpu import GROUPS_OF, SAME, _oracle_rows
from tests.test_shift_records_gpu import _dense, _launch

pytestmark = pytest.mark.gpu

CASES = [S.Case(6, 3, 300, 70, 7, True), S.Case(12, 5, 300, 70, 6, False)]


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def test_the_cases_are_what_the_plan_takes():
    """(6,3) and (12,5) at 300 bp are rows of the shared case table: riders and shift records / shift records alone"""
    for c in CASES:
        assert c in S.AT_300, c


@pytest.mark.parametrize("t", [4, 2])
@pytest.mark.parametrize("kind", ["dense", "iid"])
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_centres_loop_against_group_records_direct_and_oracle(dev, case, kind, t):
    L, d, n = case.L, case.d, case.n
    params = (t, L, L - d, d)
    seed = 9000 + 100 * L + 10 * d + case.length
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
    P, G, _ = _oracle(seqs, ("centres", kind, L, d, case.length), t, L, L - d, d, rows, threads=8)
    assert P.any()
    for a in rows:
        assert np.array_equal(Ps[a, :a + 1], P[a, :a + 1]), a
        assert np.array_equal(Gs[a, :a + 1], G[a, :a + 1]), a
