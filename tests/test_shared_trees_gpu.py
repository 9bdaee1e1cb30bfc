"""The shift-record kernels' counting loop with shared centre trees (gkm_bitslice.h window_group_any_centres, SHARED = true;
k_gram_bitslice PK = 6, 7) on the GPU, at the smallest problems that run the very kernels the benchmark runs, for EVERY (L, d)
whose threshold is the top plane -- the pairs for which the loop exists (tests/test_group_any.TOP_PLANE; all 15 have a
bit-sliced instantiation):

    70 rows x 300 bp   64 residents, 2 riders at an equal tile count, a short second tile: PK = 7 (L = 12 has no rider variant
                       and takes PK = 6, as tests/same_length_cases.AT_300 lists it)
    40 rows x 600 bp   two lanes per row, no riders: PK = 6

The variant and the riders are read back from the launch (gkmhip_last_variant, gkmhip_last_riders through _launch).

Input: every row is a mutated copy of one ancestor (a substitution at each base with a probability of its own between 3 % and
25 %), so any two rows are homologous along the main diagonal with 6 % to 44 % mismatches: windows with 0 .. 2 d mismatches, hits
in most bit rows of both groups, and centre windows on both sides of the threshold next to each other -- the cases that the
shared sums and the folded top half adder decide (tests/test_shared_trees.py holds them one by one on the CPU).

Per case: KERNEL_BITSLICE (the new loop) against KERNEL_BITSLICE_GROUPS (kernel code 3: PK = 4 / 5, the stepped counter,
untouched), bit for bit in the int32 profiles of the lower triangle and in the raw matrix; and against the CPU oracle on the
whole lower triangle (well under a second per case on the CPU)."""
import numpy as np
import pytest

from tests import same_length_cases as S
from tests.test_group_any import TOP_PLANE
from tests.test_rider_packing import probe  # noqa: F401  (the fixture)
from tests.test_rider_parity_gpu import _oracle
from tests.test_same_length_plan_host import plan
from tests.test_same_length_sweep_gpu import GROUPS_OF, SAME
from tests.test_shift_records_gpu import _launch

pytestmark = pytest.mark.gpu

PAIRS = sorted(TOP_PLANE)
SHAPES = [(300, 70), (600, 40)]
_INPUTS = {}


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def _mutated_copies(n, length):
    """n rows, each the same ancestor with substitutions at a rate of its own; rows n - 2 and n - 1 (riders' neighbours in the
    last tile at n = 70) are exact copies of rows 1 and 64, so that full-length identical pairs occur as well"""
    if (n, length) not in _INPUTS:
        rng = np.random.default_rng(1800 + length)
        anc = rng.integers(0, 4, length).astype(np.uint8)
        seqs = []
        for i in range(n):
            rate = 0.03 + 0.22 * ((i * 7) % 11) / 10.0
            sub = rng.random(length) < rate
            seqs.append(np.where(sub, (anc + rng.integers(1, 4, length)) & 3, anc).astype(np.uint8))
        seqs[n - 2] = seqs[1].copy()
        seqs[n - 1] = seqs[min(64, n - 3)].copy()
        _INPUTS[(n, length)] = seqs
    return _INPUTS[(n, length)]


def test_the_cases_are_what_the_plan_takes(probe):
    """every top-plane pair is in the device table, 300 bp keeps one lane per row and 600 bp two, and the launch plan restated
    on the CPU (tests/test_same_length_plan_host.py) takes the variants asserted below from the launches themselves"""
    assert len(PAIRS) == 15 and set(PAIRS) <= set(S.ALL_LD)
    for L, d in PAIRS:
        assert S.lanes_of(L, 300) == 1 and S.lanes_of(L, 600) == 2, (L, d)
        at300 = [c for c in S.AT_300 if (c.L, c.d) == (L, d)]
        assert len(at300) == 1 and (at300[0].pk, at300[0].riders) == ((7, True) if L <= 11 else (6, False))
        assert plan(probe, L, d, 300, 70)[:2] == ((7, 2) if L <= 11 else (6, 0)), (L, d)
        assert plan(probe, L, d, 600, 40)[:2] == (6, 0), (L, d)


@pytest.mark.parametrize("length,n", SHAPES, ids=["300bp-n70", "600bp-n40"])
@pytest.mark.parametrize("L,d", PAIRS)
def test_shared_trees_against_group_records_and_oracle(dev, L, d, length, n):
    t = 4
    params = (t, L, L - d, d)
    seqs = _mutated_copies(n, length)
    pk, riders = ((7, True) if L <= 11 else (6, False)) if length == 300 else (6, False)
    Ps, Gs, rs, name_s, pk_s = _launch(dev, seqs, params, dev.KERNEL_BITSLICE)
    Pg, Gg, rg, name_g, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS)
    assert (name_s, pk_s, rs) == (SAME, pk, 2 if riders else 0)
    assert (name_g, pk_g, rg) == (SAME, GROUPS_OF[pk], rs)
    il = np.tril_indices(n)
    assert np.array_equal(Ps[il], Pg[il])
    assert np.array_equal(Gs, Gg) and (np.triu(Gs, 1) == 0).all()
    P, G, _ = _oracle(seqs, ("mutated", length, n), t, L, L - d, d, threads=8)
    # the input does what it is for: hits at every mismatch count 0 .. d
    assert all(P[..., m].any() for m in range(d + 1))
    assert np.array_equal(Ps[il], P[il]) and np.array_equal(Gs[il], G[il])
