"""The shift-record kernels' counting loop with SHIFT-SHARED centre trees (gkm_bitslice.h window_group_any_centres, SHIFTED =
true; k_gram_bitslice PK = 6, 7: the second centre's own words taken as the first centre's sum one bit row on) on the GPU, at the
smallest same-length problems that reach each path of the loop:

    70 rows x 300 bp   two tiles, 2 riders in bit rows 30 and 31: PK = 7
    70 rows x 281 bp   the lower edge of the one-lane band, riders: PK = 7
    70 rows x 310 bp   no riders: PK = 6, and the resident reaches bit row 31 -- the row the shifted planes lose
    40 rows x 600 bp   two lanes per row: PK = 6

for (L, d) = (11, 3) and (10, 3) (bias 0 with one head word per centre; bias 1 with none), kernel types 4 (weighted) and 0, on a
seeded iid input and on a dense-hit input built from tests/dense_inputs.py (tests/test_shift_records_gpu._dense: centre counts
on and either side of the threshold in most bit rows of both groups).  The two further pairs that take the form, (10, 2) and
(11, 4), run one dense case each at 300 bp.  The variant and the riders are read back from each launch.

Per case: KERNEL_BITSLICE (the new loop) against KERNEL_BITSLICE_GROUPS (kernel code 3: PK = 4 / 5, the stepped counter,
untouched) and KERNEL_DIRECT (k_gram_direct), bit for bit in the int32 profiles of the lower triangle and in the raw matrix; and
against the CPU oracle on the whole lower triangle."""
import numpy as np
import pytest

from tests import same_length_cases as S
from tests.test_rider_packing import probe  # noqa: F401  (the fixture)
from tests.test_rider_parity_gpu import _oracle, _seqs
from tests.test_same_length_plan_host import plan
from tests.test_same_length_sweep_gpu import GROUPS_OF, SAME
from tests.test_shift_records_gpu import _dense, _launch
from tests.test_shift_shared_trees import TAKEN

pytestmark = pytest.mark.gpu

REQUIRED = [(11, 3), (10, 3)]
FURTHER = sorted(set(TAKEN) - set(REQUIRED))
# (length, rows, PK, riders)
SHAPES = [(300, 70, 7, 2), (281, 70, 7, 2), (310, 70, 6, 0), (600, 40, 6, 0)]
_INPUTS = {}


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def _input(kind, n, length, L):
    key = (kind, n, length, L if kind == "dense" else 0)
    if key not in _INPUTS:
        _INPUTS[key] = _seqs(n, length, 2000 + length) if kind == "iid" else _dense(n, length, L, 20 + length % 7)
    return key, _INPUTS[key]


def test_the_cases_are_what_the_plan_takes(probe):
    """the launch plan restated on the CPU (tests/test_same_length_plan_host.py) takes the variants asserted below from the
    launches themselves, and the lengths lie where this file says: one lane per row up to 310 bp, two at 600"""
    assert FURTHER == [(10, 2), (11, 4)]
    for L, d in TAKEN:
        assert [S.lanes_of(L, n) for n in (281, 300, 310, 600)] == [1, 1, 1, 2] and S.lanes_of(L, 280) == 0
        for length, n, pk, riders in SHAPES:
            assert plan(probe, L, d, length, n)[:2] == (pk, riders), (L, d, length)


def _check(dev, t, L, d, length, n, pk, riders, kind):
    params = (t, L, L - 4, d)
    key, seqs = _input(kind, n, length, L)
    Ps, Gs, rs, name_s, pk_s = _launch(dev, seqs, params, dev.KERNEL_BITSLICE)
    Pg, Gg, rg, name_g, pk_g = _launch(dev, seqs, params, dev.KERNEL_BITSLICE_GROUPS)
    Pd, Gd, rd, name_d, pk_d = _launch(dev, seqs, params, dev.KERNEL_DIRECT)
    assert (name_s, pk_s, rs) == (SAME, pk, riders)
    assert (name_g, pk_g, rg) == (SAME, GROUPS_OF[pk], riders)
    assert (name_d, pk_d, rd) == ("k_gram_direct", 0, 0)
    il = np.tril_indices(n)
    assert np.array_equal(Ps[il], Pg[il]) and np.array_equal(Ps[il], Pd[il])
    assert np.array_equal(Gs, Gg) and np.array_equal(Gs, Gd) and (np.triu(Gs, 1) == 0).all()
    P, G, _ = _oracle(seqs, ("shift-shared",) + key, *params, threads=8)
    assert all(P[..., m].any() for m in range(d + 1))      # hits at every mismatch count 0 .. d
    assert np.array_equal(Ps[il], P[il]) and np.array_equal(Gs[il], G[il])


@pytest.mark.parametrize("kind", ["iid", "dense"])
@pytest.mark.parametrize("t", [4, 0])
@pytest.mark.parametrize("length,n,pk,riders", SHAPES, ids=["300bp-n70", "281bp-n70", "310bp-n70", "600bp-n40"])
@pytest.mark.parametrize("L,d", REQUIRED)
def test_shift_shared_against_group_records_direct_and_oracle(dev, L, d, length, n, pk, riders, t, kind):
    _check(dev, t, L, d, length, n, pk, riders, kind)


@pytest.mark.parametrize("L,d", FURTHER)
def test_further_pairs_that_take_the_form(dev, L, d):
    _check(dev, 4, L, d, 300, 70, 7, 2, "dense")
