"""Which k_gram_bitslice variant a same-length launch takes, recomputed on the CPU for every row of
tests/same_length_cases.py: the packing through bitslice_cpu_probe.so (gkm_pack.h pack_rows and
same_length_packing_check, the functions gkm_gram.hip plan_bitslice calls) and the plan's own rules restated here -- wider
tiles where they are fewer, one resident piece per lane or the several-pieces variants, riders where whole rows fit and
L <= 11, shift records unless their longer hit list leaves the four LDS granules that group records stay inside.  The GPU
sweep (tests/test_same_length_sweep_gpu.py) asserts the same numbers from `last_variant()`; this file proves that the
table reaches the variants it claims, and that the bands of tests/same_length_cases.py are the packing's."""
import ctypes

import numpy as np
import pytest

from tests import helpers
from tests import same_length_cases as S
from tests.test_rider_packing import _consts, _pack, probe  # noqa: F401  (the fixture)

LDS_GRANULE = 1280
LDS_WAVE_BUDGET = 4 * LDS_GRANULE        # gkm_gram_bitslice.h BS_LDS_WAVE_BUDGET
POSTAB_PAD = 5


def static_lds(pk, d):
    """gkm_gram_bitslice.h bs_same_length_static_lds: profiles [d + 1][64, or 128 with riders], 128 hit records of two
    words (group records) or three (shift records), 64 rider tags"""
    riders, shift = pk in (5, 7), pk in (6, 7)
    return ((d + 1) * (128 if riders else 64) + (3 if shift else 2) * 128 + (64 if riders else 0)) * 4


def colpk_words(maxlen):
    return (maxlen + 15) // 16 + 1


def postab_words(maxlen, L):
    return (POSTAB_PAD + L - 1 + maxlen + POSTAB_PAD + 8 + 3) // 4


def dyn_lds(length, L):
    return (2 * colpk_words(length) + postab_words(length, L)) * 4


def has_riders_variant(L):
    """k_gram_bitslice PK = 5, 7 exist where a rider piece's windows fit its two bit rows: L - 1 <= RIDER_NB W - RIDER_W"""
    return L - 1 <= 2 * S.W - 10


def _tiles(probe, n, length, L, max_rows):
    rows = np.arange(n, dtype=np.int32)
    nwin = np.full(n, length - L + 1, dtype=np.int32)
    vp = ctypes.c_void_p
    return probe.packprobe_plan_tiles(rows.ctypes.data_as(vp), nwin.ctypes.data_as(vp), n, L, max_rows)


def plan(probe, L, d, length, n, groups=False):
    """plan_bitslice for n rows of one length in a triangular launch -> (PK, riders, one piece per lane)"""
    RW = _consts(probe)[2]
    rows = np.arange(n, dtype=np.int32)
    lay = _pack(probe, rows, length, L, 0)
    slots = 64 if lay["ntiles"] <= 1.04 * _tiles(probe, n, length, L, 128) else 128
    lanes = lay["pieces"][:, 0]
    shares = bool((lanes[1:] == lanes[:-1]).any())
    packed = slots != 64 or shares or lay["check"] != 0
    if packed:
        return (1 if slots == 64 else 2), 0, False
    pk, riders = 4, 0
    if has_riders_variant(L):
        withr = _pack(probe, rows, length, L, RW)
        if withr["nriders"] > 0 and withr["ntiles"] <= lay["ntiles"] and withr["check"] == 0:
            pk, riders = 5, withr["nriders"]
    if not groups:
        dyn = dyn_lds(length, L)
        fits = static_lds(pk + 2, d) + dyn <= LDS_WAVE_BUDGET
        groups_fit = static_lds(pk, d) + dyn <= LDS_WAVE_BUDGET
        if fits or not groups_fit:
            pk += 2
    return pk, riders, True


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_case_reaches_the_variant_the_table_says(probe, case):
    assert (case.L, case.d) in helpers.ALL_LD, "no bit-sliced instantiation: a table error"
    pk, riders, one_piece = plan(probe, case.L, case.d, case.length, case.n)
    assert (pk, riders > 0) == (case.pk, case.riders)
    assert one_piece == (S.lanes_of(case.L, case.length) > 0)
    # under KERNEL_BITSLICE_GROUPS the same packing runs the group-record variant
    gpk, griders, _ = plan(probe, case.L, case.d, case.length, case.n, groups=True)
    assert gpk == {6: 4, 7: 5}.get(case.pk, case.pk) and griders == riders
    if riders:
        assert case.length <= S.RIDER_B0 * S.W and has_riders_variant(case.L) and (case.n, riders) == (70, 2)
    if one_piece:   # a second tile exists, and it is a short one: its rows use the second profile copy
        lanes = S.lanes_of(case.L, case.length)
        assert case.n == S.rows_for(lanes) and _pack(probe, np.arange(case.n), case.length, case.L, 0)["ntiles"] == 2


def test_the_table_holds_what_the_sweep_is_for():
    C = S.CASES
    assert {(c.L, c.d) for c in C if c.length == 300 and c.n == 70} == set(helpers.ALL_LD) and len(helpers.ALL_LD) == 43
    assert all(c.pk == (6 if c.L == 12 else 5 if (c.L, c.d) == (11, 5) else 7) for c in S.AT_300)
    assert {c.pk for c in C} == {1, 2, 4, 5, 6, 7}
    five = [c for c in C if S.lanes_of(c.L, c.length) == 5 and c.d == 4]
    assert five and all(c.pk == 4 for c in five)                                   # shift records do not fit, group records do
    assert any(c.d == 4 and c.pk == 6 and S.lanes_of(c.L, c.length) == 4 for c in C)   # the neighbour band: both fit
    for c in C:                                                                    # neither fits: shift records again
        if (c.L, c.d, c.length) == (10, 4, 1869):
            assert c.pk == 6 and static_lds(4, c.d) + dyn_lds(c.length, c.L) > LDS_WAVE_BUDGET
    for lanes in (1, 2, 3, 5, 6):           # both edges of the band, and the first length below it
        at = {(c.L, c.length) for c in C if S.lanes_of(c.L, c.length) == lanes}
        Ls = {L for L, _ in at}
        assert any((L, S.band(L, lanes)[0]) in at and (L, S.band(L, lanes)[1]) in at for L in Ls), lanes
        assert any(c.pk in (1, 2) and c.length == S.band(c.L, lanes)[0] - 1 for c in C), lanes
    assert any(c.length == 320 and c.pk == 6 and not c.riders for c in C)
    assert len(S.MODE_CASES) == 4 and {c.pk for c in S.MODE_CASES} == {7, 5, 4}


@pytest.mark.parametrize("L", range(5, 13))
def test_bands_are_the_packings(probe, L):
    """Every length from L to 2 047 bp: the rows keep one resident piece per lane, and the pre-launch check accepts the
    layout, exactly inside the bands of same_length_cases.band; no same-length problem reaches seven lanes."""
    assert S.band(L, 7) is None and S.band(L, 6)[1] < S.MAXLEN
    for length in range(L, S.MAXLEN + 1):
        lay = _pack(probe, np.arange(4), length, L, 0)
        lanes = lay["pieces"][:, 0]
        one_piece = not (lanes[1:] == lanes[:-1]).any() and lay["check"] == 0
        k = S.lanes_of(L, length)
        assert one_piece == (k > 0), length
        if k:
            assert len(lanes) == 4 * k and lay["pieces"][:, 5].max() // S.lane_capacity(L) == k - 1, length


def test_the_fuzz_tool_draws_from_the_same_bands():
    """tools/fuzz_parity.py keeps its own copy of the band rule (it must load without this test package's newer files)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(helpers.ROOT, "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.BITSLICED == helpers.ALL_LD
    for L in range(5, 13):
        for lanes in range(1, 7):
            assert mod.band(L, lanes) == S.band(L, lanes)


def test_lds_rule_matches_the_header():
    """The figures the header asserts at compile time and DESIGN.md quotes, and the (11, 5) fallback"""
    assert static_lds(7, 3) + dyn_lds(300, 11) == 4328 and static_lds(6, 3) + dyn_lds(600, 10) == 3500
    assert static_lds(7, 5) + dyn_lds(300, 11) > LDS_WAVE_BUDGET >= static_lds(5, 5) + dyn_lds(300, 11)
