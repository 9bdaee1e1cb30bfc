"""The instruction profile of the shift-record kernels' counting loop with SHIFT-SHARED centre trees (gkm_bitslice.h
window_group_any_centres, SHIFTED = true), read from the ISA of the product build by tools/issue_model.py.

Where the bounds come from, per shift at W = 10, L = 11 (P = 4 planes): 20 for the match words; 9 for the extension words (Z10 ..
Z14 and Z16 .. Z19: Z15 has no reader left); 23 for the trees -- 4 for S = z3 + .. + z7 (two full adders: s; k1, k2), 3 for its
planes shifted one bit row on, 4 for U = Z8 + .. + Z12 (u; m1, m2), and per centre one full adder in column 0 over {z2 or z7, s or
s >> 1, u} and two in column 1 over {k1, k2 (shifted for the second centre), m1, m2, that carry}; per group 6 for the two sides'
steps, 2 to combine them with plane 0 and 3 for the threshold (y = b1 & v, maj(p, q, y), & AVg); 6 for the one compaction and the
origin word: 20 + 9 + 23 + 2 x 11 + 6 = 80.  L = 10 has one extension word less (Z14 drops out) and the bias of one as the third
input of each centre's column-0 adder: 79.  The bounds are those figures + 1.  The shared trees they replace listed 82 / 82 / 81
(tests/test_shared_trees_isa.py, whose upper bounds this build meets as well); (10, 2) went from 83 to 79 and (11, 4) from 90 to
88 in the same way, and (12, 4), which stays on the shared form, lists 93 as before.

The build's listing when these bounds were set (VALU = full-rate + SGPR-operand + half-rate):

    variant        per shift: VALU  half-rate  SGPR-operand  compactions  LDS     one trip: VALU  LDS  gathers   VGPRs  scratch  static LDS
    [10,11,3,4]               122   8          21            2            2                 76    10   1         71     0
    [10,11,3,6]               80    4          21            1            2                 82    12   1         71     0        2 560
    [10,11,3,7]               80    4          21            1            2                 87    13   1         69     0        3 840
    [10,10,3,6]               79    4          21            1            2                 82    12   1         71     0        2 560

The trips are instruction for instruction what tests/test_shift_records_isa.py pins: the change is in the counting loop alone.
Instruction CLASSES are counted (full rate, SGPR operand, half rate, LDS, compactions), never particular opcodes."""
import importlib.util
import os
import shutil

import pytest

from tests.test_shift_records_isa import TRIP_LDS_MAX, TRIP_VALU_MAX, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> VALU instructions per shift at most: the listing's figure + 1
SHIFT_VALU_MAX = {(10, 11, 3, 7): 81, (10, 11, 3, 6): 81, (10, 10, 3, 6): 80}
# profiles [d + 1][64, or 128 with riders], 128 shift records of three words, 64 rider tags (gkm_gram_bitslice.h)
STATIC_LDS = {(10, 11, 3, 7): 3840, (10, 11, 3, 6): 2560, (10, 10, 3, 6): 2560}


@pytest.fixture(scope="module")
def im(built):
    obj = os.path.join(ROOT, "gkmqc_amd", "csrc", "build", "gkm_gram_bitslice.o")
    if not (os.path.exists(obj) and shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin")):
        pytest.skip("needs the built device object and llvm-objdump")
    spec = importlib.util.spec_from_file_location("issue_model", os.path.join(ROOT, "tools", "issue_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.obj = obj
    return mod


@pytest.mark.parametrize("kernel", sorted(SHIFT_VALU_MAX))
def test_counting_loop_with_shift_shared_trees(im, kernel):
    kernel = list(kernel)
    pk = kernel[3]
    m = im.analyse(im.obj, kernel, 4)
    shift = _valu(m["per_shift"])
    print(kernel, "per shift", m["per_shift"], "trip", m["trip"])
    assert shift <= SHIFT_VALU_MAX[tuple(kernel)], shift
    assert m["per_shift"]["half_rate"] <= 4
    assert m["per_shift"]["compactions"] == 1
    assert m["per_shift"]["lds"] <= 2
    assert m["per_shift"]["sgpr_operand"] >= 2 * 10                   # the column's two bit planes per word, as before
    # the figures are those of one block of four shifts, not of a fallback or of a sub-loop
    assert m["per_shift"]["note"].startswith("the loop over blocks of 4 shifts")
    assert shift == int(shift) and shift >= 60, shift
    # the trips: the bounds of tests/test_shift_records_isa.py
    assert m["trip_copies"] >= 4
    assert 50 <= _valu(m["trip"]) <= TRIP_VALU_MAX[pk], _valu(m["trip"])
    assert 8 <= m["trip"]["lds"] <= TRIP_LDS_MAX[pk], m["trip"]["lds"]
    assert m["trip"]["vmem"] == 1
    r = im.resources(im.obj, kernel)
    print(kernel, r)
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r
    assert r["static_lds_bytes"] == STATIC_LDS[tuple(kernel)], r


def test_group_record_kernel_keeps_its_profile(im):
    """[10,11,3,4] (kernel code 3, the on-GPU cross-check of the new loop) is built from window_group_any_grouped as before:
    exactly its present profile"""
    m = im.analyse(im.obj, [10, 11, 3, 4], 4)
    ps = m["per_shift"]
    print("[10,11,3,4] per shift", ps)
    assert (_valu(ps), ps["half_rate"], ps["sgpr_operand"], ps["compactions"], ps["lds"]) == (122, 8, 21, 2, 2), ps
    r = im.resources(im.obj, [10, 11, 3, 4])
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r
