"""The instruction profile of the shift-record kernels' counting loop once the two centre trees share the words they have in
common and the top half adder is folded into the threshold (gkm_bitslice.h window_group_any_centres, SHARED = true), read from
the ISA of the product build by tools/issue_model.py.

Where the bounds come from, per shift at W = 10, L = 11 (P = 4 planes): 20 for the match words, 10 for the extension words, 4 for
the two shared full adders FA(Z7, Z8, Z9) and FA(Z10, Z11, Z12), per group 10 for its tree (3 full adders in column 0 over its five
own words and the two shared sums, 2 in column 1 over their carries and the two shared ones), 6 for the two sides' steps, 2 to
combine them with plane 0 and 3 for the threshold (y = b1 & v, maj(p, q, y), & AVg), and 6 for the one compaction and the origin
word: 20 + 10 + 4 + 2 x (10 + 6 + 2 + 3) + 6 = 82.  L = 10 has one extension word less (81; the bias of one rides in the shared
half adder of Z10, Z11); L = 12, d = 4 shares two full adders over seven common words and keeps its last stage (a full adder in
column 2): 93 in the listing.  The bounds are those figures + 1.  The private trees they replace listed 88 / 88 / 87 / 95
(tests/test_centres_isa.py, whose upper bounds this build meets as well).

The build's listing when these bounds were set (VALU = full-rate + SGPR-operand + half-rate):

    variant        per shift: VALU  half-rate  SGPR-operand  compactions  LDS     one trip: VALU  LDS  gathers   VGPRs  scratch  static LDS
    [10,11,3,4]               122   8          21            2            2                 76    10   1         71     0
    [10,11,3,6]               82    4          21            1            2                 82    12   1         71     0        2 560
    [10,11,3,7]               82    4          21            1            2                 87    13   1         69     0        3 840
    [10,10,3,6]               81    4          21            1            2                 82    12   1         71     0        2 560
    [10,12,4,6]               93    4          21            1            2                 82    12   1         71     0        2 816

The trips are instruction for instruction what tests/test_shift_records_isa.py pins: the change is in the counting loop alone.
Instruction CLASSES are counted (full rate, SGPR operand, half rate, LDS, compactions), never particular opcodes."""
import importlib.util
import os
import shutil

import pytest

from tests.test_shift_records_isa import TRIP_LDS_MAX, TRIP_VALU_MAX, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> VALU instructions per shift at most: the listing's figure + 1
SHIFT_VALU_MAX = {(10, 11, 3, 7): 83, (10, 11, 3, 6): 83, (10, 10, 3, 6): 82, (10, 12, 4, 6): 94}
# profiles [d + 1][64, or 128 with riders], 128 shift records of three words, 64 rider tags (gkm_gram_bitslice.h)
STATIC_LDS = {(10, 11, 3, 7): 3840, (10, 11, 3, 6): 2560, (10, 10, 3, 6): 2560, (10, 12, 4, 6): 2816}


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
def test_counting_loop_with_shared_trees(im, kernel):
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
