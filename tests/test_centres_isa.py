"""The instruction profile of the shift-record kernels' counting loop once it steps no counter (gkm_bitslice.h
window_group_any_centres: per group of five words the centre window's adder tree and ten ops), read from the ISA of the product
build by tools/issue_model.py.

Where the bounds come from, per shift at W = 10, L = 11 (P = 4 planes): 20 for the match words, 10 for the extension words, two
adder trees of 16 (7 full adders + 1 half adder), two groups of 10 (three per side, four to combine), 6 for the one compaction
and the origin word: 88.  L = 10 has one extension word less (87; the bias of one rides in the trees' half adders); L = 12,
d = 4 one more and larger trees: 95 in the listing.  The bounds are those figures + 1.  The crossings loop they replace listed 106 /
105 / 110 (tests/test_crossings_isa.py, whose upper bounds this build meets as well).

The build's listing when these bounds were set (VALU = full-rate + SGPR-operand + half-rate):

    variant        per shift: VALU  half-rate  SGPR-operand  compactions  LDS     one trip: VALU  LDS  gathers   VGPRs  scratch
    [10,11,3,4]               122   8          21            2            2                 76    10   1         71     0
    [10,11,3,6]               88    4          21            1            2                 82    12   1         71     0
    [10,11,3,7]               88    4          21            1            2                 87    13   1         69     0
    [10,10,3,6]               87    4          21            1            2                 82    12   1         71     0
    [10,12,4,6]               95    4          21            1            2                 82    12   1         71     0

The trips are instruction for instruction what tests/test_shift_records_isa.py pins: the change is in the counting loop alone.
Instruction CLASSES are counted (full rate, SGPR operand, half rate, LDS, compactions), never particular opcodes.

tools/issue_model.py finds the counting loop as the smallest loop body with the column words' scalar loads and exactly one
block's push sites; the group-record kernel's figures, which tests/test_crossings_isa.py and tests/test_host_logic.py pin,
must come out of that rule as they did out of the old one."""
import importlib.util
import os
import shutil

import pytest

from tests.test_shift_records_isa import TRIP_LDS_MAX, TRIP_VALU_MAX, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> VALU instructions per shift at most: the listing's figure + 1
SHIFT_VALU_MAX = {(10, 11, 3, 7): 89, (10, 11, 3, 6): 89, (10, 10, 3, 6): 88, (10, 12, 4, 6): 96}


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
def test_counting_loop_of_the_shift_record_kernels(im, kernel):
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


def test_group_record_kernel_keeps_its_loop(im):
    """[10,11,3,4] (kernel code 3, the on-GPU cross-check of the new loop) is built from window_group_any_grouped as before, and
    the tool's new loop detection reads it as the old one did"""
    m = im.analyse(im.obj, [10, 11, 3, 4], 4)
    ps = m["per_shift"]
    print("[10,11,3,4] per shift", ps)
    assert (_valu(ps), ps["half_rate"], ps["sgpr_operand"], ps["compactions"], ps["lds"]) == (122, 8, 21, 2, 2), ps
    r = im.resources(im.obj, [10, 11, 3, 4])
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r
