"""The instruction profile of the shift-record kernels' counting loop once it groups hits from top-plane crossings
(gkm_bitslice.h window_group_any_crossings, from the middle), read from the ISA of the product build by tools/issue_model.py.

Where the bounds come from: the group-record variant PK = 4 of the same build keeps window_group_any_grouped and its 122 / 121 /
126 VALU instructions per shift (L = 11 / 10 / 12); shift records take 4 off (tests/test_shift_records_isa.py); not stepping
the top plane takes 7 off in the one-direction form, which every instantiation can fall back to, and 12 in the from-the-middle
form: 111 / 110 / 115 at most.  The from-the-middle form is what the build keeps (it fits 72 VGPRs without scratch in every
instantiation), so the bounds below are its listing's figures + 1.

The build's listing when these bounds were set (VALU = full-rate + SGPR-operand + half-rate):

    variant        per shift: VALU  half-rate  SGPR-operand  compactions  LDS     one trip: VALU  LDS  gathers   VGPRs  scratch
    [10,11,3,4]               122   8          21            2            2                 76    10   1         71     0
    [10,11,3,6]               106   4          21            1            2                 82    12   1         71     0
    [10,11,3,7]               106   4          21            1            2                 87    13   1         69     0
    [10,10,3,4]               121   8          21            2            2                 76    10   1         71     0
    [10,10,3,6]               105   4          21            1            2                 82    12   1         71     0
    [10,12,4,4]               126   8          21            2            2                 77    10   1         71     0
    [10,12,4,6]               110   4          21            1            2                 82    12   1         71     0

(The one-direction form, -DGKM_BS_CROSSINGS_MIDDLE=0, lists 111 / 111 / 110 / 115 for the four shift-record kernels.)  The
trips are instruction for instruction what tests/test_shift_records_isa.py pins: the change is in the counting loop alone."""
import importlib.util
import os
import shutil

import pytest

from tests.test_shift_records_isa import TRIP_LDS_MAX, TRIP_VALU_MAX, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> VALU instructions per shift at most: the listing's figure + 1 (the issue's bounds were 111 / 111 / 110 / 115)
SHIFT_VALU_MAX = {(10, 11, 3, 7): 107, (10, 11, 3, 6): 107, (10, 10, 3, 6): 106, (10, 12, 4, 6): 111}
# what the group-record variant of the same (L, d) lists, and what the one-direction form guarantees below it
GROUPS_VALU = {11: 122, 10: 121, 12: 126}


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
    groups = im.analyse(im.obj, kernel[:3] + [4], 4)
    shift, gshift = _valu(m["per_shift"]), _valu(groups["per_shift"])
    print(kernel, "per shift", m["per_shift"], "trip", m["trip"], "group records per shift", groups["per_shift"])
    # the group-record kernel of the same (L, d) keeps the loop it had
    assert gshift == GROUPS_VALU[kernel[1]] and groups["per_shift"]["compactions"] == 2, gshift
    # -4 for shift records, -7 for the form that is always reachable; the from-the-middle form's own figure + 1
    assert shift <= gshift - 4 - 7, (shift, gshift)
    assert shift <= SHIFT_VALU_MAX[tuple(kernel)], shift
    assert m["per_shift"]["half_rate"] <= 4
    assert m["per_shift"]["compactions"] == 1
    assert m["per_shift"]["sgpr_operand"] >= 2 * 10                   # the column's two bit planes per word, as before
    assert m["per_shift"]["lds"] <= groups["per_shift"]["lds"] and m["per_shift"]["lds"] <= 2
    # the trips: the bounds of tests/test_shift_records_isa.py
    assert m["trip_copies"] >= 4
    assert 50 <= _valu(m["trip"]) <= TRIP_VALU_MAX[pk], _valu(m["trip"])
    assert 8 <= m["trip"]["lds"] <= TRIP_LDS_MAX[pk], m["trip"]["lds"]
    assert m["trip"]["vmem"] == 1
    r = im.resources(im.obj, kernel)
    print(kernel, r)
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r


def test_group_record_kernel_keeps_its_loop(im):
    """[10,11,3,4] (kernel code 3, the on-GPU cross-check of the new loop) is built from window_group_any_grouped as before:
    within the 120-145 that tests/test_host_logic.py pins, and at the figures it had."""
    m = im.analyse(im.obj, [10, 11, 3, 4], 4)
    ps = m["per_shift"]
    print("[10,11,3,4] per shift", ps)
    assert 120 <= _valu(ps) <= 145, _valu(ps)
    assert (_valu(ps), ps["half_rate"], ps["sgpr_operand"], ps["compactions"], ps["lds"]) == (122, 8, 21, 2, 2), ps
    r = im.resources(im.obj, [10, 11, 3, 4])
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r
