"""The instruction profile of the same-length Gram kernel's SHIFT-RECORD variants (k_gram_bitslice PK = 6, and PK = 7 with
riders: what config 2 runs), read from the ISA of the product build by tools/issue_model.py and held against the same build's
group-record variant PK = 4, whose own profile tests/test_host_logic.py and tests/test_rider_isa.py pin.

The build's listing when these bounds were set (VALU = full-rate + SGPR-operand + half-rate):

    variant        per shift: VALU  half-rate  compactions  LDS     one trip: VALU  LDS  gathers   VGPRs  scratch
    [10,11,3,4]               122   8          2            2                 76    10   1         71     0
    [10,11,3,6]               118   4          1            2                 82    12   1         71     0
    [10,11,3,7]               118   4          1            2                 87    13   1         69     0
    [10,10,3,4]               121   8          2            2                 76    10   1         71     0
    [10,10,3,6]               117   4          1            2                 82    12   1         71     0

Per shift the second v_cmp / v_mbcnt_lo / v_mbcnt_hi / v_add_lshl and the second origin v_or_b32 are gone and one v_or_b32 (any0 |
any1) has come: -4 VALU, all four of them half-rate.  The three words of a push are one ds_write2st64_b32 and one ds_write_b32:
as many LDS instructions as the two pushes of the group records had.  A trip reads and re-pushes one word more (+2 LDS) and
takes the group from the record (+6 VALU; +5 more with the rider tag, as in PK = 5).  The trip's upper bounds below are
those figures plus three VALU instructions and one LDS instruction of slack for the compiler's scheduling."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIP_VALU_MAX = {6: 85, 7: 90}
TRIP_LDS_MAX = {6: 13, 7: 14}


def _valu(part):
    return part["full_rate"] + part["sgpr_operand"] + part["half_rate"]


@pytest.mark.parametrize("kernel", [[10, 11, 3, 6], [10, 11, 3, 7], [10, 10, 3, 6]])
def test_shift_record_variants_against_the_group_record_build(built, kernel):
    obj = os.path.join(ROOT, "gkmqc_amd", "csrc", "build", "gkm_gram_bitslice.o")
    if not (os.path.exists(obj) and shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin")):
        pytest.skip("needs the built device object and llvm-objdump")
    spec = importlib.util.spec_from_file_location("issue_model", os.path.join(ROOT, "tools", "issue_model.py"))
    im = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(im)
    pk = kernel[3]
    m = im.analyse(obj, kernel, 4)
    groups = im.analyse(obj, kernel[:3] + [4], 4)
    # exactly one compaction per shift (one v_mbcnt pair), where the group records have two
    assert m["per_shift"]["compactions"] == 1 and groups["per_shift"]["compactions"] == 2
    assert _valu(m["per_shift"]) <= _valu(groups["per_shift"]) - 4, (_valu(m["per_shift"]), _valu(groups["per_shift"]))
    assert m["per_shift"]["half_rate"] <= groups["per_shift"]["half_rate"] - 3
    assert m["per_shift"]["lds"] <= groups["per_shift"]["lds"]
    assert m["per_shift"]["sgpr_operand"] >= 2 * 10                   # the column's two bit planes per word, as before
    # one trip copy per push site (four shifts per block) at least; the trip within its bounds, one gather
    assert m["trip_copies"] >= 4
    assert 50 <= _valu(m["trip"]) <= TRIP_VALU_MAX[pk], _valu(m["trip"])
    assert 8 <= m["trip"]["lds"] <= TRIP_LDS_MAX[pk], m["trip"]["lds"]
    assert m["trip"]["vmem"] == 1
    # the same register class (seven waves per SIMD), no scratch, and the static LDS the launch plan reckons with
    r = im.resources(obj, kernel)
    assert r["vgprs"] <= 72 and r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, r
    slots = 128 if pk == 7 else 64
    assert r["static_lds_bytes"] == 4 * ((kernel[2] + 1) * slots + 3 * 128 + (64 if pk == 7 else 0)), r
