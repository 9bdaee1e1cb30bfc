"""The instruction profile of the same-length Gram kernel WITH RIDERS (k_gram_bitslice PK = 5: what config 2 runs), read from
the ISA of the product build by tools/issue_model.py, held to the bounds that tests/test_host_logic.py pins for the variant
without riders: the counting loop is the same loop (120-145 VALU instructions per shift), and what the rider tag adds to a
trip -- one LDS read, a compare, two selects -- stays inside at most 90 VALU instructions, at most 18 LDS instructions
and exactly one vector-memory gather."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kernel", [[10, 11, 3, 5], [10, 10, 3, 5]])
def test_rider_variant_keeps_the_pinned_profile(built, kernel):
    obj = os.path.join(ROOT, "gkmqc_amd", "csrc", "build", "gkm_gram_bitslice.o")
    if not (os.path.exists(obj) and shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin")):
        pytest.skip("needs the built device object and llvm-objdump")
    spec = importlib.util.spec_from_file_location("issue_model", os.path.join(ROOT, "tools", "issue_model.py"))
    im = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(im)
    m = im.analyse(obj, kernel, 4)
    plain = im.analyse(obj, kernel[:3] + [4], 4)
    shift = m["per_shift"]["full_rate"] + m["per_shift"]["sgpr_operand"] + m["per_shift"]["half_rate"]
    assert 120 <= shift <= 145, shift
    # the counting loop is not touched: instruction for instruction what the variant without riders has
    assert all(m["per_shift"][k] == plain["per_shift"][k] for k in ("full_rate", "sgpr_operand", "half_rate", "lds"))
    assert m["per_shift"]["sgpr_operand"] >= 2 * 10
    trip = m["trip"]["full_rate"] + m["trip"]["sgpr_operand"] + m["trip"]["half_rate"]
    assert m["trip_copies"] >= 7 and 50 <= trip <= 90, trip
    assert 8 <= m["trip"]["lds"] <= 18 and m["trip"]["vmem"] == 1
    # ... and costs a trip no more than the tag read and a handful of VALU instructions
    plain_trip = plain["trip"]["full_rate"] + plain["trip"]["sgpr_operand"] + plain["trip"]["half_rate"]
    assert m["trip"]["lds"] == plain["trip"]["lds"] + 1 and trip <= plain_trip + 8
