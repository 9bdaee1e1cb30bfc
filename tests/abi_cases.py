"""What tests/test_abi_layout_gpu.py and tests/test_abi_streams_gpu.py share: sentinel-filled device outputs whose
untouched cells are compared by bytes, NaN-padded matrices, and the launch table -- one small problem per path of a Gram
launch, with the kernel name, variant and riders a launch of it must report, so that a case can never quietly exercise
another path.

Row counts are never a multiple of 64 (k_untile moves 64-column blocks: the last block is always a partial one), and a
case's two leading dimensions are n + 3 (rows not 64-byte aligned) and 2 n + 1; the profiles take n + 5."""
from collections import namedtuple

import numpy as np

from tests import helpers
from tests import same_length_cases as S

# a quiet NaN with a payload: no computation produces it, and it compares unequal to itself, so only the bytes can be checked
SENTINEL_F64 = 0x7FF80000DEADBEEF
# profiles are sums of products of positional weights: never negative below the int32 wrap, which these problems are far from
SENTINEL_I32 = -0x7FFFFFFF

SAME, PACKED, PACKED128, DIRECT = ("k_gram_bitslice<same length>", "k_gram_bitslice<packed>", "k_gram_bitslice<packed,128>",
                                   "k_gram_direct")

# name, L, d, sequences (a function: made on first use), kernel code name, then what the launch reports, and the row of
# same_length_cases it is (None for the others)
Launch = namedtuple("Launch", "name L d seqs kernel kernel_name variant riders case")


def _same_length(L, d, length, n, pk, riders):
    case = [c for c in S.CASES if (c.L, c.d, c.length, c.n) == (L, d, length, n)]
    assert len(case) == 1 and (case[0].pk, case[0].riders) == (pk, riders), (L, d, length, n)
    case = case[0]
    return Launch("pk%d" % pk, L, d, lambda: same_length_input(case), "KERNEL_BITSLICE", SAME, pk, riders, case)


def same_length_input(case):
    """the sequences tests/test_same_length_sweep_gpu.py runs this row on (its oracle values are shared by key)"""
    from tests.test_rider_parity_gpu import _seqs
    return _seqs(case.n, case.length, 1000 * case.L + 100 * case.d + case.length)


def ragged():
    return helpers.synth_codes(35, 36, 300, (150, 600))


def ragged_301():
    return helpers.synth_codes(150, 151, 300, (150, 600))


LAUNCHES = [
    _same_length(10, 3, 300, 70, 7, True),
    _same_length(12, 4, 300, 70, 6, False),
    _same_length(11, 5, 300, 70, 5, True),
    _same_length(10, 4, 1521, 15, 4, False),
    Launch("packed", 11, 3, ragged, "KERNEL_BITSLICE", PACKED, 1, False, None),
    Launch("packed128", 10, 3, lambda: helpers.synth_codes(150, 151, 300, (60, 110)), "KERNEL_BITSLICE", PACKED128, 2, False,
           None),
    Launch("direct", 11, 3, ragged, "KERNEL_DIRECT", DIRECT, 0, False, None),
]
WEIGHTINGS = [4, 2]          # kernel types: positional weights and none


def launch_id(x):
    return x.name


def by_name(name):
    return [x for x in LAUNCHES if x.name == name][0]


def leading_dimensions(n):
    assert n % 64
    return [n + 3, 2 * n + 1]


def assert_path(ctx, launch):
    """the most recent Gram launch of `ctx` took the path the table names"""
    got = (ctx.last_kernel_name(), ctx.last_variant(), ctx.last_riders() > 0)
    assert got == (launch.kernel_name, launch.variant, launch.riders), (launch.name, got)


def subset_with_a_jump(n):
    """the ascending row subset of test_gpu_parity.test_row_subsets_and_local_rows"""
    return np.array(sorted(set(range(0, n, 3)) | {1, n - 1}), dtype=np.int32)


# ------------------------------------------------------------------ sentinels
def sentinel_f64(shape, device="cuda"):
    import torch
    return torch.full(tuple(shape), SENTINEL_F64, dtype=torch.int64, device=device).view(torch.float64)


def sentinel_i32(shape, device="cuda"):
    import torch
    return torch.full(tuple(shape), SENTINEL_I32, dtype=torch.int32, device=device)


def refill(t):
    """put the sentinel back into every cell of a tensor made by sentinel_f64 / sentinel_i32 (on the current stream)"""
    import torch
    if t.dtype == torch.float64:
        t.view(torch.int64).fill_(SENTINEL_F64)
    else:
        assert t.dtype == torch.int32
        t.fill_(SENTINEL_I32)


def bits(t):
    """a tensor or array of doubles / int32 as a numpy array of integers of the same width: what `==` compares is the bytes"""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    if a.dtype == np.float64:
        return np.ascontiguousarray(a).view(np.int64)
    assert a.dtype in (np.int32, np.int64), a.dtype
    return a


def untouched(t, mask):
    """True if every cell of `t` that `mask` selects (a boolean array of t's shape, or of its leading axes) still holds
    the sentinel's bytes"""
    b = bits(t)
    want = SENTINEL_F64 if b.dtype == np.int64 else SENTINEL_I32
    return bool((b[np.asarray(mask, dtype=bool)] == want).all())


def same_bytes(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def nan_padded(K, ld, device="cuda"):
    """K ([m, n], numpy or torch) on the device inside an [m, ld] matrix whose columns n..ld-1 are NaN -> the [:, :n] view,
    row stride ld"""
    import torch
    K = torch.as_tensor(K)
    m, n = K.shape
    assert ld >= n
    full = torch.full((m, ld), float("nan"), dtype=torch.float64, device=device)
    full[:, :n] = K.to(device)
    view = full[:, :n]
    assert view.stride() == (ld, 1) and (ld == n or not view.is_contiguous())
    return view
