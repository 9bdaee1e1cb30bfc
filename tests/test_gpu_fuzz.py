"""A short randomised parity sweep (tools/fuzz_parity.py: random kernel type, L, k, d, M, H, length
distributions incl. duplicates / poly-A / reverse complements) as part of the GPU suite.  Longer
sweeps were run by hand on the box: about 2 000 cases / 4 000 kernel runs without a mismatch."""
import importlib.util
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the seed that draws from the whole legal region (--region whole: d up to L, k from 0, L from 2).  Cases with d >= 5 outside
# the bit-sliced table are about one draw in twelve; this seed's second and fifth draws are such cases -- (3, 12, 1, 11) and
# (5, 6, 0, 5) -- so the sweep reaches one whatever the speed of the box.
WHOLE_REGION_SEED = 38


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12, WHOLE_REGION_SEED])
def test_random_parameter_sweep(built, seed, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    whole = ["--region", "whole"] if seed == WHOLE_REGION_SEED else []
    monkeypatch.setattr(sys, "argv", ["fuzz_parity.py", "--seconds", "12", "--seed", str(seed)] + whole)
    mod.main()                                   # raises SystemExit with the failing case on a mismatch
    out = capsys.readouterr().out
    assert "fuzz ok" in out
    high_d = int(re.search(r"(\d+) with d >= 5 outside the bit-sliced table", out).group(1))
    if whole:
        assert high_d > 0, "the whole-region sweep reached no case that only k_gram_direct serves"
    else:
        assert high_d == 0                       # (the default draw stops at d = 4 outside the table)


@pytest.mark.gpu
def test_random_svm_problems(built, monkeypatch, capsys):
    """tools/fuzz_svm.py: random kernels, sizes, class balance, C, tol, duplicated samples -- the GPU
    C-SVC bit-identical to scikit-learn (about 3 300 cases in the hand-run sweeps of round 1)."""
    spec = importlib.util.spec_from_file_location("fuzz_svm", os.path.join(ROOT, "tools", "fuzz_svm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setenv("GKM_SVM_MAX_ITER", "300000")     # a pathological draw is skipped after ~2 s instead of running 10^7 iterations
    monkeypatch.setattr(sys, "argv", ["fuzz_svm.py", "--seconds", "15", "--seed", "21"])
    mod.main()
    assert "svm fuzz ok" in capsys.readouterr().out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [22])
def test_random_svm_problems_varied_diagonals(built, seed, monkeypatch, capsys):
    """the same sweep drawing from the kinds whose diagonal is not constant or which are indefinite as well (--kinds:
    vardiag, krein, poly beside the default three): same budget, same iteration cap"""
    spec = importlib.util.spec_from_file_location("fuzz_svm", os.path.join(ROOT, "tools", "fuzz_svm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setenv("GKM_SVM_MAX_ITER", "300000")
    monkeypatch.setattr(sys, "argv", ["fuzz_svm.py", "--seconds", "15", "--seed", str(seed), "--kinds", ",".join(mod.KINDS)])
    mod.main()
    out = capsys.readouterr().out
    assert "svm fuzz ok" in out
    seen = dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", re.search(r"kinds: (.*)", out).group(1)))
    assert seen["vardiag"] + seen["krein"] + seen["poly"] > 0, seen


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [13, 14])
def test_random_block_sweep(built, seed, monkeypatch, capsys):
    """tools/fuzz_block.py: the column-range launch of the scoring path (random rows, ranges, leading dimensions,
    kernels, GKM_FORCE_PACKED / GKM_COL_CHUNK) -- raw values bit for bit, kernel values and untouched sentinels."""
    spec = importlib.util.spec_from_file_location("fuzz_block", os.path.join(ROOT, "tools", "fuzz_block.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.delenv("GKM_FORCE_PACKED", raising=False)
    monkeypatch.delenv("GKM_COL_CHUNK", raising=False)
    monkeypatch.setattr(sys, "argv", ["fuzz_block.py", "--seconds", "12", "--seed", str(seed)])
    mod.main()
    assert "block fuzz ok" in capsys.readouterr().out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [15, 16])
def test_random_interpretation_sweep(built, seed, monkeypatch, capsys):
    """tools/fuzz_interpret.py: explain / ism / hypothetical tallies and the mutants' self profiles on random shapes (tiled
    and k = 0 included), weights and row / column subsets, dense-hit sequences mixed with iid ones -- bit for bit the CPU
    references."""
    spec = importlib.util.spec_from_file_location("fuzz_interpret", os.path.join(ROOT, "tools", "fuzz_interpret.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["fuzz_interpret.py", "--seconds", "12", "--seed", str(seed)])
    mod.main()                                   # raises SystemExit with the failing case on a mismatch
    assert "interpret fuzz ok" in capsys.readouterr().out


# tools/fuzz_windows.py.  The seed was picked on the CPU (--dry: the draw without the device) as the first of 1..4000 whose
# first 40 cases hold a case of each of the five kinds asserted below (the 35th takes 68 732 bytes of LDS: L = 12, d = 12,
# W = 75, strides 1 and 63), so every longer run of it does too.  The count is set for the 12 to 15 s of the sibling sweeps:
# 120 cases took 12.5 s on the MI355X box, run after the other window tests (130 cases took 15.9 s as the first test of a
# process, HIP start-up included, and 170 cases 17.3 s; the oracle's share is 3.5e9 l-mer comparisons of the 120 cases).
WINDOW_SEED, WINDOW_CASES = 549, 120


@pytest.mark.gpu
def test_random_window_sweep(built, monkeypatch, capsys):
    """tools/fuzz_windows.py: the scan's words and self profiles, k_wsim_profiles' profiles and G (exact against the oracle),
    window_kernel against cross_kernel byte for byte and window_best, over the whole legal (L, k, d, W, stride) region.  A
    fixed count of cases, so that the same cases run on every box."""
    spec = importlib.util.spec_from_file_location("fuzz_windows", os.path.join(ROOT, "tools", "fuzz_windows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["fuzz_windows.py", "--cases", str(WINDOW_CASES), "--seed", str(WINDOW_SEED)])
    mod.main()                                   # raises SystemExit with the failing case on a mismatch
    out = capsys.readouterr().out
    assert "window fuzz ok: %d cases" % WINDOW_CASES in out
    seen = re.search(r"(\d+) with d >= 9, (\d+) with more than 64 KiB of LDS, (\d+) with a stretch-limited tile of k_wsim_profiles, "
                     r"(\d+) with a stretch-limited group of k_scan_profiles, (\d+) with L <= 3", out)
    assert seen and all(int(v) > 0 for v in seen.groups()), out
