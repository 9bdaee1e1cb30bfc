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
