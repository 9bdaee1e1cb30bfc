"""Host side of the product library (no GPU needed): the C ABI loads and exports what
include/*.h declares; weights, positional weights and the FASTA reader match the
reference fixtures; the boundary fails loudly (non-zero, no crash) without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import helpers

ROOT = helpers.ROOT


@pytest.fixture(scope="module")
def dev(built):
    from gkmqc_amd import device
    device.load()
    return device


def _declared_functions(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gkm(?:hip|svm)?_[a-z0-9_]+)\s*\(", txt)))


@pytest.mark.parametrize("header,least", [("gkmkern_pylib.h", 8), ("gkm_hip.h", 8), ("gkm_svm.h", 3)])
def test_every_declared_symbol_is_exported(dev, header, least):
    lib = ctypes.CDLL(dev.lib_path())
    names = _declared_functions(header)
    assert len(names) >= least
    for name in names:
        assert hasattr(lib, name), "%s declared in include/%s but not exported" % (name, header)


@pytest.mark.parametrize("name", ["gkmhip_probe_copy", "gkmhip_probe_spin", "gkmhip_pause_stream",
                                  "gkmhip_create_stream_reserving", "gkmhip_create_stream_beside_prio"])
def test_measurement_probes_are_not_exported(dev, name):
    """The one-off probes of the collective-beside-Gram question are answered (profiles/r5_collective_beside_probe*.txt)
    and are no part of the drop-in library's surface."""
    assert not hasattr(ctypes.CDLL(dev.lib_path()), name)


def test_gkmopt_layout_matches_reference(dev):
    # x86-64 offsets probed from the reference build
    offs = [getattr(dev.gkmOpt, f).offset for f, _ in dev.gkmOpt._fields_]
    assert offs == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 60]
    assert ctypes.sizeof(dev.gkmOpt) == 64


def test_parameter_check_messages(dev):
    assert dev.check_parameters(4, 11, 7, 3) is None
    assert dev.check_parameters(6, 11, 7, 3) == "unknown kernel type"
    assert dev.check_parameters(-1, 11, 7, 3) == "unknown kernel type"
    assert dev.check_parameters(2, 1, 1, 0) == "L < 2"
    assert dev.check_parameters(2, 13, 7, 3) == "L > 12"
    assert dev.check_parameters(2, 10, 11, 0) == "k > L"
    assert dev.check_parameters(2, 10, 8, 3) == "d > L - k"


def test_mismatch_weights_bit_identical(dev):
    for (t, L, k, d), ref in helpers.golden_weights().items():
        got = dev.mismatch_weights(t, L, k)[: d + 1]
        assert got.tobytes() == ref.tobytes(), (t, L, k, d)


def test_position_weights(dev):
    cases, lens, _ = helpers.quirks_expected()
    for c in cases:
        for i, ln in enumerate(lens):
            n = int(ln) - c["L"] + 1
            got = dev.position_weights(c["kernel_type"], n, c["M"], c["H"])
            assert (got == c["wt"][i, :n]).all(), (c["idx"], i)


def test_region_mismatch_weights_bit_identical(dev):
    """all 528 (kernel type, L, k) with 2 <= L <= 12, 0 <= k <= L: c_0 .. c_{L-k} against the reference's
    (tests/golden/region_expected.npz)"""
    weights = helpers.region_expected()[3]
    assert len(weights) == 528
    for (t, L, k), ref in weights.items():
        assert dev.check_parameters(t, L, k, L - k) is None, (t, L, k)
        assert dev.mismatch_weights(t, L, k)[: L - k + 1].tobytes() == ref.tobytes(), (t, L, k)


def test_region_position_weights(dev):
    cases, lens, _, _ = helpers.region_expected()
    for c in cases:
        for i, ln in enumerate(lens):
            n = int(ln) - c["L"] + 1
            got = dev.position_weights(c["kernel_type"], n, c["M"], c["H"])
            assert (got == c["wt"][i, :n]).all(), (c["idx"], i)


def test_region_fasta_reader_lengths(dev):
    seqs, n_pos, n_invalid, n_trunc = dev.read_problem(helpers.REGION_POS, helpers.REGION_NEG)
    _, lens, npos, _ = helpers.region_expected()
    assert [len(s) for s in seqs] == list(lens) and n_pos == npos and n_invalid == 0 and n_trunc == 0


def test_fasta_reader_matches_oracle_and_reference_lengths(dev):
    from oracle import oracle as O
    seqs, n_pos, n_invalid, n_trunc = dev.read_problem(helpers.QUIRK_POS, helpers.QUIRK_NEG)
    oseqs, o_pos, o_invalid, o_trunc = O.read_problem(helpers.QUIRK_POS, helpers.QUIRK_NEG)
    _, lens, npos = helpers.quirks_expected()
    assert n_pos == npos == o_pos
    assert [len(s) for s in seqs] == list(lens)
    assert all((a == b).all() for a, b in zip(seqs, oseqs))
    assert (n_invalid, n_trunc) == (o_invalid, o_trunc)


def test_fasta_reader_edge_cases(dev, tmp_path):
    p = tmp_path / "p.fa"
    n = tmp_path / "n.fa"
    # text before the first header is ignored; last line without newline; long single line
    p.write_bytes(b"junk before header\n>a desc\nACGT\n\nacgtn\n>b\n" + b"G" * 3000 + b"\n>c\nTT\r\nGG\r\n>d")
    n.write_bytes(b">x\nAAAA")
    seqs, n_pos, n_invalid, n_trunc = dev.read_problem(str(p), str(n))
    assert n_pos == 4 and len(seqs) == 5
    assert seqs[0].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert len(seqs[1]) == 2047 and n_trunc == 1
    assert seqs[2].tolist() == [3, 3, 2, 2]
    assert len(seqs[3]) == 0
    assert seqs[4].tolist() == [0, 0, 0, 0]
    assert n_invalid == 1
    with pytest.raises(dev.GkmError):
        dev.read_problem(str(tmp_path / "missing.fa"), str(n))


def test_fasta_reader_on_large_quirky_files(dev, tmp_path):
    """The mmap reader against the oracle's on files of 0.4-0.7 MB (the quirks fixture is 20 KB) full of what can go wrong:
    junk before the first header, CRLF, blank lines, multi-line records, '>' inside a line, records of 0 and of 3 000
    bases (truncated at 2 047), lower case and N, a last line without its newline.  (Round 5 also parsed such files in
    four ranges cut at headers, at the same time: same result, 0.3 ms of a 72-ms call -- not kept.)"""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)

    def make(path, records, junk):
        out = [junk]
        for i in range(records):
            kind = int(rng.integers(0, 10))
            n = 0 if kind == 0 else 3000 if kind == 1 else int(rng.integers(1, 700))
            seq = letters[rng.integers(0, 8 if kind < 8 else 10, n)].tobytes()
            eol = b"\r\n" if kind == 2 else b"\n"
            out.append(b">r%d with > inside the header" % i + eol)
            width = int(rng.choice([60, 61, 80, 1000000]))
            for at in range(0, len(seq), width):
                line = seq[at:at + width]
                out.append(line + (b" >not a header" if kind == 3 and at == 0 else b"") + eol)
                if kind == 4:
                    out.append(eol)
        blob = b"".join(out)
        path.write_bytes(blob[:-1])     # (the last line has no newline)
        return len(blob)

    p, n = tmp_path / "p.fa", tmp_path / "n.fa"
    assert make(p, 2500, b"junk line\nmore junk > here\n") > 600 * 1024 and make(n, 1800, b"") > 400 * 1024
    seqs, n_pos, n_invalid, n_trunc = dev.read_problem(str(p), str(n))
    oseqs, o_pos, o_invalid, o_trunc = O.read_problem(str(p), str(n))
    assert (n_pos, len(seqs)) == (o_pos, len(oseqs)) == (2500, 4300)
    assert all(len(a) == len(b) and (a == b).all() for a, b in zip(seqs, oseqs))
    assert (n_invalid, n_trunc) == (o_invalid, o_trunc) and n_trunc > 100 and n_invalid > 1000


def _call_wrapper(dev, opt, nrows=64):
    kmat = np.full((nrows, nrows), -7.0)
    rows = (kmat.ctypes.data + np.arange(nrows) * kmat.strides[0]).astype(np.uintp)
    sizes = np.full(2, -1, dtype=np.int32)
    rc = dev.load().gkm_main_pywrapper(ctypes.byref(opt), rows.ctypes.data, sizes.ctypes.data)
    return rc, kmat, sizes


def test_boundary_rejects_bad_input_without_touching_output(dev, tmp_path):
    def opt(**kw):
        base = dict(kernel_type=4, L=11, k=7, d=3, M=50, H=50.0, gamma=1.0,
                    posfile=helpers.QUIRK_POS.encode(), negfile=helpers.QUIRK_NEG.encode(), nthreads=1, verbosity=0)
        base.update(kw)
        return dev.gkmOpt(**base)
    # k = -1 passes the reference's parameter check (src/gkmkern_pylib.c:38-64 never tests k >= 0); the weights
    # routine then refuses it, and the call must stop there instead of running on uninitialised weights
    for bad in (opt(L=13), opt(d=5), opt(kernel_type=9), opt(verbosity=7), opt(k=-1),
                opt(posfile=str(tmp_path / "nope.fa").encode())):
        rc, kmat, sizes = _call_wrapper(dev, bad)
        assert rc != 0
        assert (kmat == -7.0).all() and (sizes == -1).all()
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    rc, kmat, _ = _call_wrapper(dev, opt(posfile=str(empty).encode()))
    assert rc != 0 and (kmat == -7.0).all()
    short = tmp_path / "short.fa"
    short.write_bytes(b">s\nACGTAC\n")   # shorter than L: undefined in the reference, an error here
    rc, kmat, _ = _call_wrapper(dev, opt(posfile=str(short).encode()))
    assert rc != 0 and (kmat == -7.0).all()


def test_no_silent_cpu_fallback(dev):
    """Without a GPU the product must fail loudly; with one it must succeed."""
    import torch
    o = dev.gkmOpt(4, 11, 7, 3, 50, 50.0, 1.0, helpers.QUIRK_POS.encode(), helpers.QUIRK_NEG.encode(), 1, 0)
    rc, kmat, sizes = _call_wrapper(dev, o)
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc != 0 and (kmat == -7.0).all()
        with pytest.raises(dev.GkmError):
            dev.GramContext(4, 11, 7, 3)


def test_product_does_not_reference_the_oracle():
    """The shipped package must not import, link or load anything under oracle/."""
    pkg = os.path.join(ROOT, "gkmqc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "liboracle" not in txt and "gkm_oracle" not in txt and "from oracle" not in txt \
                    and "import oracle" not in txt and "_ref/" not in txt, os.path.join(dirpath, f)


def test_no_timing_variants_in_the_product(built):
    """The ablation kernels of rounds 1-3 (a fifth template parameter VARIANT != 0: parts of the work skipped, WRONG
    results) and the GKM_VARIANT switch that selected them are gone from the source (tools/variants.sh rebuilds them
    from revision a4bed73 into build_variants/): the drop-in library holds four-parameter instantiations only, and
    neither the library nor the kernel source knows the switch."""
    import re
    blob = open(os.path.join(ROOT, "gkmqc_amd", "bin", "gkmkern_pylib.so"), "rb").read()
    found = re.findall(rb"_Z15k_gram_bitsliceILi\d+ELi\d+ELi\d+ELi[0123]E(Li\d+E)?Ev6BsArgs", blob)
    assert len(found) > 100 and set(found) == {b""}, set(found)
    assert b"GKM_VARIANT" not in blob
    for f in ("gkm_gram_bitslice.hip", "gkm_gram_bitslice.h", "gkm_gram.hip", "gkm_bitslice.h", "gkm_pack.h"):
        assert "VARIANT" not in open(os.path.join(ROOT, "gkmqc_amd", "csrc", f)).read(), f


@pytest.mark.parametrize("value", ["0,x", "7,", "-1", "99", "two"])
def test_device_selection_is_validated(dev, monkeypatch, value):
    """GKM_DEVICES / GKM_DEVICE that do not name HIP devices of the node are errors, not a silent
    fallback to device 0 (atoi("x") used to make "0,x" mean device 0 twice)."""
    for var in ("GKM_DEVICES", "GKM_DEVICE"):
        monkeypatch.delenv("GKM_DEVICES", raising=False)
        monkeypatch.delenv("GKM_DEVICE", raising=False)
        monkeypatch.setenv(var, value)
        o = dev.gkmOpt(4, 11, 7, 3, 50, 50.0, 1.0, helpers.QUIRK_POS.encode(), helpers.QUIRK_NEG.encode(), 1, 0)
        rc, kmat, sizes = _call_wrapper(dev, o)
        assert rc != 0 and (kmat == -7.0).all() and (sizes == -1).all()


def test_issue_model_reads_the_hot_kernel(built):
    """tools/issue_model.py (the analysis behind DESIGN.md §5a and `roofline.issue_model`) must keep finding, in the ISA of
    the product build, the counting loop (four shifts per block, ~130 VALU instructions per shift, the two SGPR-operand
    instructions per word among them) and the trips (one copy per push site + the final partial one), and must price the
    half-rate opcodes apart from the full-rate ones."""
    import importlib.util
    import shutil
    obj = os.path.join(ROOT, "gkmqc_amd", "csrc", "build", "gkm_gram_bitslice.o")
    if not (os.path.exists(obj) and shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin")):
        pytest.skip("needs the built device object and llvm-objdump")
    spec = importlib.util.spec_from_file_location("issue_model", os.path.join(ROOT, "tools", "issue_model.py"))
    im = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(im)
    assert im.classify("v_bitop3_b32 v1, v2, v3, v4 bitop3:0x96") == "F"
    assert im.classify("v_xor_b32_e32 v1, s5, v3") == "S"
    assert im.classify("v_lshlrev_b32_e32 v1, 1, v3") == "H" and im.classify("v_bcnt_u32_b32 v1, v2, v3") == "H"
    assert im.classify("s_add_i32 s1, s2, s3") is None and im.classify("ds_read_b32 v1, v2") is None
    for kernel, words in (([10, 11, 3, 4], 10), ([10, 10, 3, 4], 10)):
        m = im.analyse(obj, kernel, 4)
        per_shift = m["per_shift"]["full_rate"] + m["per_shift"]["sgpr_operand"] + m["per_shift"]["half_rate"]
        assert 120 <= per_shift <= 145, per_shift
        assert m["per_shift"]["sgpr_operand"] >= 2 * words            # the column's two bit planes per word
        # (a copy whose s_setprio sits behind its body in the listing is not paired: 8 of the 10 are found)
        assert m["trip_copies"] >= 7 and 50 <= m["trip"]["full_rate"] + m["trip"]["sgpr_operand"] + m["trip"]["half_rate"] <= 90
        assert m["trip"]["half_rate"] > m["trip"]["full_rate"] * 0.8   # the trips are where the half-rate opcodes are
        assert 8 <= m["trip"]["lds"] <= 18 and m["trip"]["vmem"] == 1   # ... and the LDS instructions (5.8 cycles each, round 5)
        assert m["trip"]["cycles_all"] > 2.0 * (m["trip"]["full_rate"] + m["trip"]["sgpr_operand"] + m["trip"]["half_rate"])
