"""Randomised parity sweep on the GPU box: random (kernel type, L, k, d, M, H), random length
distributions (fixed, ragged, minimal, duplicates, poly-A), random row subsets -- integer
mismatch profiles and K of the device layer against the CPU oracle (test infrastructure).
python tools/fuzz_parity.py [--seconds 240] [--seed 1] [--region whole]

--region whole: outside the bit-sliced table the draw covers every legal tuple -- L in 2..12, k in 0..L, d in 0..L-k, so
d up to L -- where the default stops at d <= 4, L >= 3, k >= 1.  The last line counts the cases with d >= 5 outside the
bit-sliced table: the ones only k_gram_direct serves."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


from tests.helpers import ALL_LD as BITSLICED   # noqa: E402  every (L, d) with a bit-sliced kernel


def band(L, lanes):
    """(lo, hi): the lengths at which rows of one length take `lanes` lanes each, one resident piece per lane, and share
    none -- where a same-length problem runs the one-piece-per-lane variants.  lanes - 1 full lanes
    of `cap` windows, and a last piece that owns at most `cap` and leaves too few bit rows for the next row to start
    in (its first piece would own fewer than 30 windows).  tests/test_same_length_plan_host.py holds this against the
    packing for every length and L."""
    cap = (320 - (L - 1)) // 5 * 5
    spare = 1
    while (spare * 10 - (L - 1)) // 5 * 5 < 30:
        spare += 1
    return (lanes - 1) * cap + (32 - spare) * 10 + 1, lanes * cap + L - 1


def band_length(rng, L):
    """A fixed length at which rows of l-mer length L keep one resident piece per lane: one lane half of the time -- with riders up
    to 300 bp -- two to six lanes otherwise, the band's edges and the first length outside it now and then."""
    lanes = 1 if rng.random() < 0.5 else int(rng.integers(2, 7))
    lo, hi = band(L, lanes)
    return int(rng.choice([int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)), lo, hi, lo - 1, hi + 1, 300]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--region", choices=("default", "whole"), default="default")
    a = ap.parse_args()
    import torch  # noqa: F401
    from gkmqc_amd import device, synth
    from oracle import oracle as O
    rng = np.random.default_rng(a.seed)
    tmp = tempfile.mkdtemp()
    pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    t_end = time.time() + a.seconds
    cases = 0
    high_d = 0        # cases with d >= 5 and no bit-sliced kernel
    kernels = {}
    while time.time() < t_end:
        t = int(rng.integers(0, 6))
        if rng.random() < 0.75:   # (L, d) pairs with a bit-sliced instantiation
            L, d = BITSLICED[int(rng.integers(len(BITSLICED)))]
            k = int(rng.integers(1, L - d + 1))
        elif a.region == "whole":
            L = int(rng.integers(2, 13))
            k = int(rng.integers(0, L + 1))
            d = int(rng.integers(0, L - k + 1))
        else:
            L = int(rng.integers(3, 13))
            k = int(rng.integers(1, L + 1))
            d = int(rng.integers(0, min(4, L - k) + 1))
        if device.check_parameters(t, L, k, d):
            continue
        M, H = int(rng.integers(1, 256)), float(rng.integers(1, 200))
        gamma = float(rng.choice([0.5, 1.0, 2.0]))
        mode = int(rng.choice([0, 0, 5, 5, 5, 1, 2, 3, 4]))
        n = int(rng.integers(2, 90))
        if mode == 0:
            lens = np.full(n, int(rng.integers(L, 700)))
        elif mode == 5:   # fixed lengths inside (or just outside) a band: the one-piece-per-lane kernel variants
            length = min(band_length(rng, L), 2047)
            if length <= 320 and rng.random() < 0.3:
                n = int(rng.integers(130, 200))     # more than one tile with riders
            elif length > 700:
                n = int(rng.integers(2, 40))        # (the oracle's time)
            lens = np.full(n, max(length, L))
        elif mode == 1:
            lens = rng.integers(L, 700, n)
        elif mode == 2:
            lens = rng.integers(L, L + 12, n)
        elif mode == 3:
            lens = rng.choice([150, 300, 320, 321, 640, 2047], n)
        else:
            lens = rng.integers(L, 2048, n)
        seqs = [letters[rng.integers(0, 4, int(ln))].tobytes() for ln in lens]
        if n > 4:
            seqs[1] = seqs[0]                                  # duplicate
            seqs[2] = b"A" * len(seqs[2])                      # poly-A
            seqs[3] = bytes(reversed(seqs[0].translate(bytes.maketrans(b"ACGT", b"TGCA"))))  # reverse complement
        n_pos = max(1, n // 2)
        synth.write_fasta(pf, seqs[:n_pos], "p")
        synth.write_fasta(nf, seqs[n_pos:], "n")
        opt = O.make_opt(t, L, k, d, M, H, gamma, pf, nf)
        ref = O.gram(opt, want_profiles=True, nthreads=16)
        codes = [device.encode(s) for s in seqs]
        kerns = [device.KERNEL_AUTO, device.KERNEL_DIRECT]
        if (L, d) in BITSLICED:   # whatever `auto` makes of the pair: both record kinds of the bit-sliced kernel
            kerns += [device.KERNEL_BITSLICE, device.KERNEL_BITSLICE_GROUPS]
        for kern in kerns:
            res = device.gram_matrix(codes, t, L, k, d, M, H, gamma, want_profiles=True, kernel=kern)
            K = res["K"].cpu().numpy()
            P = res["P"].cpu().numpy()
            il = np.tril_indices(n)
            if not (P[il] == ref["P"][il]).all():
                raise SystemExit("PROFILE MISMATCH t=%d L=%d k=%d d=%d n=%d mode=%d kernel=%s PK %d seed=%d case=%d" %
                                 (t, L, k, d, n, mode, res["kernel"], res["variant"], a.seed, cases))
            # (a poly-A row with large weights wraps its int32 self profile -- like the reference -- and
            #  its square root is NaN on both sides: NaNs must coincide, the rest must agree)
            kd, kr = K[il], ref["K"][il]
            fin = np.isfinite(kr)
            same_nan = np.array_equal(np.isnan(kd), np.isnan(kr))
            err = (np.abs(kd[fin] - kr[fin]).max() / max(1e-300, np.abs(kr[fin]).max())) if fin.any() else 0.0
            tol = 1e-9 if t in (3, 5) else 1e-12
            if not (same_nan and err < tol):
                raise SystemExit("K MISMATCH %g t=%d L=%d k=%d d=%d n=%d mode=%d kernel=%s" % (err, t, L, k, d, n, mode, res["kernel"]))
            used = "%s PK %d" % (res["kernel"], res["variant"])
            kernels[used] = kernels.get(used, 0) + 1
        cases += 1
        high_d += int(d >= 5 and (L, d) not in BITSLICED)
        if cases % 50 == 0:
            print("%d cases ok %s" % (cases, kernels), flush=True)
    print("fuzz ok: %d cases, %d with d >= 5 outside the bit-sliced table, kernels used: %s" % (cases, high_d, kernels))


if __name__ == "__main__":
    main()
