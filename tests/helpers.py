"""Shared helpers for the test-suite (test infrastructure; may use the oracle)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

QUIRK_POS = os.path.join(GOLDEN, "quirks_pos.fa")
QUIRK_NEG = os.path.join(GOLDEN, "quirks_neg.fa")
REGION_POS = os.path.join(GOLDEN, "region_pos.fa")
REGION_NEG = os.path.join(GOLDEN, "region_neg.fa")


def golden_weights():
    raw = json.load(open(os.path.join(GOLDEN, "mismatch_weights.json")))
    return {tuple(int(x) for x in k.split(",")): np.array([float.fromhex(v) for v in vals])
            for k, vals in raw.items()}


def quirks_expected():
    z = np.load(os.path.join(GOLDEN, "quirks_expected.npz"))
    cases = []
    i = 0
    while "q%d_params" % i in z:
        t, L, k, d, M, H, g = z["q%d_params" % i]
        cases.append(dict(idx=i, kernel_type=int(t), L=int(L), k=int(k), d=int(d), M=int(M), H=float(H),
                          gamma=float(g), P=z["q%d_P" % i], sqnorm=z["q%d_sqnorm" % i], K=z["q%d_K" % i],
                          wt=z["q%d_wt" % i]))
        i += 1
    return cases, z["lens"], int(z["n_pos"])


def region_expected():
    """tests/golden/region_expected.npz: the reference on the 20 sequences of region_pos.fa + region_neg.fa over the whole
    legal (L, k, d) region (tests/golden/make_golden.py --only-region).  -> (cases, lens, n_pos, weights): cases as
    quirks_expected() gives them, K and sqnorm None where the reference has no defined value (L = 12, k = 0, d = 12);
    weights maps each of the 528 (kernel_type, L, k) to the reference's c_0 .. c_{L-k}."""
    z = np.load(os.path.join(GOLDEN, "region_expected.npz"))
    lens = z["lens"]
    n = len(lens)
    il = np.tril_indices(n)
    cases, at = [], 0
    for i, (t, L, k, d, M, H, g) in enumerate(z["params"]):
        d = int(d)
        P = np.zeros((n, n, d + 1), dtype=np.int32)
        P[il] = z["P"][at: at + len(il[0]) * (d + 1)].reshape(-1, d + 1)
        at += len(il[0]) * (d + 1)
        has = bool(z["has_K"][i])
        cases.append(dict(idx=i, kernel_type=int(t), L=int(L), k=int(k), d=d, M=int(M), H=float(H), gamma=float(g), P=P,
                          sqnorm=z["sqnorm"][i] if has else None, K=z["K"][i] if has else None, wt=z["wt"][i]))
    assert at == len(z["P"])
    weights = {tuple(int(x) for x in tlk): w[: tlk[1] - tlk[2] + 1] for tlk, w in zip(z["weights_tlk"], z["weights"])}
    return cases, lens, int(z["n_pos"].reshape(-1)[0]), weights


def same_nonfinite_rel_err(a, b):
    """(NaN and infinity in the same cells of a and b, the largest per-element relative error of b's finite cells) -- a
    type with negative c_m can give a negative squared norm, whose root is NaN in the reference too"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    inf = ~fin & ~np.isnan(b)
    same = bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[inf], b[inf]))
    return same, max_rel_err(a[fin], b[fin])


def synthetic_expected():
    return np.load(os.path.join(GOLDEN, "synthetic_expected.npz"))


def tril_unpack(vec, n):
    K = np.zeros((n, n))
    i, j = np.tril_indices(n, -1)
    K[i, j] = vec
    return K


def tril_pack(K):
    i, j = np.tril_indices(K.shape[0], -1)
    return K[i, j]


def max_rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    denom = np.maximum(np.abs(b), 1e-300)
    return float(np.max(np.abs(a - b) / denom)) if a.size else 0.0


def synth_codes(n_pos, n_neg, length=300, length_range=None):
    """The synthetic problem of bench.py / the golden generator as base-code arrays."""
    from gkmqc_amd import synth
    from gkmqc_amd.device import encode
    pos = synth.make_sequences(1, n_pos, length, length_range)
    neg = synth.make_sequences(2, n_neg, length, length_range)
    return [encode(s) for s in pos + neg]


def ragged_expected():
    """tests/golden/ragged_expected.npz: a small ragged problem through the reference's profiles and gkm_main_pywrapper
    (tests/golden/make_golden.py --only-ragged).  -> (files, cases): files maps "pos" / "neg" to the arguments of
    synth.make_sequences; each case holds the parameters, P over the lower triangle with the diagonal (row-major) and K
    over the strict lower triangle."""
    z = np.load(os.path.join(GOLDEN, "ragged_expected.npz"))
    files = {}
    for name in ("pos", "neg"):
        seed, n, ln, lo, hi, ls = (int(x) for x in z[name + "_cfg"])
        files[name] = (seed, n, ln, (lo, hi), ls)
    cases = []
    i = 0
    while "p%d_params" % i in z:
        t, L, k, d, M, H, g = z["p%d_params" % i]
        cases.append(dict(kernel_type=int(t), L=int(L), k=int(k), d=int(d), M=int(M), H=float(H), gamma=float(g),
                          P=z["p%d_P" % i], K=z["p%d_K" % i]))
        i += 1
    return files, cases


def batch_rows_expected():
    """tests/golden/batch_rows_expected.npz: the reference's gkmkernel_kernelfunc_batch (src/libgkm.c:1115-1153) driven
    by tests/golden/make_golden.py --only-batch.  -> list of dict(name, n_support, n_query, length, length_range,
    kernel_type, L, k, d, M, H, gamma, K[n_query, n])."""
    z = np.load(os.path.join(GOLDEN, "batch_rows_expected.npz"))
    cases = []
    for key in z.files:
        if not key.endswith("_cfg"):
            continue
        name = key[:-4]
        nsup, nq, ln, lo, hi = (int(x) for x in z[key])
        i = 0
        while "%s_p%d_params" % (name, i) in z:
            t, L, k, d, M, H, g = z["%s_p%d_params" % (name, i)]
            cases.append(dict(name="%s_p%d" % (name, i), n_support=nsup, n_query=nq, length=ln or 300,
                              length_range=(lo, hi) if hi else None, kernel_type=int(t), L=int(L), k=int(k), d=int(d),
                              M=int(M), H=float(H), gamma=float(g), K=z["%s_p%d_K" % (name, i)]))
            i += 1
    return cases


# every (L, d) the bit-sliced Gram kernel is instantiated for (the instantiation table of gkmqc_amd/csrc/gkm_gram_bitslice.hip)
ALL_LD = [(L, d) for L in range(5, 13) for d in range(0, 5)] + [(11, 5), (12, 5), (12, 6)]


def raw_from_profiles(P, c):
    """Raw G(a, j) = sum_m c_m P_m(a, j), ascending m from 0.0 -- the Gram kernels' accumulation order."""
    G = np.zeros(P.shape[:2])
    for m in range(P.shape[2]):
        G = G + c[m] * P[:, :, m].astype(np.float64)
    return G


def oracle_raw(O, t, L, k, d, pf, nf):
    """Raw G(a, j) for every pair of the problem in pf + nf through the CPU oracle."""
    r = O.gram(O.make_opt(t, L, k, d, posfile=pf, negfile=nf, nthreads=8), want_profiles=True)
    P = r["P"]
    i, j = np.triu_indices(r["n"], 1)
    P[i, j] = P[j, i]
    return raw_from_profiles(P, O.mismatch_weights(t, L, k)[: d + 1])


def oracle_problem(seqs, params):
    """The CPU oracle on a list of base-code arrays (at least two), params = (t, L, k, d, M, H, gamma)
    -> dict(P [n, n, d + 1], G raw, K), all symmetric."""
    import tempfile
    from oracle import oracle as O
    t, L, k, d, M, H, gamma = params
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
        half = max(1, len(seqs) // 2)          # (the oracle's reader wants both files non-empty)
        for path, part in ((pf, seqs[:half]), (nf, seqs[half:])):
            with open(path, "wb") as f:
                for i, s in enumerate(part):
                    f.write(b">s%d\n" % i + letters[np.asarray(s)].tobytes() + b"\n")
        r = O.gram(O.make_opt(t, L, k, d, M, H, gamma, pf, nf), want_profiles=True, nthreads=8)
    n = r["n"]
    assert n == len(seqs)
    P, K = r["P"], r["K"]
    i, j = np.triu_indices(n, 1)
    P[i, j] = P[j, i]
    K[i, j] = K[j, i]
    return dict(P=P, G=raw_from_profiles(P, O.mismatch_weights(t, L, k)[: d + 1]), K=K)


def oracle_cells(seqs, rows, cols, params):
    """Oracle raw G and K at [rows][:, cols] of the problem `seqs`, from the oracle run on only the sequences these
    cells name (a cell depends on its two sequences alone: tests/test_oracle_golden.py pins that)."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    sub = np.unique(np.concatenate((rows, cols)))
    pick = list(sub) if len(sub) > 1 else [sub[0], sub[0]]
    r = oracle_problem([seqs[int(s)] for s in pick], params)
    at = {int(s): i for i, s in enumerate(sub)}
    ri = np.array([at[int(a)] for a in rows])
    ci = np.array([at[int(j)] for j in cols])
    return r["G"][np.ix_(ri, ci)], r["K"][np.ix_(ri, ci)]
