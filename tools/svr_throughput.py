"""Time epsilon-SVR training (gkmqc_amd/svmcv.py train_svr_folds, gkmqc_amd/gkmmodel.py train_svr) at gkmQC's shape:
600-bp peak-like sequences, L=10 k=6 d=3, weighted kernel (type 4), synthetic targets (class, GC content, noise).

    python tools/svr_throughput.py [--n 10000 --n-small 8000 --length 600 --no-sklearn --json out.json]

Prints the Gram matrix's milliseconds, then for `--n` sequences (2l = 20 000 solver positions: the general solver) and
`--n-small` (2l = 16 000: k_smo) the solver's milliseconds and iterations, and scikit-learn's SVR.fit on the host copy of
the same matrix for comparison (same coefficients: checked)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000, help="sequences (default: 10000)")
    ap.add_argument("--n-small", type=int, default=8000, help="sequences of the k_smo run (default: 8000)")
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--no-sklearn", action="store_true", help="skip scikit-learn's SVR.fit")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import svmcv
    from gkmqc_amd import synth
    half = a.n // 2
    qs = synth.make_peak_sequences(41, half, a.length, True) + synth.make_peak_sequences(42, a.n - half, a.length, False)
    codes = dv.encode(b"".join(qs))
    seqs = dv.FlatSequences(codes, np.arange(a.n + 1, dtype=np.int64) * a.length)
    gc = ((codes == 1) | (codes == 2)).reshape(a.n, a.length).mean(1)
    z = np.where(np.arange(a.n) < half, 1.0, 0.0) + 2.0 * gc + 0.1 * np.random.default_rng(5).normal(size=a.n)

    dv.gram_matrix(dv.FlatSequences(codes[:64 * a.length], seqs.off[:65]), 4, 10, 6, 3, symmetric=True)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = dv.gram_matrix(seqs, 4, 10, 6, 3, symmetric=True)
    K = res["K"]
    torch.cuda.synchronize()
    gram_ms = (time.perf_counter() - t0) * 1e3
    print("gram: %d x %d, %.1f ms" % (a.n, a.n, gram_ms), flush=True)
    svmcv.train_svr_folds(K, [np.arange(64)], z, a.C, a.epsilon)          # warm-up (both solvers' first launch)
    svmcv.train_svr_folds(K, [np.arange(64)], z, a.C, a.epsilon, shrinking=True)
    Kh = K.cpu().numpy() if not a.no_sklearn else None
    out = dict(n=a.n, length=a.length, gram_ms=gram_ms, runs=[])
    for n in (a.n, a.n_small):
        train = np.arange(n) if n == a.n else np.concatenate((np.arange(n // 2), half + np.arange(n - n // 2)))
        solver = "k_smo_general" if 2 * n > svmcv.FAST_FOLD_SAMPLES else "k_smo"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = svmcv.train_svr_folds(K, [train], z, a.C, a.epsilon)
        ms = (time.perf_counter() - t0) * 1e3
        run = dict(sequences=n, positions=2 * n, solver=solver, solver_ms=ms, iterations=int(sol.iters[0]),
                   n_sv=len(sol.support[0]))
        line = "%s: %d sequences (2l = %d), %.1f ms, %d iterations, %d SVs" % (solver, n, 2 * n, ms, sol.iters[0],
                                                                              len(sol.support[0]))
        if Kh is not None:
            from sklearn.svm import SVR
            kt = Kh[np.ix_(train, train)]
            t0 = time.perf_counter()
            m = SVR(kernel="precomputed", C=a.C, epsilon=a.epsilon, tol=1e-3, shrinking=False, cache_size=2000)
            m.fit(kt, z[train])
            run["sklearn_ms"] = (time.perf_counter() - t0) * 1e3
            run["sklearn_iterations"] = int(np.ravel(m.n_iter_)[0])
            run["identical"] = bool(np.array_equal(m.support_, sol.support[0])
                                    and m.dual_coef_[0].tobytes() == sol.dual_coef[0].tobytes()
                                    and m.intercept_[0] == sol.intercept[0])
            line += "; scikit-learn SVR.fit %.0f ms (%d iterations), identical: %s" % (
                run["sklearn_ms"], run["sklearn_iterations"], run["identical"])
        print(line, flush=True)
        out["runs"].append(run)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
