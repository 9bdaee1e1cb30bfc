"""Time the boxed SVM solver entries (a bound per problem and per class: gkmsvm_train_batch_boxed /
gkmsvm_train_batch_general_boxed) at config 2's cross-validation shape -- 5 folds of 8 000 from the
10 000 x 10 000 matrix of tools/svm_bench.py (5 000 + 5 000 sequences of 300 bp, type 4, L=11 k=7 d=3) -- in one process
on one GPU:

    unboxed  svmcv.crossValidate through this library        vs  through --parent-lib (the parent commit's library)
    box      train_folds, box (C, C) per problem (boxed)     vs  train_folds, scalar C (unboxed): same iterations, same bits,
             so the ratio is the per-iteration cost of a bound per class -- k_smo, k_smo_general, k_smo_general + shrinking
    grid     cross_validate_grid over --grid-Cs x 5 folds    vs  the loop of one crossValidate per C on the same matrix

    python tools/svm_box_throughput.py [--parent-lib path/to/gkmkern_pylib.so --repeats 3 --grid-Cs 0.01,0.1,1,10,100,1000
                                        --only unboxed,box,grid --out profiles/svm_box_throughput.txt]

Per comparison: one warm-up of either side, then `--repeats` timed rounds, each round one side and then the other
(interleaved); reported per side the median wall time (a host clock around calls that end with their results on the
host) and its spread (max - min over the rounds).  Every round checks that the two sides returned equal results before
its times count.  The grid's one launch is made once before its rounds and its iteration counts printed; a C at which a
fold stops at the solver's iteration cap is left out of the comparison (both sides would re-solve it with scikit-learn
on the host) and named."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def verdict(a, b, sa, sb):
    if a + sa < b - sb:
        return "first cheaper"
    if b + sb < a - sa:
        return "second cheaper"
    return "inside the run-to-run spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-pos", type=int, default=5000)
    ap.add_argument("--n-neg", type=int, default=5000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid-Cs", default="0.01,0.1,1,10,100,1000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="unboxed,box,grid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import gkmsvm, svmcv, synth
    only = a.only.split(",")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    tmp = tempfile.mkdtemp(prefix="svm_box_")
    pos, neg = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    ps = synth.make_sequences(1, a.n_pos, a.length)
    ns = synth.make_sequences(2, a.n_neg, a.length)
    rng = np.random.default_rng(5)
    motifs = [b"TGACTCAGCA", b"GGGCGGGGCC", b"CACGTGACCA"]
    for i in range(a.n_pos):                     # tools/svm_bench.py's signal: one of three motifs in half the positives
        if rng.random() < 0.5:
            m = motifs[int(rng.integers(3))]
            at = int(rng.integers(0, a.length - len(m)))
            ps[i] = ps[i][:at] + m + ps[i][at + len(m):]
    synth.write_fasta(pos, ps, "p")
    synth.write_fasta(neg, ns, "n")
    K, n_pos, n_neg = gkmsvm.computeGkmKernel([4, 11, 7, 3, 50, 50, 1.0, pos, neg, 16, 0], resident=True)
    torch.cuda.synchronize()
    NCV, SEED, TOL = 5, 7, 1e-3
    args_svm = [1.0, TOL, 0, 512, NCV, 1, 0, SEED, 5]
    plan = svmcv.plan_folds(args_svm, n_pos, n_neg)
    y, trains = plan["y"], plan["u_trains"]
    say("svm_box_throughput: %d + %d sequences of %d bp, type 4 L=11 k=7 d=3; %d folds of %d; tol %g; %d timed rounds after "
        "one warm-up, interleaved; %s" % (n_pos, n_neg, a.length, len(trains), len(trains[0]), TOL, a.repeats,
                                          torch.cuda.get_device_name(0)))

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return r, time.perf_counter() - t0

    def rounds(first, second, same, repeats=None):
        r1, r2 = first(), second()
        if not same(r1, r2):
            return None
        w1, w2 = [], []
        for _ in range(repeats or a.repeats):
            r1, t1 = timed(first)
            r2, t2 = timed(second)
            if not same(r1, r2):
                return None
            w1.append(t1)
            w2.append(t2)
        return np.median(w1), np.ptp(w1), np.median(w2), np.ptp(w2)

    def report(what, one, two, res, extra=""):
        if res is None:
            say("%s: THE TWO SIDES RETURNED DIFFERENT RESULTS -- no times" % what)
            return
        m1, s1, m2, s2 = res
        say("%s: %s %8.4f s (spread %.4f) | %s %8.4f s (spread %.4f) | %s / %s %6.3f, %s; results equal every round%s"
            % (what, one, m1, s1, two, m2, s2, one, two, m1 / m2, verdict(m1, m2, s1, s2), extra))

    # ---------------------------------------------------------------- the unboxed path against the parent's library
    if "unboxed" in only:
        if a.parent_lib is None:
            say("unboxed: no --parent-lib given, comparison skipped")
        else:
            here = svmcv._lib()
            parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
            for name in ("gkmsvm_train_batch", "gkmsvm_train_batch_general", "gkmsvm_decision_batch", "gkmsvm_last_error"):
                getattr(parent, name).restype = getattr(here, name).restype
                getattr(parent, name).argtypes = getattr(here, name).argtypes
            real = svmcv._lib

            def through(lib):
                def run():
                    svmcv._lib = lambda: lib
                    try:
                        return svmcv.crossValidate(args_svm, K, n_pos, n_neg, plan=plan)
                    finally:
                        svmcv._lib = real
                return run
            res = rounds(through(here), through(parent), lambda x, y: x == y)
            report("unboxed  crossValidate C=1, 5 x %d" % len(trains[0]), "this library", "parent's library", res)

    # ---------------------------------------------------------------- what a bound per class costs
    if "box" in only:
        def same_sol(x, y):
            return (list(x.iters) == list(y.iters) and x.rho.tobytes() == y.rho.tobytes()
                    and all(p.tobytes() == q.tobytes() for p, q in zip(x.alpha, y.alpha))
                    and all(p.tobytes() == q.tobytes() for p, q in zip(x.grad, y.grad)))
        fast = svmcv.FAST_FOLD_SAMPLES
        for what, limit, shrinking in (("k_smo", fast, False), ("k_smo_general", 0, False),
                                       ("k_smo_general + shrinking", fast, True)):
            svmcv.FAST_FOLD_SAMPLES = limit
            try:
                its = []

                def boxed():
                    sol = svmcv.train_folds(K, trains, y, [1.0] * len(trains), TOL, shrinking)[0]
                    its[:] = [int(i) for i in sol.iters]
                    return sol
                res = rounds(boxed, lambda: svmcv.train_folds(K, trains, y, 1.0, TOL, shrinking)[0], same_sol)
            finally:
                svmcv.FAST_FOLD_SAMPLES = fast
            report("box      %-26s C=1" % what, "boxed (C, C)", "unboxed", res, "; iterations %s" % its)

    # ---------------------------------------------------------------- what the grid buys
    if "grid" in only:
        Cs = [float(x) for x in a.grid_Cs.split(",")]
        labels = [y[t] for t in trains]
        t0 = time.perf_counter()
        sol, _ = svmcv.train_tasks(K, [t for _ in Cs for t in trains], [lab for _ in Cs for lab in labels],
                                   [C for C in Cs for _ in trains], TOL, False)
        t1 = time.perf_counter() - t0
        its = np.asarray(sol.iters).reshape(len(Cs), len(trains))
        say("grid     one launch of %d problems (%d C x %d folds): %.4f s; iterations per C: %s"
            % (its.size, len(Cs), len(trains), t1, ", ".join("%g: %d..%d" % (C, abs(r).min(), abs(r).max())
                                                             for C, r in zip(Cs, its))))
        capped = [C for C, r in zip(Cs, its) if (r < 0).any()]
        if capped:
            say("grid     C = %s: a fold stops at the iteration cap; left out of the comparison" % capped)
        Cs = [C for C in Cs if C not in capped]

        def grid():
            return [(r["auc_mean"], r["auc_std"]) for r in
                    svmcv.cross_validate_grid(K, n_pos, n_neg, Cs, (None,), NCV, 1, SEED, TOL)]

        def loop():
            return [svmcv.crossValidate([C] + args_svm[1:], K, n_pos, n_neg, plan=plan) for C in Cs]
        per_C = []
        for C in Cs:
            _, t = timed(lambda: svmcv.crossValidate([C] + args_svm[1:], K, n_pos, n_neg, plan=plan))
            per_C.append(t)
        say("grid     crossValidate alone per C (one timed call each, after the launch above): %s"
            % ", ".join("%g: %.4f s" % (C, t) for C, t in zip(Cs, per_C)))
        res = rounds(grid, loop, lambda x, y: [tuple(map(float, p)) for p in x] == [tuple(map(float, p)) for p in y])
        report("grid     %d values of C x %d folds" % (len(Cs), len(trains)), "cross_validate_grid",
               "loop of crossValidate", res, "; slowest single C %.4f s, sum %.4f s" % (max(per_C), sum(per_C)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
