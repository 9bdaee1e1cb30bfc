"""Time fold_panel and train_panel (gkmqc_amd/gkmpanels.py) against the loops they replace, at gkmQC's
shape -- L=10 k=6 d=3, kernel type 4 -- in one process on one GPU:

    fold     fold_panel(models[:n])        vs  LmerPanel([lmer_weights(m) for m in models[:n]])      n = 1, 8, 20, 64
    train    train_panel(pool, n tasks)    vs  n x train(pos_t.fa, neg_t.fa)

    python tools/panel_fold_throughput.py [--models 1,8,20,64 --train-tasks 8 --repeats 3 --pos 5000 --neg 5000
                                           --length 600 --only fold,train --out profiles/panel_fold_throughput.txt]

The pool is synth.write_peak_problem's positives and negatives in one FASTA file; task t's label column takes a seeded
half of the positives as 1 and a seeded half of the negatives as 0, everything else `.`.  The models of the fold come
from one train_panel call over max(--models) tasks.  Per n: one warm-up of either side, then `--repeats` timed rounds,
each round the one call and then the whole loop (alternating the two sides).  Reported per side: the median wall time
(a host clock around calls that end with their results on the host) with its spread (max - min over the rounds); for
the fold also, from the last round, the kernels' milliseconds (HIP events summed over the pieces: k_panel_weights
against n x k_lmer_weights), the host's class sums (panel_classes; for the loop lmer_classes is timed on its own with
the model's norms, outside the rounds) and everything else (the norms' launches, uploads, the copy back, LmerPanel).
The claim under test is "a fold of n costs less than n single folds, beyond both sides' spreads": the ratio loop / fold
is printed with both spreads, and a line says plainly where it fails.  Every round checks the folded panel against the
loop's, bit for bit, and the train round the model files byte for byte."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def verdict(one, loop, s_one, s_loop, what):
    if one + s_one < loop - s_loop:
        return "%s cheaper" % what
    if loop + s_loop < one - s_one:
        return "loop cheaper: THE CLAIM FAILS HERE"
    return "inside the run-to-run spread: THE CLAIM IS NOT SHOWN HERE"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="1,8,20,64")
    ap.add_argument("--train-tasks", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pos", type=int, default=5000)
    ap.add_argument("--neg", type=int, default=5000)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--only", default="fold,train")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpanels as pn
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    KP = dict(kernel_type=4, L=10, k=6, d=3)
    sizes = [int(s) for s in a.models.split(",")]
    only = a.only.split(",")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    tmp = tempfile.mkdtemp(prefix="panel_fold_")
    pf, nf, pool = (os.path.join(tmp, x) for x in ("pos.fa", "neg.fa", "pool.fa"))
    synth.write_peak_problem(pf, nf, a.pos, a.neg, a.length)
    with open(pool, "wb") as out:
        for path in (pf, nf):
            with open(path, "rb") as f:
                out.write(f.read())
    seqs, names, _, _ = dv.read_fasta(pool)
    n_tasks = max(sizes + [a.train_tasks])
    Y = np.full((len(names), n_tasks), pn.NOT_IN_TASK, dtype=np.int8)
    for t in range(n_tasks):
        rng = np.random.default_rng(1000 + t)
        Y[rng.permutation(a.pos)[:a.pos // 2], t] = 1
        Y[a.pos + rng.permutation(a.neg)[:a.neg // 2], t] = 0
    tasks = ["task%d" % t for t in range(n_tasks)]
    say("panel_fold_throughput: L=10 k=6 d=3 type 4; pool %d + %d x %d bp, %d tasks of %d + %d records; %d timed rounds "
        "after one warm-up; %s" % (a.pos, a.neg, a.length, n_tasks, a.pos // 2, a.neg // 2, a.repeats,
                                   torch.cuda.get_device_name(0)))

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return r, time.perf_counter() - t0

    def rounds(one, loop, same):
        one(), loop()
        w1, w2 = [], []
        for _ in range(a.repeats):
            r1, t1 = timed(one)
            r2, t2 = timed(loop)
            w1.append(t1)
            w2.append(t2)
            ok = same(r1, r2)
        return np.median(w1), np.ptp(w1), np.median(w2), np.ptp(w2), ok

    if "train" in only:
        nt = a.train_tasks
        split = []
        for t in range(nt):
            files = []
            for lab, word in ((1, "pos"), (0, "neg")):
                path = os.path.join(tmp, "t%d_%s.fa" % (t, word))
                with open(path, "w") as f:
                    for i in np.flatnonzero(Y[:, t] == lab):
                        f.write(">%s\n%s\n" % (names[i], gp.codes_to_text(seqs[i])))
                files.append(path)
            split.append(files)

        def texts(models):
            out = []
            for m in models:
                m.save(os.path.join(tmp, "m.txt"))
                with open(os.path.join(tmp, "m.txt"), "rb") as f:
                    out.append(f.read())
            return out
        m1, s1, m2, s2, ok = rounds(lambda: pn.train_panel(pool, (tasks[:nt], Y[:, :nt]), **KP)[1],
                                    lambda: [gp.train(p, n, **KP) for p, n in split],
                                    lambda x, y: texts(x) == texts(y))
        say("train    n_tasks %2d: train_panel %8.4f s (spread %.4f) | loop of %2d train %8.4f s (spread %.4f) | loop / "
            "train_panel %5.2f, %s; model files equal: %s" % (nt, m1, s1, nt, m2, s2, m2 / m1,
                                                              verdict(m1, m2, s1, s2, "train_panel"), ok))

    if "fold" in only:
        _, models = pn.train_panel(pool, (tasks[:max(sizes)], Y[:, :max(sizes)]), **KP)
        say("models: %d, support vectors %d..%d" % (len(models), min(m.n_sv for m in models), max(m.n_sv for m in models)))
        for n in sizes:
            sub, nm = models[:n], ["m%d" % i for i in range(n)]
            ev1, ev2 = [], []

            def fold():
                del ev1[:]
                return pn.fold_panel(sub, nm, on_piece=ev1.append)

            def loop():
                del ev2[:]
                return gp.LmerPanel([gp.lmer_weights(m, on_piece=ev2.append) for m in sub], nm)
            m1, s1, m2, s2, ok = rounds(fold, loop, lambda x, y: x.W.tobytes() == y.W.tobytes()
                                        and x.rho.tobytes() == y.rho.tobytes())
            k1, k2 = sum(e["kernel_ms"] for e in ev1) / 1e3, sum(e["kernel_ms"] for e in ev2) / 1e3
            c1 = ev1[0]["classes_ms"] / 1e3
            # the loop's host classes: lmer_classes per model with norms of the right shape (their values do not change its cost)
            t0 = time.perf_counter()
            for m in sub:
                gp.lmer_classes(m, np.ones(m.n_sv))
            c2 = time.perf_counter() - t0
            say("fold     n_models %2d: fold_panel %8.4f s (spread %.4f; k_panel_weights %.4f, host classes %.4f = %2.0f %%, "
                "rest %.4f; %d classes) | loop of %2d %8.4f s (spread %.4f; k_lmer_weights %.4f, host classes %.4f = %2.0f "
                "%%, rest %.4f) | loop / fold %5.2f, %s; kernels loop / fold %5.2f; equal bits: %s"
                % (n, m1, s1, k1, c1, 100 * c1 / m1, m1 - k1 - c1, ev1[0]["classes"], n, m2, s2, k2, c2, 100 * c2 / m2,
                   m2 - k2 - c2, m2 / m1, verdict(m1, m2, s1, s2, "fold"), k2 / k1, ok))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
