"""Time in-silico mutagenesis (gkmpredict.ism) at gkmQC's shape: train on 5 000 + 5 000 peak-like 600-bp sequences
(L=10 k=6 d=3, weighted kernel type 4), run ISM on held-out queries, and score every single-base mutant of the first
--n-brute of them through `score` (brute force) in the same run.

    python tools/ism_throughput.py [--n-train 5000 --n-query 200 --n-brute 20 --block 0 --json out.json]

Prints ISM ms per query (for all the queries, and for the brute-force queries alone), k_ism's milliseconds (HIP events,
summed over the blocks of a second, instrumented call) and its share of the wall time, the self-profile kernels'
milliseconds, brute-force ms per query, the speed-up, and the worst difference between the two."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=5000, help="positives and as many negatives (default: 5000)")
    ap.add_argument("--n-query", type=int, default=200)
    ap.add_argument("--n-brute", type=int, default=20, help="queries scored mutant by mutant (default: 20)")
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--block", type=int, default=0, help="queries per block (0: gkmpredict.default_ism_block)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    tmp = tempfile.mkdtemp()
    pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    synth.write_peak_problem(pf, nf, a.n_train, a.n_train, a.length)
    qs = synth.make_peak_sequences(41, a.n_query // 2, a.length, True) + \
        synth.make_peak_sequences(42, a.n_query - a.n_query // 2, a.length, False)
    codes = dv.encode(b"".join(qs))
    off = np.arange(len(qs) + 1, dtype=np.int64) * a.length
    queries = dv.FlatSequences(codes, off)
    nb = min(a.n_brute, a.n_query)
    brute_q = [np.array(queries[i]) for i in range(nb)]

    t0 = time.perf_counter()
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    print("train: %.2f s, %d SVs of %d" % (time.perf_counter() - t0, model.n_sv, 2 * a.n_train), flush=True)
    block = a.block or gp.default_ism_block(a.length, model.d)
    gp.ism(model, dv.FlatSequences(codes[:a.length * 2], off[:3]))        # warm-up: context, first launches
    gp.score(model, brute_q[:2])
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    _, I = gp.ism(model, queries, block=block)
    wall_s = time.perf_counter() - t0
    blocks = []                                                            # the same again, instrumented per block
    _, I2 = gp.ism(model, queries, block=block, on_block=blocks.append)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(I, I2))
    ism_ms = sum(b["ism_kernel_ms"] for b in blocks)
    self_ms = sum(b["self_kernels_ms"] for b in blocks)
    comparisons = sum(b["comparisons"] for b in blocks)

    t0 = time.perf_counter()
    _, Ib = gp.ism(model, brute_q)
    wall_small_s = time.perf_counter() - t0

    t0 = time.perf_counter()                                               # brute force: every mutant through score
    mutants, index = [], []
    for qi, x in enumerate(brute_q):
        for t in range(len(x)):
            for b in range(4):
                if b != x[t]:
                    y = x.copy()
                    y[t] = b
                    mutants.append(y)
                    index.append((qi, t, b))
    _, sx = gp.score(model, brute_q)
    _, sy = gp.score(model, mutants)
    brute = [np.zeros((len(x), 4)) for x in brute_q]
    for (qi, t, b), s in zip(index, sy):
        brute[qi][t, b] = s - sx[qi]
    brute_s = time.perf_counter() - t0
    worst = max(np.abs(x - y).max() for x, y in zip(Ib, brute)) / np.abs(model.dual_coef()).sum()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(Ib, I[:nb]))

    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, n_query=a.n_query, length=a.length, block=block,
               blocks=len(blocks), wall_s=wall_s, ism_ms_per_query=wall_s * 1e3 / a.n_query, ism_kernel_ms=ism_ms,
               kernel=blocks[0]["kernel"], comparisons=comparisons, comparisons_per_s=comparisons / (ism_ms / 1e3),
               kernel_share_of_wall=ism_ms / 1e3 / wall_s, self_kernels_ms=self_ms, n_brute=nb,
               n_mutants=len(mutants), ism_small_ms_per_query=wall_small_s * 1e3 / nb,
               brute_ms_per_query=brute_s * 1e3 / nb, speedup=(brute_s / nb) / (wall_s / a.n_query),
               speedup_same_queries=brute_s / wall_small_s, worst_rel_to_brute=worst)
    print("ism: %d queries x %d SVs in %.2f s = %.2f ms per query (block %d); k_ism %.1f ms = %.3g l-mer comparisons/s, "
          "%.1f %% of the wall time; self profiles %.1f ms" % (a.n_query, model.n_sv, wall_s, wall_s * 1e3 / a.n_query,
                                                              block, ism_ms, comparisons / (ism_ms / 1e3),
                                                              100 * ism_ms / 1e3 / wall_s, self_ms))
    print("brute force: %d queries, %d mutants through score in %.2f s = %.1f ms per query; ism of the same %d queries "
          "alone %.2f ms per query; speed-up %.1fx (%.1fx on the same queries); worst difference %.2g x sum |dual_coef|"
          % (nb, len(mutants), brute_s, brute_s * 1e3 / nb, nb, wall_small_s * 1e3 / nb, out["speedup"],
             out["speedup_same_queries"], worst))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
