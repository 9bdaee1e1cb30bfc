"""Time per-base importance (gkmpredict.explain) at gkmQC's shape: train on 5 000 + 5 000 peak-like 600-bp sequences
(L=10 k=6 d=3, weighted kernel type 4) and explain 1 000 held-out queries.

    python tools/explain_throughput.py [--n-train 5000 --n-query 1000 --block 0 --json out.json]

Prints queries/s, the explain kernel's milliseconds (HIP events around k_explain, summed over the blocks of a second, instrumented call), its l-mer
comparisons/s, and its share of the wall time of the explain call."""
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
    ap.add_argument("--n-query", type=int, default=1000)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--block", type=int, default=0, help="queries per block (0: gkmpredict.default_explain_block)")
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

    t0 = time.perf_counter()
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    print("train: %.2f s, %d SVs of %d" % (time.perf_counter() - t0, model.n_sv, 2 * a.n_train), flush=True)
    block = a.block or gp.default_explain_block(a.length)
    gp.explain(model, dv.FlatSequences(codes[:a.length * 4], off[:5]))     # warm-up: context, first launch
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    _, E = gp.explain(model, queries, block=block)
    wall_s = time.perf_counter() - t0
    blocks = []                                                            # the same again, instrumented per block
    _, E2 = gp.explain(model, queries, block=block, on_block=blocks.append)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(E, E2))
    explain_ms = sum(b["explain_kernel_ms"] for b in blocks)
    comparisons = sum(b["comparisons"] for b in blocks)
    _, scores = gp.score(model, queries)
    worst = max(abs(e.sum() - (s - model.rho)) for e, s in zip(E, scores)) / np.abs(model.dual_coef()).sum()
    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, n_query=a.n_query, length=a.length, block=block,
               blocks=len(blocks), wall_s=wall_s, queries_per_s=a.n_query / wall_s, explain_kernel_ms=explain_ms,
               kernel=blocks[0]["kernel"], comparisons=comparisons, comparisons_per_s=comparisons / (explain_ms / 1e3),
               kernel_share_of_wall=explain_ms / 1e3 / wall_s, completeness_worst_rel=worst)
    print("explain: %d queries x %d SVs in %.2f s = %.1f queries/s (block %d); k_explain %.1f ms = %.3g l-mer "
          "comparisons/s, %.1f %% of the wall time; completeness error <= %.2g x sum |dual_coef|"
          % (a.n_query, model.n_sv, wall_s, a.n_query / wall_s, block, explain_ms, comparisons / (explain_ms / 1e3),
             100 * explain_ms / 1e3 / wall_s, worst))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
