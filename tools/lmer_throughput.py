"""Time l-mer weight tables (gkmqc_amd/gkmtables.py lmer_weights, score_with_table) at gkmQC's shape:
600-bp peak-like sequences, L=10 k=6 d=3, weighted kernel (type 4).

    python tools/lmer_throughput.py [--n-train 5000 --n-query 100000 --no-l12 --json out.json]

Prints the table build (host aggregation of the support vectors' l-mers, k_lmer_weights milliseconds from HIP events
summed over its pieces, comparisons/s, wall), scoring the queries from the table against `score` on the same queries
(queries/s each, worst |difference| / sum |dual_coef|), and one table build at L=12 from the same support vectors and
coefficients (L=12 k=6 d=3: the build's cost depends on the classes, not on how the model was trained)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(gp, model):
    pieces = []
    t0 = time.perf_counter()
    gp.lmer_classes(model, np.ones(model.n_sv))
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    tab = gp.lmer_weights(model, on_piece=pieces.append)
    wall_s = time.perf_counter() - t0
    kernel_ms = sum(p["kernel_ms"] for p in pieces)
    comparisons = sum(p["comparisons"] for p in pieces)
    return tab, dict(L=model.L, classes=pieces[0]["classes"], pieces=len(pieces), host_aggregation_s=host_s,
                     kernel_ms=kernel_ms, comparisons=comparisons, comparisons_per_s=comparisons / (kernel_ms / 1e3),
                     wall_s=wall_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=5000, help="positives and as many negatives (default: 5000)")
    ap.add_argument("--n-query", type=int, default=100000)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--no-l12", action="store_true", help="skip the L=12 build")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    tmp = tempfile.mkdtemp()
    pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    synth.write_peak_problem(pf, nf, a.n_train, a.n_train, a.length)
    qs = synth.make_peak_sequences(31, a.n_query // 2, a.length, True) + \
        synth.make_peak_sequences(32, a.n_query - a.n_query // 2, a.length, False)
    queries = dv.FlatSequences(dv.encode(b"".join(qs)), np.arange(len(qs) + 1, dtype=np.int64) * a.length)
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    print("model: %d SVs of %d, %d l-mers" % (model.n_sv, 2 * a.n_train, sum(len(s) - 9 for s in model.seqs)), flush=True)

    # warm-up: kernels' first launches, both scoring paths
    tab, _ = build(gp, model)
    warm = dv.FlatSequences(queries.codes[:a.length * 64], queries.off[:65])
    gp.score_with_table(tab, warm)
    gp.score(model, warm)
    torch.cuda.synchronize()

    tab, b10 = build(gp, model)
    print("build L=10: %(classes)d classes, host aggregation %(host_aggregation_s).3f s, k_lmer_weights %(kernel_ms).1f ms "
          "over %(pieces)d pieces (%(comparisons).3g comparisons = %(comparisons_per_s).3g /s), wall %(wall_s).2f s" % b10,
          flush=True)

    blocks = []
    t0 = time.perf_counter()
    _, s_tab = gp.score_with_table(tab, queries, on_block=blocks.append)
    tab_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, s_ref = gp.score(model, queries)
    ref_s = time.perf_counter() - t0
    scale = np.abs(model.dual_coef()).sum()
    worst = float(np.max(np.abs(s_tab - s_ref)) / scale)
    score_kernel_ms = sum(b["score_kernel_ms"] for b in blocks)
    print("score_with_table: %d queries in %.3f s = %.0f queries/s (%d blocks, k_lmer_score %.2f ms); score: %.2f s = %.0f "
          "queries/s; %.1fx; worst |difference| / sum|dual_coef| = %.3g"
          % (a.n_query, tab_s, a.n_query / tab_s, len(blocks), score_kernel_ms, ref_s, a.n_query / ref_s, ref_s / tab_s,
             worst), flush=True)
    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, n_query=a.n_query, length=a.length, build_l10=b10,
               table_score_s=tab_s, table_queries_per_s=a.n_query / tab_s, table_blocks=len(blocks),
               table_score_kernel_ms=score_kernel_ms, score_s=ref_s, score_queries_per_s=a.n_query / ref_s,
               speedup=ref_s / tab_s, worst_diff_over_sum_abs_dual=worst)

    if not a.no_l12:
        m12 = gp.Model(4, 12, 6, 3, model.M, model.H, model.gamma, model.C, model.tol, model.shrinking, model.rho,
                       model.n0, model.alpha, model.names, model.seqs)
        _, b12 = build(gp, m12)
        print("build L=12: %(classes)d classes, host aggregation %(host_aggregation_s).3f s, k_lmer_weights %(kernel_ms).1f "
              "ms over %(pieces)d pieces (%(comparisons).3g comparisons = %(comparisons_per_s).3g /s), wall %(wall_s).2f s"
              % b12, flush=True)
        out["build_l12"] = b12
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
