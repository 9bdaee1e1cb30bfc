"""Time the score of every single-base mutant (gkmpredict.mutant_scores) for an RBF model at gkmQC's shape: train a
weighted RBF model (type 5, gamma 1.0) and a weighted linear one (type 4) on the same 5 000 + 5 000 peak-like 600-bp
sequences (L=10 k=6 d=3), run mutant_scores on held-out queries, run the same queries through k_ism (`ism`) on the
type-4 model and on a type-4 model carrying the RBF model's own support vectors (the same enumeration work: what is left
is the fold), and score every single-base mutant of the first --n-brute queries through `score` (brute force, the only
route an RBF model had) in the same run.

    python tools/mutscores_throughput.py [--n-train 5000 --n-query 200 --n-brute 20 --block 0 --json out.json]

Prints ms per query of each route, k_ism_rbf's and k_ism's milliseconds (HIP events, summed over the blocks of an
instrumented call) and l-mer comparisons/s, the Gram and self-profile kernels' milliseconds, brute-force ms per query,
the speed-up, and the worst difference from brute force in units of sum |dual_coef|."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, *args, **kw):
    """(wall seconds, result, per-block measurements of a second, instrumented call with the same result)"""
    t0 = time.perf_counter()
    _, res = fn(*args, **kw)
    wall_s = time.perf_counter() - t0
    blocks = []
    _, again = fn(*args, on_block=blocks.append, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res, again))
    return wall_s, res, blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=5000, help="positives and as many negatives (default: 5000)")
    ap.add_argument("--n-query", type=int, default=200)
    ap.add_argument("--n-brute", type=int, default=20, help="queries scored mutant by mutant (default: 20)")
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--block", type=int, default=0, help="queries per block (0: gkmpredict.default_mutscores_block)")
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
    rbf = gp.train(pf, nf, kernel_type=5, L=10, k=6, d=3, gamma=a.gamma)
    print("train type 5 (gamma %g): %.2f s, %d SVs of %d" % (a.gamma, time.perf_counter() - t0, rbf.n_sv, 2 * a.n_train),
          flush=True)
    t0 = time.perf_counter()
    lin = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    print("train type 4: %.2f s, %d SVs of %d" % (time.perf_counter() - t0, lin.n_sv, 2 * a.n_train), flush=True)
    # the RBF model's support vectors under the linear kernel: k_ism's time does not depend on the coefficients
    twin = gp.Model(4, rbf.L, rbf.k, rbf.d, rbf.M, rbf.H, rbf.gamma, rbf.C, rbf.tol, rbf.shrinking, rbf.rho, rbf.n0,
                    rbf.alpha, rbf.names, rbf.seqs)
    block = a.block or gp.default_mutscores_block(a.length, rbf.d, rbf.n_sv)
    warm = dv.FlatSequences(codes[:a.length * 2], off[:3])                 # warm-up: contexts, first launches
    gp.mutant_scores(rbf, warm)
    gp.ism(lin, warm)
    gp.score(rbf, brute_q[:2])
    torch.cuda.synchronize()

    wall_s, ms, blocks = _timed(gp.mutant_scores, rbf, queries, block=block)
    rbf_ms = sum(b["ism_kernel_ms"] for b in blocks)
    rbf_cmp = sum(b["comparisons"] for b in blocks)
    gram_ms = sum(b["gram_kernel_ms"] for b in blocks)
    self_ms = sum(b["self_kernels_ms"] for b in blocks)
    assert blocks[0]["kernel"] == "k_ism_rbf"
    lin_wall_s, _, lin_blocks = _timed(gp.ism, lin, queries, block=block)
    lin_ms = sum(b["ism_kernel_ms"] for b in lin_blocks)
    lin_cmp = sum(b["comparisons"] for b in lin_blocks)
    twin_wall_s, _, twin_blocks = _timed(gp.ism, twin, queries, block=block)
    twin_ms = sum(b["ism_kernel_ms"] for b in twin_blocks)
    assert sum(b["comparisons"] for b in twin_blocks) == rbf_cmp and twin_blocks[0]["kernel"] == "k_ism"

    t0 = time.perf_counter()
    _, msb = gp.mutant_scores(rbf, brute_q)
    wall_small_s = time.perf_counter() - t0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(msb, ms[:nb]))

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
    _, sx = gp.score(rbf, brute_q)
    _, sy = gp.score(rbf, mutants)
    brute = [np.repeat(np.full((len(x), 1), sx[qi]), 4, axis=1) for qi, x in enumerate(brute_q)]
    for (qi, t, b), s in zip(index, sy):
        brute[qi][t, b] = s
    brute_s = time.perf_counter() - t0
    worst = max(np.abs(x - y).max() for x, y in zip(msb, brute)) / np.abs(rbf.dual_coef()).sum()
    effect = max(np.abs(v - v[np.arange(len(x)), x][:, None]).max() for v, x in zip(msb, brute_q)) \
        / np.abs(rbf.dual_coef()).sum()

    nq = a.n_query
    out = dict(n_train=2 * a.n_train, gamma=a.gamma, n_sv_rbf=rbf.n_sv, n_sv_lin=lin.n_sv, n_query=nq, length=a.length,
               block=block, blocks=len(blocks), wall_s=wall_s, ms_per_query=wall_s * 1e3 / nq, rbf_kernel_ms=rbf_ms,
               rbf_kernel_ms_per_query=rbf_ms / nq, rbf_comparisons=rbf_cmp, rbf_comparisons_per_s=rbf_cmp / (rbf_ms / 1e3),
               kernel_share_of_wall=rbf_ms / 1e3 / wall_s, gram_kernel_ms=gram_ms, self_kernels_ms=self_ms,
               lin_wall_s=lin_wall_s, lin_kernel_ms=lin_ms, lin_kernel_ms_per_query=lin_ms / nq, lin_comparisons=lin_cmp,
               lin_comparisons_per_s=lin_cmp / (lin_ms / 1e3), twin_wall_s=twin_wall_s, twin_kernel_ms=twin_ms,
               twin_kernel_ms_per_query=twin_ms / nq, rbf_over_twin=rbf_ms / twin_ms,
               rbf_over_lin_per_comparison=(rbf_ms / rbf_cmp) / (lin_ms / lin_cmp), n_brute=nb, n_mutants=len(mutants),
               small_ms_per_query=wall_small_s * 1e3 / nb, brute_ms_per_query=brute_s * 1e3 / nb,
               speedup=(brute_s / nb) / (wall_s / nq), speedup_same_queries=brute_s / wall_small_s,
               worst_rel_to_brute=worst, largest_effect_rel=effect)
    print("mutant_scores (type 5, gamma %g): %d queries x %d SVs in %.2f s = %.2f ms per query (block %d); k_ism_rbf %.1f "
          "ms = %.2f ms per query, %.3g l-mer comparisons/s, %.1f %% of the wall time; Gram %.1f ms, self profiles %.1f ms"
          % (a.gamma, nq, rbf.n_sv, wall_s, wall_s * 1e3 / nq, block, rbf_ms, rbf_ms / nq, rbf_cmp / (rbf_ms / 1e3),
             100 * rbf_ms / 1e3 / wall_s, gram_ms, self_ms))
    print("k_ism, the same queries, type-4 model trained on the same sequences (%d SVs): %.1f ms = %.2f ms per query, %.3g "
          "comparisons/s; k_ism_rbf per comparison is %.3fx k_ism" % (lin.n_sv, lin_ms, lin_ms / nq,
                                                                     lin_cmp / (lin_ms / 1e3),
                                                                     out["rbf_over_lin_per_comparison"]))
    print("k_ism, the same queries, the RBF model's own %d SVs under the linear kernel: %.1f ms = %.2f ms per query; "
          "k_ism_rbf is %.3fx k_ism: the RBF fold costs %.1f ms of %.1f (%.1f %%)"
          % (rbf.n_sv, twin_ms, twin_ms / nq, rbf_ms / twin_ms, rbf_ms - twin_ms, rbf_ms,
             100 * (rbf_ms - twin_ms) / rbf_ms))
    print("brute force: %d queries, %d mutants through score in %.2f s = %.1f ms per query; mutant_scores of the same %d "
          "queries alone %.2f ms per query; speed-up %.1fx (%.1fx on the same queries); worst difference %.2g x sum "
          "|dual_coef| (largest mutation effect %.2g x)"
          % (nb, len(mutants), brute_s, brute_s * 1e3 / nb, nb, wall_small_s * 1e3 / nb, out["speedup"],
             out["speedup_same_queries"], worst, effect))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
