"""Time training on all sequences and scoring new ones (gkmqc_amd/gkmmodel.py, gkmquery.py) at gkmQC's shape: 600-bp peak-like
sequences, L=10 k=6 d=3, weighted kernel (type 4).

    python tools/predict_throughput.py [--n-train 5000 --n-query 100000 --block 0 --json out.json]

Prints train time, per-block and total score time with queries/s, the split of a block between the Gram kernel (HIP
events) and the rest (upload + table kernels, self norms, normalise, decision), and the pairs/s of the block launch next to
the triangle launch's on the training sequences, same process, same device."""
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
    ap.add_argument("--n-query", type=int, default=100000)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--block", type=int, default=0, help="queries per block (0: gkmpredict.default_block)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    tmp = tempfile.mkdtemp()
    pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    synth.write_peak_problem(pf, nf, a.n_train, a.n_train, a.length)
    t0 = time.perf_counter()
    qs = synth.make_peak_sequences(31, a.n_query // 2, a.length, True) + \
        synth.make_peak_sequences(32, a.n_query - a.n_query // 2, a.length, False)
    codes = dv.encode(b"".join(qs))
    off = np.arange(len(qs) + 1, dtype=np.int64) * a.length
    queries = dv.FlatSequences(codes, off)
    print("queries made in %.1f s" % (time.perf_counter() - t0), flush=True)

    # warm-up: context, kernels' first launch, solver
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    gp.score(model, dv.FlatSequences(codes[:a.length * 64], off[:65]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    train_s = time.perf_counter() - t0
    print("train: %.2f s, %d SVs of %d" % (train_s, model.n_sv, 2 * a.n_train), flush=True)

    block = a.block or gp.default_block(model.n_sv)
    t0 = time.perf_counter()
    _, scores = gp.score(model, queries, block=block)
    score_s = time.perf_counter() - t0
    print("score: %d queries in %.2f s = %.0f queries/s (block %d)" % (a.n_query, score_s, a.n_query / score_s, block),
          flush=True)

    blocks = []
    _, scores2 = gp.score(model, queries, block=block, on_block=blocks.append)
    assert np.array_equal(scores, scores2)
    for b in blocks:
        print("  block: %(queries)d queries, wall %(wall_ms).1f ms: upload %(upload_ms).1f, norms + gram %(norms_gram_ms).1f "
              "(Gram kernel %(gram_kernel_ms).1f), normalise %(normalize_ms).1f, decision %(decision_ms).1f  [%(kernel)s]" % b)
    gram_ms = sum(b["gram_kernel_ms"] for b in blocks)
    wall_ms = sum(b["wall_ms"] for b in blocks)
    pairs = float(model.n_sv) * a.n_query
    block_pps = pairs / (gram_ms / 1e3)

    # the triangle launch on the training sequences, same run
    seqs, _, _, _ = dv.read_problem(pf, nf)
    dv.gram_matrix(seqs, 4, 10, 6, 3, keep_context=True)
    tri = dv.gram_matrix(seqs, 4, 10, 6, 3, keep_context=True)
    n = len(seqs)
    tri_pairs = n * (n + 1) / 2.0
    tri_pps = tri_pairs / (tri["ms"] / 1e3)
    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, n_query=a.n_query, length=a.length, block=block,
               n_blocks=len(blocks), train_s=train_s, score_s=score_s, queries_per_s=a.n_query / score_s,
               instrumented_wall_ms=wall_ms, gram_kernel_ms=gram_ms,
               upload_ms=sum(b["upload_ms"] for b in blocks),
               norms_gram_ms=sum(b["norms_gram_ms"] for b in blocks),
               normalize_ms=sum(b["normalize_ms"] for b in blocks),
               decision_ms=sum(b["decision_ms"] for b in blocks),
               block_pairs=pairs, block_pairs_per_s=block_pps, block_kernel=blocks[0]["kernel"],
               triangle_pairs=tri_pairs, triangle_ms=tri["ms"], triangle_pairs_per_s=tri_pps,
               triangle_kernel=tri["kernel"])
    print("Gram kernel %.1f ms of %.1f ms instrumented wall (%.1f %%); block launch %.3g pairs/s, triangle launch %.3g "
          "pairs/s (ratio %.3f)" % (gram_ms, wall_ms, 100 * gram_ms / wall_ms, block_pps, tri_pps, block_pps / tri_pps))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
