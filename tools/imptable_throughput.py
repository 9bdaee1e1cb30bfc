"""Time per-base importance tables (gkmqc_amd/gkmtables.py lmer_importance, explain_with_table,
hypothetical_with_table) at gkmQC's shape: 600-bp peak-like sequences, L=10 k=6 d=3, weighted kernel
(type 4).

    python tools/imptable_throughput.py [--n-train 5000 --n-small 1000 --n-large 100000 --json out.json]

Prints, from one process: the table build (k_lmer_importance milliseconds from HIP events summed over its pieces,
comparisons/s) beside k_lmer_weights on the same classes; explain_with_table and hypothetical_with_table on --n-small and
--n-large queries, wall time (the table's upload included) and kernel time; `explain` and `hypothetical` on the --n-small
queries; and the worst differences between the two routes as multiples of sum |dual_coef|."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(fn, model):
    pieces = []
    t0 = time.perf_counter()
    tab = fn(model, on_piece=pieces.append)
    wall_s = time.perf_counter() - t0
    kernel_ms = sum(p["kernel_ms"] for p in pieces)
    comparisons = sum(p["comparisons"] for p in pieces)
    return tab, dict(kernel=pieces[0]["kernel"], classes=pieces[0]["classes"], pieces=len(pieces), kernel_ms=kernel_ms,
                     comparisons=comparisons, comparisons_per_s=comparisons / (kernel_ms / 1e3), wall_s=wall_s)


def timed(fn, key, *args):
    """-> (values, dict): wall seconds of one call, queries/s, the summed kernel milliseconds of its blocks"""
    blocks = []
    t0 = time.perf_counter()
    _, values = fn(*args, on_block=blocks.append)
    wall_s = time.perf_counter() - t0
    n = sum(b["queries"] for b in blocks)
    info = dict(queries=n, wall_s=wall_s, queries_per_s=n / wall_s, ms_per_query=1e3 * wall_s / n, blocks=len(blocks),
                kernel_ms=sum(b[key] for b in blocks))
    if "self_kernels_ms" in blocks[0]:
        info["self_kernels_ms"] = sum(b["self_kernels_ms"] for b in blocks)
    return values, info


def worst(a, b, scale):
    return float(max(np.max(np.abs(x - y)) for x, y in zip(a, b)) / scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=5000, help="positives and as many negatives (default: 5000)")
    ap.add_argument("--n-small", type=int, default=1000, help="queries both routes serve (default: 1000)")
    ap.add_argument("--n-large", type=int, default=100000, help="queries the table route serves alone (default: 100000)")
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    tmp = tempfile.mkdtemp()
    pf, nf = os.path.join(tmp, "p.fa"), os.path.join(tmp, "n.fa")
    synth.write_peak_problem(pf, nf, a.n_train, a.n_train, a.length)
    qs = synth.make_peak_sequences(31, a.n_large // 2, a.length, True) + \
        synth.make_peak_sequences(32, a.n_large - a.n_large // 2, a.length, False)
    order = np.random.default_rng(5).permutation(len(qs))               # (positives and negatives mixed in every prefix)
    codes = dv.encode(b"".join(qs[i] for i in order))
    large = dv.FlatSequences(codes, np.arange(len(qs) + 1, dtype=np.int64) * a.length)
    small = dv.FlatSequences(codes[:a.length * a.n_small], large.off[:a.n_small + 1])
    warm = dv.FlatSequences(codes[:a.length * 16], large.off[:17])
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    scale = float(np.abs(model.dual_coef()).sum())
    print("model: %d SVs of %d, %d l-mers" % (model.n_sv, 2 * a.n_train, sum(len(s) - 9 for s in model.seqs)), flush=True)

    # warm-up: every kernel's first launch, all four routes
    itab, _ = build(gp.lmer_importance, model)
    build(gp.lmer_weights, model)
    for fn, arg in ((gp.explain_with_table, itab), (gp.hypothetical_with_table, itab), (gp.explain, model),
                    (gp.hypothetical, model)):
        fn(arg, warm)
    torch.cuda.synchronize()

    itab, bi = build(gp.lmer_importance, model)
    _, bw = build(gp.lmer_weights, model)
    fmt = ("%(kernel)s: %(classes)d classes, %(kernel_ms).1f ms over %(pieces)d pieces (%(comparisons).3g comparisons = "
           "%(comparisons_per_s).3g /s), wall %(wall_s).2f s")
    print("build " + fmt % bi, flush=True)
    print("build " + fmt % bw, flush=True)
    print("k_lmer_importance / k_lmer_weights = %.2fx" % (bi["kernel_ms"] / bw["kernel_ms"]), flush=True)
    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, length=a.length, build_importance=bi, build_weights=bw,
               build_ratio=bi["kernel_ms"] / bw["kernel_ms"])

    line = "%s: %d queries in %.3f s = %.0f queries/s = %.4f ms per query (%d blocks, kernel %.2f ms%s)"

    def report(name, info):
        extra = ", self profiles %.2f ms" % info["self_kernels_ms"] if "self_kernels_ms" in info else ""
        print(line % (name, info["queries"], info["wall_s"], info["queries_per_s"], info["ms_per_query"], info["blocks"],
                      info["kernel_ms"], extra), flush=True)
        out[name] = info

    e_tab, info = timed(gp.explain_with_table, "explain_kernel_ms", itab, small)
    report("explain_with_table_small", info)
    e_ref, info = timed(gp.explain, "explain_kernel_ms", model, small)
    report("explain_small", info)
    h_tab, info = timed(gp.hypothetical_with_table, "hyp_kernel_ms", itab, small)
    report("hypothetical_with_table_small", info)
    h_ref, info = timed(gp.hypothetical, "hyp_kernel_ms", model, small)
    report("hypothetical_small", info)
    out["explain_speedup_small"] = out["explain_small"]["wall_s"] / out["explain_with_table_small"]["wall_s"]
    out["hypothetical_speedup_small"] = (out["hypothetical_small"]["wall_s"] /
                                         out["hypothetical_with_table_small"]["wall_s"])
    out["worst_explain_diff_over_sum_abs_dual"] = worst(e_tab, e_ref, scale)
    out["worst_hypothetical_diff_over_sum_abs_dual"] = worst(h_tab, h_ref, scale)
    print("at %d queries, the table's upload included: explain_with_table %.1fx explain, hypothetical_with_table %.1fx "
          "hypothetical" % (a.n_small, out["explain_speedup_small"], out["hypothetical_speedup_small"]), flush=True)
    print("worst |difference| / sum|dual_coef|: explain %.3g, hypothetical %.3g"
          % (out["worst_explain_diff_over_sum_abs_dual"], out["worst_hypothetical_diff_over_sum_abs_dual"]), flush=True)
    del e_tab, e_ref, h_tab, h_ref

    _, info = timed(gp.explain_with_table, "explain_kernel_ms", itab, large)
    report("explain_with_table_large", info)
    _, info = timed(gp.hypothetical_with_table, "hyp_kernel_ms", itab, large)
    report("hypothetical_with_table_large", info)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
