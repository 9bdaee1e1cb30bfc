"""Time hypothetical importance (gkmpredict.hypothetical) at gkmQC's shape: train on 5 000 + 5 000 peak-like 600-bp
sequences (L=10 k=6 d=3, weighted kernel type 4), run it on held-out queries, run the two-pass composition that needs no
new kernel on the same queries (ism_block with fold_u = 0 and fold_b = share for the mutant columns, explain_block for the
own column), and run `explain` on every single-base mutant of the first --n-brute queries (brute force), all in one run.

    python tools/hyp_throughput.py [--n-train 5000 --n-query 200 --n-brute 5 --block 0 --json out.json]

Prints ms per query of each of the three, the fused kernel's milliseconds (HIP events, summed over the blocks of a second,
instrumented call) and its share of the wall time, the two passes' kernel milliseconds, the self-profile kernels'
milliseconds, and the worst difference of the two-pass composition and of brute force from the fused result."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def two_pass(gp, dv, model, seqs, block, kernel_ms):
    """gkmpredict.hypothetical with the raw values from gkmhip_ism_block (mutant columns) and gkmhip_explain_block (own
    column) instead of gkmhip_hyp_block; kernel_ms collects [ism_block ms, explain_block ms] per block"""
    import torch
    S, Q, d = model.n_sv, len(seqs), model.d
    ctx = dv.cached_context(*model.kernel_params())
    share = gp.explain_shares(model)
    c = dv.mismatch_weights(model.kernel_type, model.L, model.k)[:d + 1]
    zero = np.zeros(d + 1)
    sv_codes = np.concatenate(model.seqs)
    sv_off = np.zeros(S + 1, dtype=np.int64)
    np.cumsum([len(s) for s in model.seqs], out=sv_off[1:])
    rows = np.arange(S, dtype=np.int32)
    out = []
    stream = torch.cuda.current_stream().cuda_stream
    sq = torch.empty(S + block, dtype=torch.float64, device="cuda")
    dual = torch.from_numpy(model.dual_coef()).cuda()
    most = max(int(seqs.off[min(Q, q0 + block)] - seqs.off[q0]) for q0 in range(0, Q, block))
    R = torch.empty((most, 4), dtype=torch.float64, device="cuda")
    own = torch.empty(most, dtype=torch.float64, device="cuda")
    prof = torch.empty((most, 4, d + 1), dtype=torch.int64, device="cuda")
    for q0 in range(0, Q, block):
        q1 = min(Q, q0 + block)
        qb = q1 - q0
        qoff = seqs.off[q0:q1 + 1]
        nb = int(qoff[-1] - qoff[0])
        union = dv.FlatSequences(np.concatenate((sv_codes, seqs.codes[qoff[0]:qoff[-1]])),
                                 np.concatenate((sv_off, sv_off[-1] + (qoff[1:] - qoff[0]))))
        ctx.set_sequences(union, stream)
        ctx.self_norms(sq.data_ptr(), stream)
        ctx.ism_self_profiles(S, S + qb, prof.data_ptr(), stream)
        coef = dual / sq[:S]
        xscale = 1.0 / sq[S:S + qb]
        ctx.ism_block(rows, S, S + qb, zero, share, zero, coef.data_ptr(), R.data_ptr(), None, stream)
        ms = [ctx.last_kernel_ms()]
        ctx.explain_block(rows, S, S + qb, share, coef.data_ptr(), xscale.data_ptr(), own.data_ptr(), stream)
        ms.append(ctx.last_kernel_ms())
        kernel_ms.append(ms)
        g = torch.zeros((nb, 4), dtype=torch.float64, device="cuda")
        for m in range(d + 1):
            g.add_(prof[:nb, :, m].double().mul_(float(c[m])))
        res = R[:nb] * (1.0 / g.sqrt_())
        x = torch.from_numpy(seqs.codes[qoff[0]:qoff[-1]].astype(np.int64)).cuda()
        res.scatter_(1, x[:, None], own[:nb, None])
        host = res.cpu().numpy()
        out.extend(np.split(host, (qoff[1:-1] - qoff[0]).astype(np.int64)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=5000, help="positives and as many negatives (default: 5000)")
    ap.add_argument("--n-query", type=int, default=200)
    ap.add_argument("--n-brute", type=int, default=5, help="queries explained mutant by mutant (default: 5)")
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--block", type=int, default=0, help="queries per block (0: gkmpredict.default_hyp_block)")
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
    block = a.block or gp.default_hyp_block(a.length, model.d)
    warm = dv.FlatSequences(codes[:a.length * 2], off[:3])
    gp.hypothetical(model, warm)                                           # warm-up: context, first launches
    two_pass(gp, dv, model, warm, 2, [])
    gp.explain(model, brute_q[:2])
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    _, Hf = gp.hypothetical(model, queries, block=block)
    wall_s = time.perf_counter() - t0
    blocks = []                                                            # the same again, instrumented per block
    _, H2 = gp.hypothetical(model, queries, block=block, on_block=blocks.append)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(Hf, H2))
    hyp_ms = sum(b["hyp_kernel_ms"] for b in blocks)
    self_ms = sum(b["self_kernels_ms"] for b in blocks)
    comparisons = sum(b["comparisons"] for b in blocks)

    t0 = time.perf_counter()                                               # A/B: the two-pass composition
    pass_ms = []
    Ht = two_pass(gp, dv, model, queries, block, pass_ms)
    torch.cuda.synchronize()
    two_s = time.perf_counter() - t0
    two_ism_ms = sum(m[0] for m in pass_ms)
    two_explain_ms = sum(m[1] for m in pass_ms)
    two_worst = max(np.abs(x - y).max() for x, y in zip(Ht, Hf)) / np.abs(model.dual_coef()).sum()
    two_identical = all(np.array_equal(x, y) for x, y in zip(Ht, Hf))

    t0 = time.perf_counter()                                               # brute force: explain every mutant
    mutants, index = [], []
    for qi, x in enumerate(brute_q):
        for t in range(len(x)):
            for b in range(4):
                if b != x[t]:
                    y = x.copy()
                    y[t] = b
                    mutants.append(y)
                    index.append((qi, t, b))
    _, ex = gp.explain(model, brute_q)
    _, ey = gp.explain(model, mutants)
    brute = [np.zeros((len(x), 4)) for x in brute_q]
    for qi, x in enumerate(brute_q):
        brute[qi][np.arange(len(x)), x] = ex[qi]
    for (qi, t, b), e in zip(index, ey):
        brute[qi][t, b] = e[t]
    brute_s = time.perf_counter() - t0
    brute_worst = max(np.abs(x - y).max() for x, y in zip(brute, Hf[:nb])) / np.abs(model.dual_coef()).sum()
    brute_identical = all(x.tobytes() == y.tobytes() for x, y in zip(brute, Hf[:nb]))

    out = dict(n_train=2 * a.n_train, n_sv=model.n_sv, n_query=a.n_query, length=a.length, block=block,
               blocks=len(blocks), wall_s=wall_s, hyp_ms_per_query=wall_s * 1e3 / a.n_query, hyp_kernel_ms=hyp_ms,
               kernel=blocks[0]["kernel"], comparisons=comparisons, comparisons_per_s=comparisons / (hyp_ms / 1e3),
               kernel_share_of_wall=hyp_ms / 1e3 / wall_s, self_kernels_ms=self_ms,
               two_pass_s=two_s, two_pass_ms_per_query=two_s * 1e3 / a.n_query, two_pass_ism_kernel_ms=two_ism_ms,
               two_pass_explain_kernel_ms=two_explain_ms, two_pass_over_fused=two_s / wall_s,
               two_pass_worst_rel=two_worst, two_pass_bit_identical=two_identical, n_brute=nb,
               n_mutants=len(mutants), brute_ms_per_query=brute_s * 1e3 / nb,
               brute_over_fused=(brute_s / nb) / (wall_s / a.n_query), brute_worst_rel=brute_worst,
               brute_bit_identical=brute_identical)
    print("hypothetical: %d queries x %d SVs in %.2f s = %.2f ms per query (block %d); k_ism<true> %.1f ms = %.3g l-mer "
          "comparisons/s, %.1f %% of the wall time; self profiles %.1f ms"
          % (a.n_query, model.n_sv, wall_s, wall_s * 1e3 / a.n_query, block, hyp_ms, comparisons / (hyp_ms / 1e3),
             100 * hyp_ms / 1e3 / wall_s, self_ms))
    print("two passes: %.2f ms per query (k_ism %.1f ms + k_explain %.1f ms), %.2fx the fused time; bit-identical %s, "
          "worst difference %.2g x sum |dual_coef|" % (two_s * 1e3 / a.n_query, two_ism_ms, two_explain_ms,
                                                       two_s / wall_s, two_identical, two_worst))
    print("brute force: %d queries, %d mutants through explain in %.2f s = %.1f ms per query, %.1fx the fused time; "
          "bit-identical %s, worst difference %.2g x sum |dual_coef|"
          % (nb, len(mutants), brute_s, brute_s * 1e3 / nb, out["brute_over_fused"], brute_identical, brute_worst))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
