"""Randomised sweep of the interpretation kernels (gkmhip_explain_block, gkmhip_ism_block, gkmhip_hyp_block,
gkmhip_ism_self_profiles) against the CPU references of the test-suite on the GPU box: random kernel type in {0, 1, 2, 4},
(L, k, d) with tiled and k = 0 shapes included, M, H, 1 to 5 support vectors and 1 to 6 queries drawn from the dense-hit
generator (tests/dense_inputs.py) mixed with iid ones, a random ascending row subset, a random column range, small
integer coefficients and one unit fold vector per launch (test infrastructure).  Every value is then an integer below
2^53 and must equal the reference's bit for bit: explain's H[m], ism's U[m], P_m and B[m], the hypothetical columns,
and the mutants' self profiles at sampled positions.
python tools/fuzz_interpret.py [--seconds 240] [--seed 1]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10, 6, 3), (10, 6, 3), (8, 4, 3), (6, 3, 3), (5, 2, 3), (3, 1, 2), (12, 8, 4), (11, 5, 5), (12, 4, 8), (8, 2, 6),
          (12, 1, 11), (5, 0, 5), (4, 0, 4), (7, 0, 6), (2, 1, 1)]


def draw_sequence(rng, D, L, d, longest):
    kind = int(rng.integers(0, 6))
    n = int(rng.choice([L, L + 1, 64 + L - 1, int(rng.integers(L, longest + 1)), int(rng.integers(L, longest + 1))]))
    if kind == 0:
        return rng.integers(0, 4, size=n, dtype=np.uint8)
    if kind == 1:
        return D.homopolymer(int(rng.integers(0, 4)), n)
    if kind == 2:
        return D.repeat([(D.A, D.T), (D.C, D.G), (D.A, D.C)][int(rng.integers(0, 3))], n)
    if kind == 3:
        return D.repeat(D.unit_of(int(rng.choice([3, 4, 5, 6, 7, max(3, L - 1), L, L + 1])), int(rng.integers(0, 9))), n)
    return D.spliced(max(n, L), L, int(rng.integers(0, 1 << 30)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch  # noqa: F401
    from gkmqc_amd import device
    from tests import dense_inputs as D
    from tests import explain_ref as E
    from tests import hyp_ref as HR
    from tests import ism_ref as R
    from tests.test_dense_gpu import ExplainLauncher
    from tests.test_hyp_gpu import _Launcher as HypLauncher
    from tests.test_ism_gpu import _Launcher as IsmLauncher
    from tests.test_ism_gpu import _split, _unit

    rng = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    cases, kinds = 0, {"explain": 0, "ism": 0, "hyp": 0, "self": 0, "tiled": 0, "k0": 0}
    while time.time() < t_end:
        t = int(rng.choice([0, 1, 2, 4]))
        L, k, d = SHAPES[int(rng.integers(len(SHAPES)))]
        if device.check_parameters(t, L, k, d):
            continue
        M, H = int(rng.choice([int(rng.integers(1, 256)), 254, 255])), float(rng.choice([int(rng.integers(1, 200)), 1e6]))
        tiled = D.ism_tile(L, d) < D.MAX_LEN
        longest = D.MAX_LEN if rng.random() < 0.15 else 300
        svs = [draw_sequence(rng, D, L, d, min(longest, 120 if longest > 300 else 300)) for _ in range(int(rng.integers(1, 6)))]
        queries = [draw_sequence(rng, D, L, d, longest) for _ in range(int(rng.integers(1, 7)))]
        if rng.random() < 0.5:                                       # a near copy of a support vector among the queries
            s = svs[int(rng.integers(len(svs)))]
            queries[0] = D.substituted(s, int(rng.integers(0, min(L, d + 2) + 1)), L, int(rng.integers(0, 1 << 30)))
        seqs = svs + queries
        S, Q = len(svs), len(queries)
        rows = np.sort(rng.choice(S, size=int(rng.integers(1, S + 1)), replace=False))
        c0 = S + int(rng.integers(0, Q))
        c1 = int(rng.integers(c0 + 1, S + Q + 1))
        cols = seqs[c0:c1]
        coef = rng.integers(-5, 6, size=len(rows)).astype(np.float64)
        coef[coef == 0] = 1.0
        m = int(rng.integers(0, d + 1))
        mb = min(d + 1, L)
        bm = int(rng.integers(1, mb + 1))
        params = (t, L, k, d, M, H)
        what = "t=%d L=%d k=%d d=%d M=%d H=%g svs=%s queries=%s rows=%s [%d, %d) m=%d bm=%d seed=%d case=%d" % (
            t, L, k, d, M, H, [len(s) for s in svs], [len(x) for x in queries], rows.tolist(), c0, c1, m, bm, a.seed, cases)
        U, B, P = [], [], []
        for x in cols:
            tl = [R.tallies(x, seqs[i], t, L, d, M, H) for i in rows]
            U.append(sum(c * u for c, (u, _) in zip(coef, tl)))
            B.append(sum(c * b for c, (_, b) in zip(coef, tl)))
            P.append(sum(c * R.profile(x, seqs[i], t, L, d, M, H) for c, i in zip(coef, rows)))
        run = IsmLauncher(device, params, seqs)
        try:
            out, base = run.block(rows, c0, c1, _unit(d + 1, m), _unit(d + 1, None), _unit(d + 1, m), coef)
            for qi, (g, x) in enumerate(zip(_split(out, cols, (4,)), cols)):
                w = np.repeat(U[qi][:, m:m + 1].astype(np.float64), 4, axis=1)
                w[np.arange(len(x)), x] = 0.0
                if not np.array_equal(g, w) or base[qi] != float(P[qi][m]):
                    raise SystemExit("ISM U / P MISMATCH query %d %s" % (qi, what))
            out, _ = run.block(rows, c0, c1, _unit(d + 1, None), _unit(d + 1, bm - 1), _unit(d + 1, None), coef)
            for qi, g in enumerate(_split(out, cols, (4,))):
                if not np.array_equal(g, B[qi][:, bm].astype(np.float64)):
                    raise SystemExit("ISM B MISMATCH query %d %s" % (qi, what))
            kinds["ism"] += 1
            short = [qi for qi, x in enumerate(cols) if len(x) <= 300]
            if short:
                prof = run.self_profiles(c0, c1)
                for qi in short[:2]:
                    x = cols[qi]
                    pos = sorted(set(int(p) for p in rng.integers(0, len(x), size=3)) | {0, len(x) - 1})
                    want = R.self_profiles(x, t, L, d, M, H, positions=pos)
                    got = _split(prof, cols, (4, d + 1))[qi]
                    if not np.array_equal(got[pos], want[pos]):
                        raise SystemExit("SELF PROFILE MISMATCH query %d %s" % (qi, what))
                kinds["self"] += 1
        finally:
            run.close()
        if k > 0 and d < L:
            run = ExplainLauncher(device, params, seqs)
            try:
                got = run.block(rows, c0, c1, _unit(d + 1, m), coef)
                for qi, g in enumerate(_split(got, cols, ())):
                    if not np.array_equal(g, U[qi][:, m].astype(np.float64)):
                        raise SystemExit("EXPLAIN MISMATCH query %d %s" % (qi, what))
                    if qi == 0 and len(rows) == 1:                   # (explain_ref on its own, not through ism_ref)
                        h = E.tallies(cols[0], seqs[rows[0]], t, L, d, M, H)
                        if not np.array_equal(g, coef[0] * h[:, m]):
                            raise SystemExit("EXPLAIN MISMATCH (explain_ref) %s" % what)
                kinds["explain"] += 1
            finally:
                run.close()
            run = HypLauncher(device, params, seqs)
            try:
                out = run.block(rows, c0, c1, _unit(d + 1, m), coef)
                for qi, (g, x) in enumerate(zip(_split(out, cols, (4,)), cols)):
                    if not np.array_equal(g, HR.raw_from_tallies(x, U[qi], B[qi], _unit(d + 1, m), d)):
                        raise SystemExit("HYPOTHETICAL MISMATCH query %d %s" % (qi, what))
                kinds["hyp"] += 1
            finally:
                run.close()
        kinds["tiled"] += int(tiled and max(len(x) for x in cols) > D.ism_tile(L, d))
        kinds["k0"] += int(k == 0)
        cases += 1
        if cases % 50 == 0:
            print("%d cases ok %s" % (cases, kinds), flush=True)
    print("interpret fuzz ok: %d cases, %s" % (cases, kinds))


if __name__ == "__main__":
    main()
