"""The bracket every timed launch shares (gkm_launch_enter / begin / stop / done, gkm_context.hip): each entry point of
device.py once on one small context, then what last_kernel_name(), last_comparisons(), last_kernel_ms() and the kernel
timeline report -- the name and the comparison count of each, one event pair per timed call and none for scan_lmers, and
nothing changed by a call that is refused at its argument check."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, K, D = 6, 4, 2
CODES = 4 ** L
NV = 11                      # classes of the table folds: one scalar request of eight and a tail of three
Q_LMERS = (30 - L + 1) + (41 - L + 1) + (50 - L + 1)
BASES = 30 + 41 + 50
WIDTH, STRIDE, RECORD = 40, 7, 120
NWIN = (RECORD - WIDTH) // STRIDE + 1
WIN_LMERS = WIDTH - L + 1

# (entry point, last_kernel_name(), last_comparisons()); None: any name but "none".  The counts without a formula beside
# them are what the commit before the shared bracket returned for these inputs.
EXPECTED = [
    ("gram_block", None, 44520.0),
    ("explain_block", "k_explain", 44520.0),
    ("ism_block", "k_ism", 44520.0),
    ("hyp_block", "k_ism<true>", 44520.0),
    ("ism_self_profiles", "k_ism_self", 357860.0),
    ("self_profiles", "k_ism_self_base", 7892.0),
    ("lmer_weights", "k_lmer_weights", 2.0 * NV * CODES),
    ("lmer_score", "k_lmer_score", float(Q_LMERS)),
    ("lmer_importance", "k_lmer_importance", 2.0 * NV * CODES),
    ("lmer_explain", "k_lmer_explain", float(L * Q_LMERS)),
    ("lmer_hyp", "k_lmer_hyp", float(4 * L * Q_LMERS)),
    ("scan_profiles", "k_scan_profiles", 6650.0),
    ("scan_score", "k_scan_score", float(NWIN * WIN_LMERS)),
    ("delta_sat", "k_delta_sat", 2760.0),
    ("delta_variants", "k_delta_variants", 27.0),
]


def run_calls(dv):
    """Every timed entry point once, scan_lmers among them, inside a kernel timeline; then the two refused calls.
    -> dict(seen=[(entry point, name, comparisons, ms)], scan_lmers=(before, after), timeline_on, timeline_off,
    refused=[(raised, before, after)])"""
    import torch
    rng = np.random.default_rng(20261)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in (40,) * 6 + (30, 41, 50)]
    dev = torch.device("cuda", 0)
    ctx = dv.GramContext(4, L, K, D)
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    try:
        with torch.cuda.device(dev):
            ctx.set_sequences(seqs)
            rows = np.arange(6)
            W = torch.from_numpy(rng.standard_normal(CODES)).to(dev)
            V = torch.from_numpy(rng.standard_normal((CODES, L))).to(dev)
            coef = torch.from_numpy(rng.standard_normal(6)).to(dev)
            xscale = torch.from_numpy(rng.random(3) + 0.5).to(dev)
            c = rng.random(D + 1)
            v = torch.from_numpy(rng.integers(0, CODES, NV).astype(np.int32)).to(dev)
            cv = torch.from_numpy(rng.standard_normal(NV)).to(dev)
            G = torch.empty((6, 3), **f64)
            out1, out4, base = torch.empty(BASES, **f64), torch.empty((BASES, 4), **f64), torch.empty(3, **f64)
            prof, pself = torch.empty((BASES, 4, D + 1), **i64), torch.empty((3, D + 1), **i64)
            Wout, Vout, T = torch.empty(CODES, **f64), torch.empty((CODES, L), **f64), torch.empty(3, **f64)
            record = torch.from_numpy(rng.integers(0, 4, RECORD).astype(np.uint8)).to(dev)
            valid = torch.ones(RECORD, dtype=torch.uint8, device=dev)
            nlm = RECORD - L + 1
            lm = torch.empty(nlm, dtype=torch.int32, device=dev)
            wt = torch.from_numpy(rng.integers(1, 200, WIN_LMERS).astype(np.uint8)).to(dev)
            wprof, wout = torch.empty((NWIN, D + 1), **i64), torch.empty(NWIN, **f64)
            sat, dvar = torch.empty((RECORD, 4), **f64), torch.empty(2, **f64)
            var = np.array([[10, 1, 0, 1], [50, 2, 1, 3]], dtype=np.int32)
            alt = np.array([3, 0, 1, 2], dtype=np.uint8)
            p = torch.Tensor.data_ptr
            state = lambda: (ctx.last_kernel_name(), ctx.last_comparisons())  # noqa: E731
            calls = {
                "gram_block": lambda: ctx.gram_block(rows, 6, 9, p(G), 3),
                "explain_block": lambda: ctx.explain_block(rows, 6, 9, c, p(coef), p(xscale), p(out1)),
                "ism_block": lambda: ctx.ism_block(rows, 6, 9, c, c, c, p(coef), p(out4), p(base)),
                "hyp_block": lambda: ctx.hyp_block(rows, 6, 9, c, p(coef), p(out4)),
                "ism_self_profiles": lambda: ctx.ism_self_profiles(6, 9, p(prof)),
                "self_profiles": lambda: ctx.self_profiles(6, 9, p(pself)),
                "lmer_weights": lambda: ctx.lmer_weights(c, p(v), p(cv), NV, 0, CODES, p(Wout)),
                "lmer_score": lambda: ctx.lmer_score(6, 9, p(W), p(T)),
                "lmer_importance": lambda: ctx.lmer_importance(c, p(v), p(cv), NV, 0, CODES, p(Vout)),
                "lmer_explain": lambda: ctx.lmer_explain(6, 9, p(V), p(xscale), p(out1)),
                "lmer_hyp": lambda: ctx.lmer_hyp(6, 9, p(V), p(out4)),
                "scan_profiles": lambda: ctx.scan_profiles(p(lm), nlm, p(wt), WIDTH, STRIDE, NWIN, p(wprof)),
                "scan_score": lambda: ctx.scan_score(p(lm), nlm, p(wt), WIDTH, STRIDE, NWIN, p(W), p(wout)),
                "delta_sat": lambda: ctx.delta_sat(p(lm), nlm, 0, RECORD, p(W), p(sat)),
                "delta_variants": lambda: ctx.delta_variants(p(lm), p(record), RECORD, var, alt, p(W), p(dvar)),
            }
            res = dict(seen=[], refused=[])
            ctx.kernel_timeline(True)
            for name, _, _ in EXPECTED:
                if name == "scan_profiles":   # the l-mer words the scan and delta launches read
                    before = state()
                    ctx.scan_lmers(p(record), p(valid), RECORD, p(lm))
                    res["scan_lmers"] = (before, state())
                calls[name]()
                res["seen"].append((name,) + state() + (ctx.last_kernel_ms(),))
            res["timeline_on"] = ctx.kernel_timeline_ms()
            ctx.kernel_timeline(False)
            res["timeline_off"] = ctx.kernel_timeline_ms()
            for refused in (lambda: ctx.lmer_score(7, 7, p(W), p(T)),
                            lambda: ctx.lmer_weights(c, p(v), p(cv), NV, 5, 5, p(Wout))):
                before = state()
                try:
                    refused()
                    raised = False
                except dv.GkmError:
                    raised = True
                res["refused"].append((raised, before, state(), ctx.last_kernel_ms()))
            torch.cuda.synchronize()
            return res
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def res(built):
    from gkmqc_amd import device
    return run_calls(device)


def test_every_timed_call_reports_its_kernel_and_comparisons(res):
    assert [s[0] for s in res["seen"]] == [e[0] for e in EXPECTED]
    for (name, kernel, comparisons, ms), (_, want_kernel, want_comparisons) in zip(res["seen"], EXPECTED):
        print("%-18s %-18s %r comparisons, %.4f ms" % (name, kernel, comparisons, ms))
        if want_kernel is None:
            assert kernel and kernel != "none", name
        else:
            assert kernel == want_kernel, name
        assert comparisons == want_comparisons, name
        assert ms >= 0, name


def test_scan_lmers_takes_no_pair_and_leaves_the_last_launch(res):
    before, after = res["scan_lmers"]
    assert before == after == ("k_lmer_hyp", float(4 * L * Q_LMERS))


def test_timeline_counts_one_pair_per_timed_call(res):
    ms, launches = res["timeline_on"]
    assert ms >= 0 and launches == len(EXPECTED) == 15
    assert res["timeline_off"] == (0.0, 0)


def test_a_refused_call_leaves_no_trace(res):
    assert len(res["refused"]) == 2
    for raised, before, after, ms in res["refused"]:
        assert raised
        assert before == after == ("k_delta_variants", 27.0)
        assert ms >= 0
