"""The table and the panel functions of gkmpredict share one driver per operation (_score_folded, _scan_folded,
_delta_values, _saturation_folded) and the delta kernels one body (gkm_delta.hip).  What that sharing could break without
any value changing -- the keys of the measurement dicts, the kernel names they report, the default chunk or block -- and
the contract itself, column m of a panel result equals member m's single-table result bit for bit, on one small problem:
L = 5, k = 4, d = 1, kernel type 4; a record of 200 bases with an invalid base at 100; queries of 5, 68 and 69 bases (1,
64 and 65 l-mers); panels of 1 and 3 members."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 5
WIDTH, STRIDE, SCAN_CHUNK = 40, 7, 90                                      # 23 windows, 8 per chunk: three chunks

SCORE_KEYS = {"queries", "score_kernel_ms", "lmers", "kernel", "wall_ms"}
SCAN_KEYS = {"windows", "bases", "profile_kernel_ms", "comparisons", "kernel", "wall_ms"}
DELTA_KEYS = {"variants", "bases", "kernel_ms", "gathers", "kernel", "wall_ms"}
SATURATION_KEYS = {"positions", "bases", "kernel_ms", "gathers", "kernel", "wall_ms"}


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _same(got, want):
    """bit for bit, NaN where and only where the reference has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def _tables(gp, n=3):
    """random symmetric tables of mixed magnitude and sign (as tests/test_panel_gpu.py's), so that the order of additions
    shows"""
    rc = gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)
    out = []
    for m in range(n):
        rng = np.random.default_rng(4000 + m)
        W = rng.standard_normal(4 ** L) * 10.0 ** rng.integers(-6, 7, size=4 ** L)
        out.append(gp.LmerTable(W + W[rc], 4, L, L - 1, 1, 50, 50.0, 0.25 * m - 3.0))
    return out


def _record():
    x = np.random.default_rng(31).integers(0, 4, size=200, dtype=np.uint8)
    x[100] = 4
    return x


def _queries():
    rng = np.random.default_rng(32)
    return [rng.integers(0, 4, size=T, dtype=np.uint8) for T in (5, 68, 69)]


def _variants(x):
    """an SNV at either end, one whose context covers the invalid base, an insertion, a deletion, a no-op"""
    base = lambda p: "ACGT"[x[p]]                                          # noqa: E731
    other = lambda p: "ACGT"[(x[p] + 1) % 4]                               # noqa: E731
    return [(0, 0, base(0), other(0)), (0, 199, base(199), other(199)), (0, 98, base(98), other(98)),
            (0, 50, "", "ACG"), (0, 150, base(150) + base(151), ""), (0, 20, base(20), base(20))]


def _run(gp, folded, panel):
    """the four functions of a table or a panel on the problem -> {operation: (result, the callbacks' dicts, the result
    with the default chunk or block)}"""
    x, queries = _record(), _queries()
    variants = _variants(x)
    score, scan, delta, sat = ((gp.score_with_panel, gp.scan_with_panel, gp.delta_with_panel, gp.delta_saturation_with_panel)
                               if panel else (gp.score_with_table, gp.scan, gp.delta, gp.delta_saturation))
    chunk = gp.delta_min_chunk(L)
    out, seen = {}, {key: [] for key in ("score", "scan", "delta", "saturation")}
    out["score"] = (score(folded, queries, block=2, on_block=seen["score"].append)[1], seen["score"],
                    score(folded, queries)[1])
    out["scan"] = (scan(folded, [x], WIDTH, STRIDE, chunk=SCAN_CHUNK, on_chunk=seen["scan"].append)[0][2], seen["scan"],
                   scan(folded, [x], WIDTH, STRIDE)[0][2])
    out["delta"] = (delta(folded, [x], variants, chunk=chunk, on_chunk=seen["delta"].append), seen["delta"],
                    delta(folded, [x], variants))
    out["saturation"] = (sat(folded, [x], chunk=chunk, on_chunk=seen["saturation"].append)[0][1], seen["saturation"],
                         sat(folded, [x])[0][1])
    return out


@pytest.fixture(scope="module")
def single(gp):
    """the single-table results of the three members, made once"""
    return [_run(gp, t, False) for t in _tables(gp)]


def test_table_functions(single):
    for got in single:
        score, seen, again = got["score"]
        assert score.shape == (3,) and np.isfinite(score).all() and again.tobytes() == score.tobytes()
        assert [set(s) for s in seen] == [SCORE_KEYS] * 2 and [s["queries"] for s in seen] == [2, 1]
        assert {s["kernel"] for s in seen} == {"k_lmer_score"}
        scan, seen, again = got["scan"]
        assert scan.shape == (23,) and np.isnan(scan).any() and not np.isnan(scan).all() and _same(again, scan)
        assert [set(s) for s in seen] == [SCAN_KEYS] * 3 and [s["windows"] for s in seen] == [8, 8, 7]
        assert {s["kernel"] for s in seen} == {"k_scan_profiles"}
        delta, seen, again = got["delta"]
        assert delta.shape == (6,) and np.isnan(delta).tolist() == [False, False, True, False, False, False]
        assert delta[5] == 0.0 and not np.signbit(delta[5]) and _same(again, delta)
        assert [set(s) for s in seen] == [DELTA_KEYS] and seen[0]["kernel"] == "k_delta_variants" and seen[0]["variants"] == 6
        sat, seen, again = got["saturation"]
        assert sat.shape == (200, 4) and _same(again, sat)
        assert np.flatnonzero(np.isnan(sat).all(axis=1)).tolist() == list(range(96, 105)) and np.isnan(sat).sum() == 36
        assert [set(s) for s in seen] == [SATURATION_KEYS] and seen[0]["kernel"] == "k_delta_sat"
        assert seen[0]["positions"] == 200
        # the SNVs of the list are the map's entries
        x = _record()
        for i in (0, 1):
            p, alt = _variants(x)[i][1], _variants(x)[i][3]
            assert delta[i].tobytes() == sat[p, "ACGT".index(alt)].tobytes()


@pytest.mark.parametrize("n", [1, 3])
def test_panel_columns_keys_and_kernels(gp, single, n):
    got = _run(gp, gp.LmerPanel(_tables(gp)[:n]), True)
    models = {"models"}
    for op, keys, kernel, count in (("score", SCORE_KEYS | models, "k_panel_score", 2),
                                    ("scan", SCAN_KEYS | models | {"score_kernel", "score_kernel_ms"}, "k_scan_profiles", 3),
                                    ("delta", DELTA_KEYS | models, "k_panel_delta_variants", 1),
                                    ("saturation", SATURATION_KEYS | models, "k_panel_delta_sat", 1)):
        value, seen, again = got[op]
        want = np.stack([s[op][0] for s in single[:n]], axis=-1)
        assert value.shape == want.shape == single[0][op][0].shape + (n,), op
        for m in range(n):
            assert _same(value[..., m], want[..., m]), (op, n, m)
        assert _same(again, value), op
        assert [set(s) for s in seen] == [keys] * count, op
        assert {s["kernel"] for s in seen} == {kernel} and {s["models"] for s in seen} == {n}, op
    assert {s["score_kernel"] for s in got["scan"][1]} == {"k_panel_scan_score"}
    assert all(s["score_kernel_ms"] >= 0 and s["profile_kernel_ms"] >= 0 for s in got["scan"][1])
