"""What gkmqc_amd.gkmpredict offers, pinned without a GPU: the public names callers import from it, each the same
object as in the module that owns it (gkmmodel, gkmquery, gkmtables, gkmscan, gkmdelta); the shape of its command line
(positionals, options, defaults) as literals; the usage block of its docstring against the command table; and, for
three commands, the two promises main() itself keeps: a missing input is refused by name with exit status 1, and an
output file appears only complete."""
import argparse
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers

OWNERS = {"gkmqc_amd." + m for m in ("gkmmodel", "gkmquery", "gkmtables", "gkmscan", "gkmdelta", "gkmpredict")}

PUBLIC_NAMES = """
    BLOCK_BYTES C_SVC DELTA_MAX_ALLELE DIST_DIGIT_BITS DIST_MAX_RANKS DIST_MAX_THRESHOLDS EPSILON_SVR EXPLAIN_CHUNKS
    FORMAT IMPORTANCE_FORMAT ISM_CHUNKS LmerImportanceTable LmerPanel LmerTable MAX_SVR_SAMPLES Model ModelError
    PANEL_FORMAT PANEL_MAX_BYTES PANEL_MAX_MODELS REGION_FIELDS REGION_MAX_GAP SCAN_MAX_WIDTH SVR_FORMAT
    TABLE_FORMAT TABLE_PIECE build_parser canonical_codes check_delta check_explainable check_ism check_panel
    check_panel_delta check_panel_scan check_panel_scan_quantiles check_panel_scan_regions
    check_panel_scan_tail_counts check_queries check_scan check_scan_quantiles check_scan_regions
    check_scan_tail_counts check_table_model check_train_args codes_to_text default_block default_delta_chunk
    default_explain_block default_hyp_block default_imptable_block default_ism_block default_mutscores_block
    default_panel_scan_chunk default_scan_chunk default_table_block delta delta_chunk_plan delta_context
    delta_min_chunk delta_saturation delta_saturation_chunk_plan delta_saturation_with_panel delta_trim
    delta_with_panel dist_boundaries dist_level_bits dist_list explain explain_shares explain_with_table
    hypothetical hypothetical_with_table ism ism_coefficients keys_to_scores lmer_classes lmer_importance lmer_rc
    lmer_text lmer_weights load load_importance_table load_lmer_panel load_lmer_table main mutant_scores pack_lmers
    panel_member_names panel_row_stride quantile_ranks read_delta read_explanation read_ism read_long_fasta
    read_panel_output read_panel_quantiles read_panel_regions read_panel_tail_counts read_quantiles read_regions
    read_saturation read_scan read_tail_counts read_targets read_variants region_thresholds scan scan_chunk_plan
    scan_quantiles scan_quantiles_with_panel scan_regions scan_regions_with_panel scan_tail_counts
    scan_tail_counts_with_panel scan_window_count scan_with_panel score score_keys score_with_panel score_with_table
    select_order_statistics stitch_regions text_to_codes train train_svr window_validity write_delta
    write_explanation write_ism write_panel_delta write_panel_quantiles write_panel_regions write_panel_scan
    write_panel_scores write_panel_tail_counts write_quantiles write_regions write_saturation write_scan
    write_scores write_tail_counts
""".split()

# (option strings, default, required), in the order the parser declares them
DEVICE, BLOCK, CHUNK = (("--device",), 0, False), (("--block",), None, False), (("--chunk",), None, False)
WIDTH, STRIDE = (("--width",), None, True), (("--stride",), 1, False)
QUERY = [DEVICE, BLOCK]
REGIONS = [WIDTH, STRIDE, (("--threshold",), "0", False), (("--gap",), 0, False), CHUNK, DEVICE]
TAIL = [WIDTH, STRIDE, CHUNK, (("--thresholds",), "", False), DEVICE]
QUANTILES = [WIDTH, STRIDE, CHUNK, (("--q",), None, False), (("--ranks",), None, False),
             (("--collect-cap",), 1048576, False), DEVICE]
TRAIN = [(("-t", "--kernel-type"), 4, False), (("-L", "--full-word-length"), 10, False),
         (("-k", "--non-gap-length"), 6, False), (("-d", "--max-num-gaps"), 3, False), (("-M", "--init-decay"), 50, False),
         (("-H", "--half-life-decay"), 50, False), (("-G", "--rbf-gamma"), 1.0, False),
         (("-C", "--regularization"), 1.0, False), (("-e", "--precision"), 0.001, False), (("-u", "--shrinking"), 0, False),
         DEVICE]
# command -> (positional destinations, options), the commands in the parser's order
CLI_SHAPE = {
    "train": (["pos_fa", "neg_fa", "model"], TRAIN),
    "train-svr": (["seqs_fa", "targets", "model"], TRAIN[:8] + [(("-p", "--epsilon"), 0.1, False)] + TRAIN[8:]),
    "predict": (["query_fa", "model", "output"], QUERY),
    "explain": (["query_fa", "model", "output"], QUERY),
    "ism": (["query_fa", "model", "output"], QUERY),
    "mutant-scores": (["query_fa", "model", "output"], QUERY),
    "hypothetical": (["query_fa", "model", "output"], QUERY),
    "weights": (["model", "output"], [DEVICE]),
    "predict-table": (["query_fa", "weights", "output"], QUERY),
    "scan": (["seqs_fa", "weights", "output"], [WIDTH, STRIDE, CHUNK, DEVICE]),
    "scan-regions": (["weights", "seqs_fa", "output"], REGIONS),
    "importance-table": (["model", "output"], [DEVICE]),
    "explain-table": (["query_fa", "table", "output"], QUERY),
    "hypothetical-table": (["query_fa", "table", "output"], QUERY),
    "delta": (["weights", "seqs_fa", "variants", "output"], [CHUNK, DEVICE]),
    "delta-saturation": (["weights", "seqs_fa", "output"], [CHUNK, DEVICE]),
    "panel": (["output", "weights"], [(("--names",), None, False)]),
    "predict-panel": (["query_fa", "panel", "output"], QUERY),
    "scan-panel": (["seqs_fa", "panel", "output"], [WIDTH, STRIDE, CHUNK, DEVICE]),
    "scan-regions-panel": (["panel", "seqs_fa", "output"], REGIONS),
    "scan-tail": (["weights", "seqs_fa", "output"], TAIL),
    "scan-quantiles": (["weights", "seqs_fa", "output"], QUANTILES),
    "scan-tail-panel": (["panel", "seqs_fa", "output"], TAIL),
    "scan-quantiles-panel": (["panel", "seqs_fa", "output"], QUANTILES),
    "delta-panel": (["seqs_fa", "variants", "panel", "output"], [CHUNK, DEVICE]),
}


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def test_every_public_name_is_still_there_and_lives_in_the_family(gp):
    import importlib
    assert len(PUBLIC_NAMES) == 141
    family = [importlib.import_module(m) for m in sorted(OWNERS)]
    for name in PUBLIC_NAMES:
        obj = getattr(gp, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__ in OWNERS, name
        holders = [m for m in family if name in vars(m)]                  # (a constant has no __module__ of its own)
        assert len(holders) >= 1 and all(vars(m)[name] is obj for m in holders), name


def test_a_fresh_interpreter_imports_the_module(built):
    """(an import cycle among the six modules would fail here)"""
    r = subprocess.run([sys.executable, "-c", "import gkmqc_amd.gkmpredict"], cwd=helpers.ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr


def test_command_line_shape(gp):
    parser = gp.build_parser()
    sub = [a for a in parser._actions if isinstance(a, argparse._SubParsersAction)][0]
    assert list(sub.choices) == list(CLI_SHAPE)
    for cmd, p in sub.choices.items():
        actions = [a for a in p._actions if not isinstance(a, argparse._HelpAction)]
        positionals = [a.dest for a in actions if not a.option_strings]
        options = [(tuple(a.option_strings), a.default, a.required) for a in actions if a.option_strings]
        assert (positionals, options) == CLI_SHAPE[cmd], cmd
    assert sub.choices["panel"]._actions[-1].nargs == "+"


def test_usage_block_lists_every_command(gp):
    assert list(gp.COMMANDS) == list(CLI_SHAPE)
    assert re.findall(r"^    python -m gkmqc_amd\.gkmpredict (\S+)", gp.__doc__, re.M) == list(gp.COMMANDS)


def _table(gp, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal(4 ** 5)
    W = W + W[gp.lmer_rc(np.arange(4 ** 5, dtype=np.uint32), 5)]
    return gp.LmerTable(W, 4, 5, 3, 2, 50, 50.0, 0.125)


@pytest.fixture
def cases(gp, tmp_path, monkeypatch):
    """command -> (argv up to the output, the index of an input that must be a file, the writer's name or None); the
    compute of each is replaced by a host stand-in, so that main() reaches its write stage without a device"""
    fa, var, weights, panel, model = (str(tmp_path / n) for n in ("s.fa", "v.tsv", "w.txt", "p.npz", "m.txt"))
    with open(fa, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n")
    with open(var, "w") as f:
        f.write("a\t3\tG\tT\n")
    _table(gp, 1).save(weights)
    gp.LmerPanel([_table(gp, 1), _table(gp, 2)]).save(panel)
    gp.Model(4, 5, 3, 2, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.0, 1, [1.0, 1.0], ["a", "b"],
             [np.zeros(9, np.uint8), np.ones(9, np.uint8)]).save(model)
    monkeypatch.setattr(gp, "scan", lambda *a: [("a", np.arange(2), np.array([0.5, np.nan]))])
    monkeypatch.setattr(gp, "delta_with_panel", lambda *a: np.array([[0.25, -1.0]]))
    monkeypatch.setitem(gp._QUERY_COMMANDS, "predict", (lambda *a: (["a"], [0.75]), gp.write_scores))
    return {"scan": (["scan", "--width", "20", fa, weights], 3, "write_scan"),
            "delta-panel": (["delta-panel", fa, var, panel], 2, "write_panel_delta"),
            "predict": (["predict", fa, model], 1, None)}


@pytest.mark.parametrize("cmd", ["scan", "delta-panel", "predict"])
def test_a_missing_input_is_refused_by_name(gp, cases, cmd, tmp_path, capsys):
    argv, at, _ = cases[cmd]
    out, missing = str(tmp_path / "out"), str(tmp_path / "missing")
    assert gp.main(argv[:at] + [missing] + argv[at + 1:] + [out]) == 1
    assert capsys.readouterr().err == "gkmpredict: error: cannot read %s\n" % missing
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


@pytest.mark.parametrize("cmd", ["scan", "delta-panel", "predict"])
def test_an_output_file_appears_only_complete(gp, cases, cmd, tmp_path, capsys, monkeypatch):
    argv, _, writer = cases[cmd]
    out = str(tmp_path / "out")
    assert gp.main(argv + [out]) == 0                                     # (the stand-in's values, the real writer)
    assert os.path.getsize(out) > 0 and not os.path.exists(out + ".tmp")
    os.remove(out)
    capsys.readouterr()

    def fails_halfway(path, *args):
        with open(path, "w") as f:
            f.write("half a line")
        raise OSError("no space left on device")
    if writer is None:
        monkeypatch.setitem(gp._QUERY_COMMANDS, cmd, (gp._QUERY_COMMANDS[cmd][0], fails_halfway))
    else:
        monkeypatch.setattr(gp, writer, fails_halfway)
    assert gp.main(argv + [out]) == 1
    assert capsys.readouterr().err == "gkmpredict: error: no space left on device\n"
    assert not os.path.exists(out)
