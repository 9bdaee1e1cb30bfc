"""Train a gkm-SVM on all sequences, keep it in a model file, and score new sequences with it on the GPU.

The other half of a gkm-SVM next to the cross-validation of `gkmsvm.py` (the counterparts of LS-GKM's `gkmtrain` and
`gkmpredict`; the model file is this project's own):

  * `train` builds the Gram matrix of pos + neg on the device (device.gram_matrix, the resident path), solves ONE C-SVC on
    every sample with the GPU solver (svmcv.train_folds; scikit-learn if the solver stops at its iteration cap) and
    keeps the support vectors in LIBSVM's internal order;
  * `score` uploads [support vectors; a block of queries] into one cached context, takes the self norms of that set,
    computes the S x Qb block of kernel values (gkmhip_gram_block: SVs as rows, queries as columns) and its
    normalisation (gkmhip_normalize_block), and sums the decision values with k_decision (gkmsvm_decision_batch) --
    scikit-learn's `decision_function` of the trained SVC, bit for bit, for every block size;
  * `explain` splits each query's score over its bases (gkmhip_explain_block): per block the same upload
    as `score` and the self norms from exact 64-bit profiles (gkmhip_self_profiles: the same doubles as `score`'s while
    no profile reaches 2^31, the no-wrap domain of INTEGRATION.md §5b, and the true norms beyond), then one launch that credits every matching l-mer pair to the query bases it matched on;
  * `ism` scores every single-base substitution of each query (gkmhip_ism_block and
    gkmhip_ism_self_profiles): per block the same upload and exact self norms, one launch that tallies how each l-mer pair's
    mismatch count moves under a substitution, and one that counts every mutant's profile against itself;
  * `mutant_scores` gives the score of every single-base mutant itself, for every model `score` serves, the RBF types
    included: a linear model through `ism`'s launches, an RBF model through gkmhip_ism_rbf_block, which
    takes the raw kernel values of `score`'s Gram launch and folds each support vector's tallies through exp();
  * `hypothetical` gives, for every position and each of the four bases, the importance that base would get there
    (gkmhip_hyp_block): ism's upload, self norms, mutant self profiles and tallies, folded the way
    `explain` folds its own;
  * `weights` folds a model (not RBF) into one weight per l-mer (gkmhip_lmer_weights) and writes that
    table; `predict-table` scores from it with only the queries uploaded: their self norms, then one gather per l-mer
    (gkmhip_lmer_score) -- `predict`'s values up to rounding, for a fraction of the work;
  * `train_svr` fits an epsilon-SVR to one real target per sequence: the same Gram matrix, LIBSVM's
    2l-variable problem solved by the GPU solver with a linear term per position (svmcv.train_svr_folds); its model
    scores through the signed decision (gkmsvm_decision_signed_batch) -- scikit-learn's `SVR.predict`, bit for bit --
    and serves `explain`, `ism`, `hypothetical` and `weights` like a C-SVC model;
  * `scan` takes a weight table along sequences of any length and scores every window of W bases at a stride (DESIGN.md
    §5i, gkmhip_scan_profiles and gkmhip_scan_score): `predict-table`'s value for each window cut out, bit for bit, with
    the self norms of overlapping windows counted together; windows over a non-ACGT character have no score;
  * `importance-table` folds a model (not RBF, not k = 0) into one value per (l-mer, offset) (DESIGN.md §5j,
    gkmhip_lmer_importance); `explain-table` and `hypothetical-table` serve `explain`'s and `hypothetical`'s values from
    it, up to rounding, with only the queries uploaded: their self norms, then L gathers per base (gkmhip_lmer_explain)
    or 4 L (gkmhip_lmer_hyp);
  * `delta` gives the effect of sequence variants -- SNVs, MNVs, insertions, deletions -- from a weight table (deltaSVM,
    DESIGN.md §5k, gkmhip_delta_variants): the change in the summed weights of the l-mers a variant touches, for a list
    of variants against records of any length; `delta-saturation` gives every possible SNV of every position
    (gkmhip_delta_sat), the table-based counterpart of `ism`.

    python -m gkmqc_amd.gkmpredict train [-t -L -k -d -M -H -G -C -e -u] pos.fa neg.fa model.txt
    python -m gkmqc_amd.gkmpredict train-svr [-t -L -k -d -M -H -G -C -p -e -u] seqs.fa targets.txt model.txt
    python -m gkmqc_amd.gkmpredict predict query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict explain [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict ism [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict mutant-scores [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict hypothetical [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict weights model.txt weights.txt
    python -m gkmqc_amd.gkmpredict predict-table [--block Qb] query.fa weights.txt out.txt
    python -m gkmqc_amd.gkmpredict scan --width W [--stride s] [--chunk B] seqs.fa weights.txt out.bedgraph
    python -m gkmqc_amd.gkmpredict scan-regions --width W [--threshold t --gap g ...] weights.txt seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict importance-table model.txt table.npz
    python -m gkmqc_amd.gkmpredict explain-table [--block Qb] query.fa table.npz out.txt
    python -m gkmqc_amd.gkmpredict hypothetical-table [--block Qb] query.fa table.npz out.txt
    python -m gkmqc_amd.gkmpredict delta [--chunk B] weights.txt seqs.fa variants.tsv out.tsv
    python -m gkmqc_amd.gkmpredict delta-saturation [--chunk B] weights.txt seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict panel [--names a,b,...] panel.npz weights.txt [weights.txt ...]
    python -m gkmqc_amd.gkmpredict predict-panel [--block Qb] query.fa panel.npz out.tsv
    python -m gkmqc_amd.gkmpredict scan-panel --width W [--stride s] [--chunk B] seqs.fa panel.npz out.tsv
    python -m gkmqc_amd.gkmpredict scan-regions-panel --width W [--threshold t,... --gap g ...] panel.npz seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict scan-tail --width W [--thresholds t,... ...] weights.txt seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict scan-quantiles --width W [--q q,... | --ranks r,...] [--collect-cap n ...] weights.txt seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict scan-tail-panel --width W [--thresholds t,... ...] panel.npz seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict scan-quantiles-panel --width W [--q q,... | --ranks r,...] [...] panel.npz seqs.fa out.tsv
    python -m gkmqc_amd.gkmpredict delta-panel [--chunk B] seqs.fa variants.tsv panel.npz out.tsv
  (... stands for scan's --stride and --chunk)

The operations live in gkmmodel, gkmquery, gkmtables, gkmscan and gkmdelta (module map); this module is the
command line, and every public name of those five is importable from here as well.
"""
import argparse
import collections
import os
import sys

import numpy as np

from . import device as dv
from . import svmcv
from .gkmmodel import (C_SVC, EPSILON_SVR, FORMAT, MAX_SVR_SAMPLES, SVR_FORMAT, codes_to_text, load,  # noqa: F401
                       read_targets, text_to_codes, train, train_svr, Model, ModelError)
from .gkmquery import (BLOCK_BYTES, EXPLAIN_CHUNKS, ISM_CHUNKS, check_explainable, check_ism,  # noqa: F401
                       check_queries, default_block, default_explain_block, default_hyp_block, default_ism_block,
                       default_mutscores_block, explain, explain_shares, hypothetical, ism, ism_coefficients,
                       mutant_scores, read_explanation, read_ism, score, write_explanation, write_ism, write_scores)
from .gkmtables import (IMPORTANCE_FORMAT, PANEL_FORMAT, PANEL_MAX_BYTES, PANEL_MAX_MODELS, TABLE_FORMAT,  # noqa: F401
                        TABLE_PIECE, canonical_codes, check_panel, check_table_model, default_imptable_block,
                        default_table_block, explain_with_table, hypothetical_with_table, lmer_classes, lmer_importance,
                        lmer_rc, lmer_text, lmer_weights, load_importance_table, load_lmer_panel, load_lmer_table,
                        pack_lmers, panel_row_stride, read_panel_output, score_with_panel, score_with_table,
                        write_panel_scores, LmerImportanceTable, LmerPanel, LmerTable)
from .gkmscan import (DIST_DIGIT_BITS, DIST_MAX_RANKS, DIST_MAX_THRESHOLDS, REGION_FIELDS, REGION_MAX_GAP,  # noqa: F401
                      SCAN_MAX_WIDTH, check_panel_scan, check_panel_scan_quantiles, check_panel_scan_regions,
                      check_panel_scan_tail_counts, check_scan, check_scan_quantiles, check_scan_regions,
                      check_scan_tail_counts, default_panel_scan_chunk, default_scan_chunk, dist_boundaries,
                      dist_level_bits, keys_to_scores, quantile_ranks, read_long_fasta, read_panel_quantiles,
                      read_panel_regions, read_panel_tail_counts, read_quantiles, read_regions, read_scan,
                      read_tail_counts, scan, scan_chunk_plan, scan_quantiles, scan_quantiles_with_panel, scan_regions,
                      scan_regions_with_panel, scan_tail_counts, scan_tail_counts_with_panel, scan_window_count,
                      scan_with_panel, score_keys, select_order_statistics, stitch_regions, window_validity,
                      write_panel_quantiles, write_panel_regions, write_panel_scan, write_panel_tail_counts,
                      write_quantiles, write_regions, write_scan, write_tail_counts)
from .gkmdelta import (DELTA_MAX_ALLELE, check_delta, check_panel_delta, default_delta_chunk, delta,  # noqa: F401
                       delta_chunk_plan, delta_context, delta_min_chunk, delta_saturation, delta_saturation_chunk_plan,
                       delta_saturation_with_panel, delta_trim, delta_with_panel, read_delta, read_saturation,
                       read_variants, write_delta, write_panel_delta, write_saturation)


# ------------------------------------------------------------------ options: each declared once, shared by reference
def _opt(*flags, **kw):
    return flags, kw


_DEVICE = _opt("--device", type=int, default=0, help="GPU (default: 0)")
_BLOCK = _opt("--block", type=int, default=None, help="queries per device block (default: from device memory)")
_CHUNK = _opt("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
_WINDOWS = (_opt("--width", type=int, required=True, help="bases per window (L..2047)"),
            _opt("--stride", type=int, default=1, help="bases between window starts (default: 1)"), _CHUNK)
_TAIL = _WINDOWS + (_opt("--thresholds", default="", help="comma-separated scores, at most 4096"),)
_QUANTILES = _WINDOWS + (
    _opt("--q", default=None, help="comma-separated quantiles in 0..1, at most 64"),
    _opt("--ranks", default=None, help="comma-separated order statistics 0..n-1 instead of --q"),
    _opt("--collect-cap", type=int, default=1 << 20, help="scores the last pass may gather on the device (default: 2^20)"))
_TRAIN = (
    _opt("-t", "--kernel-type", type=int, default=4, help="kernel type 0..5 (default: 4)"),
    _opt("-L", "--full-word-length", type=int, default=10, help="full word length (default: 10)"),
    _opt("-k", "--non-gap-length", type=int, default=6, help="non-gap positions (default: 6)"),
    _opt("-d", "--max-num-gaps", type=int, default=3, help="max gaps (default: 3)"),
    _opt("-M", "--init-decay", type=int, default=50, help="initial value of the decay, -t 4/5 (default: 50)"),
    _opt("-H", "--half-life-decay", type=float, default=50, help="half life of the decay, -t 4/5 (default: 50)"),
    _opt("-G", "--rbf-gamma", type=float, default=1.0, help="gamma for RBF kernels, -t 3/5 (default: 1.0)"),
    _opt("-C", "--regularization", type=float, default=1.0, help="regularization parameter C (default: 1.0)"),
    _opt("-e", "--precision", type=float, default=0.001, help="precision parameter epsilon (default: 0.001)"),
    _opt("-u", "--shrinking", type=int, choices=(0, 1), default=0, help="shrinking heuristics (default: 0)"))
_TRAIN_SVR = _TRAIN[:8] + (_opt("-p", "--epsilon", type=float, default=0.1,
                                help="epsilon of the insensitive loss (default: 0.1)"),) + _TRAIN[8:]


def _regions(threshold_help):
    return _WINDOWS[:2] + (_opt("--threshold", default="0", help=threshold_help), _opt(
        "--gap", type=int, default=0, help="windows below the threshold a region may bridge (default: 0)"), _CHUNK)


def region_thresholds(text, panel=False):
    """--threshold -> a float, or for a panel a list of them when commas separate several."""
    try:
        values = [float(x) for x in text.split(",")] if panel else [float(text)]
    except ValueError:
        raise ModelError("--threshold: %r is no number%s" % (text, " (or comma-separated numbers)" if panel else ""))
    return values[0] if len(values) == 1 else values


def dist_list(option, text, convert):
    """A comma-separated option -> its values, or None where it was not given."""
    if text is None:
        return None
    try:
        return [convert(x) for x in text.split(",")] if text else []
    except ValueError:
        raise ModelError("%s: %r is no comma-separated list of %s" % (option, text,
                                                                     "integers" if convert is int else "numbers"))


def panel_member_names(paths, names=None):
    """The member names of `panel`: --names split at commas, or the weight files' basenames."""
    if names is None:
        return [os.path.basename(path) for path in paths]
    return names.split(",")


def check_train_args(a):
    """The argument checks `train` makes before it reads anything; an error message or None."""
    bad = dv.check_parameters(a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps)
    if bad:
        return bad
    if not 0 <= a.init_decay <= 255:
        return "-M must lie in 0..255"
    if not (a.regularization > 0 and a.precision > 0):
        return "-C and -e must be positive"
    if a.cmd == "train-svr" and not (np.isfinite(a.epsilon) and a.epsilon >= 0):
        return "-p must be finite and at least 0"
    return None


# ------------------------------------------------------------------ what each command runs
# A row of COMMANDS:
#   help         the subparser's
#   options      add_argument's arguments in order, from _opt
#   positionals  the same; a bare string is a positional of that name
#   files        the positionals that must name files
#   run(a, tmp)  load, check, compute, write to tmp -> the line for stderr or None; main() then moves tmp to a.output
#   check(a)     the refusals from the arguments alone, before main() looks for the files
#   saves        run puts the output in place itself, through the save() of what it made, and gets tmp = None
_Command = collections.namedtuple("_Command", "help options positionals files run check saves", defaults=(None, False))


def _check_train(a):
    bad = check_train_args(a)
    if bad:
        raise ModelError(bad)


def _check_block(a):
    if a.block is not None and a.block < 1:
        raise ModelError("--block must be at least 1")


def _run_train(a, tmp):
    kernel_args = (a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps, a.init_decay,
                   a.half_life_decay, a.rbf_gamma, a.regularization)
    if a.cmd == "train-svr":
        m = train_svr(a.seqs_fa, a.targets, *kernel_args, a.epsilon, a.precision, bool(a.shrinking), a.device)
        m.save(a.model)
        return "%d support vectors, rho %r (LIBSVM's: %r), %d iterations -> %s" % (m.n_sv, m.rho, -m.rho, m.n_iter, a.model)
    m = train(a.pos_fa, a.neg_fa, *kernel_args, a.precision, bool(a.shrinking), a.device)
    m.save(a.model)
    return "%d support vectors (%d negative, %d positive), rho %r -> %s" % (m.n_sv, m.n0, m.n_sv - m.n0, m.rho, a.model)


def _run_weights(a, tmp):
    m = load(a.model)
    check_table_model(m)
    lmer_weights(m, a.device).save(a.output)


def _run_importance_table(a, tmp):
    m = load(a.model)
    check_explainable(m, "importance-table")
    lmer_importance(m, a.device).save(a.output)


def _run_panel(a, tmp):
    names = panel_member_names(a.weights, a.names)
    if len(names) != len(a.weights):
        raise ModelError("panel: %d names for %d weight files" % (len(names), len(a.weights)))
    if len(a.weights) > PANEL_MAX_MODELS:
        raise ModelError("panel: %d weight files; a panel holds 1..%d tables" % (len(a.weights), PANEL_MAX_MODELS))
    LmerPanel([load_lmer_table(path) for path in a.weights], names).save(a.output)


# the commands that serve a query file from a model or a table: command -> (compute, writer)
_QUERY_COMMANDS = {
    "predict": (score, write_scores),
    "explain": (explain, write_explanation),
    "ism": (ism, write_ism),
    "mutant-scores": (mutant_scores, write_ism),
    "hypothetical": (hypothetical, write_ism),
    "predict-table": (score_with_table, write_scores),
    "explain-table": (explain_with_table, write_explanation),
    "hypothetical-table": (hypothetical_with_table, write_ism),
}


def _query(help, source, load_source):
    """The table row of a _QUERY_COMMANDS command; source: the positional that names the model or table file."""
    def run(a, tmp):
        compute, write = _QUERY_COMMANDS[a.cmd]
        names, values = compute(load_source(getattr(a, source)), a.query_fa, a.device, a.block)
        write(tmp, names, values)
    return _Command(help, (_DEVICE, _BLOCK), ("query_fa", source, "output"), ("query_fa",), run, _check_block)


def _run_predict_panel(a, tmp):
    panel = load_lmer_panel(a.panel)
    names, values = score_with_panel(panel, a.query_fa, a.device, a.block)
    write_panel_scores(tmp, panel.names, names, values)


def _run_scan(a, tmp):
    if a.cmd == "scan-panel":
        panel = load_lmer_panel(a.panel)
        check_panel_scan(panel, a.width, a.stride, a.chunk)
        results = scan_with_panel(panel, a.seqs_fa, a.width, a.stride, a.device, a.chunk)
        omitted, models = write_panel_scan(tmp, panel.names, results, a.width), " for %d models" % panel.n_models
    else:
        tab = load_lmer_table(a.weights)
        check_scan(tab, a.width, a.stride, a.chunk)
        results = scan(tab, a.seqs_fa, a.width, a.stride, a.device, a.chunk)
        omitted, models = write_scan(tmp, results, a.width), ""
    return ("%d windows scored%s, %d over a non-ACGT character left out -> %s"
            % (sum(len(r[1]) for r in results) - omitted, models, omitted, a.output))


def _run_regions(a, tmp):
    panel = a.cmd == "scan-regions-panel"
    threshold = region_thresholds(a.threshold, panel)
    if panel:
        folded = load_lmer_panel(a.panel)
        check_panel_scan_regions(folded, a.width, a.stride, threshold, a.gap, a.chunk)
        results = scan_regions_with_panel(folded, a.seqs_fa, a.width, a.stride, threshold, a.gap, a.device, a.chunk)
        n = write_panel_regions(tmp, folded.names, results)
    else:
        folded = load_lmer_table(a.weights)
        check_scan_regions(folded, a.width, a.stride, threshold, a.gap, a.chunk)
        results = scan_regions(folded, a.seqs_fa, a.width, a.stride, threshold, a.gap, a.device, a.chunk)
        n = write_regions(tmp, results)
    return "%d regions at a threshold of %s, gap %d -> %s" % (n, a.threshold, a.gap, a.output)


def _run_dist(a, tmp):
    panel = a.cmd.endswith("-panel")
    folded = load_lmer_panel(a.panel) if panel else load_lmer_table(a.weights)
    if a.cmd.startswith("scan-tail"):
        thresholds = dist_list("--thresholds", a.thresholds, float)
        check, compute = ((check_panel_scan_tail_counts, scan_tail_counts_with_panel) if panel else
                          (check_scan_tail_counts, scan_tail_counts))
        check(folded, a.width, a.stride, thresholds, a.chunk)
        result = compute(folded, a.seqs_fa, a.width, a.stride, thresholds, a.device, a.chunk)
        (write_panel_tail_counts(tmp, folded.names, result) if panel else write_tail_counts(tmp, result))
        what = "%d thresholds" % len(thresholds)
    else:
        q, ranks = dist_list("--q", a.q, float), dist_list("--ranks", a.ranks, int)
        check, compute = ((check_panel_scan_quantiles, scan_quantiles_with_panel) if panel else
                          (check_scan_quantiles, scan_quantiles))
        check(folded, a.width, a.stride, q, ranks, a.chunk, a.collect_cap)
        result = compute(folded, a.seqs_fa, a.width, a.stride, q, ranks, a.device, a.chunk, a.collect_cap)
        (write_panel_quantiles(tmp, folded.names, result) if panel else write_quantiles(tmp, result))
        what = "%d order statistics in %d scans" % (len(q if ranks is None else ranks), len(result["passes"]))
    return "%s of %s scored windows -> %s" % (what, np.max(result["scored"]), a.output)


def _run_delta(a, tmp):
    if a.cmd == "delta-panel":
        panel = load_lmer_panel(a.panel)
        check_panel_delta(panel, chunk=a.chunk)
        variants = read_variants(a.variants)
        values = delta_with_panel(panel, a.seqs_fa, variants, a.device, a.chunk)
        write_panel_delta(tmp, panel.names, variants, values)
        bad, models = int(np.isnan(values).any(axis=1).sum()) if len(values) else 0, " for %d models" % panel.n_models
    else:
        tab = load_lmer_table(a.weights)
        check_delta(tab, chunk=a.chunk)
        variants = read_variants(a.variants)
        values = delta(tab, a.seqs_fa, variants, a.device, a.chunk)
        write_delta(tmp, variants, values)
        bad, models = int(np.isnan(values).sum()), ""
    return "%d variants scored%s, %d over a non-ACGT character (nan) -> %s" % (len(values) - bad, models, bad, a.output)


def _run_delta_saturation(a, tmp):
    tab = load_lmer_table(a.weights)
    check_delta(tab, chunk=a.chunk)
    results = delta_saturation(tab, a.seqs_fa, a.device, a.chunk)
    omitted = write_saturation(tmp, results, a.seqs_fa)
    return ("%d positions scored, %d near a non-ACGT character left out -> %s"
            % (sum(len(r[1]) for r in results) - omitted, omitted, a.output))


# ------------------------------------------------------------------ the command table
COMMANDS = {
    "train": _Command("train on pos.fa + neg.fa and write a model file", _TRAIN + (_DEVICE,), ("pos_fa", "neg_fa", "model"),
                      ("pos_fa", "neg_fa"), _run_train, _check_train, saves=True),
    "train-svr": _Command("fit an epsilon-SVR to seqs.fa and targets.txt (name<TAB>value per record) and write a model file",
                          _TRAIN_SVR + (_DEVICE,), ("seqs_fa", "targets", "model"), ("seqs_fa", "targets"), _run_train,
                          _check_train, saves=True),
    "predict": _query("score the sequences of query.fa: name<TAB>score per line, in file order", "model", load),
    "explain": _query("per-base importance of the sequences of query.fa: name<TAB>v0,v1,... per line", "model", load),
    "ism": _query("in-silico mutagenesis of the sequences of query.fa: name<TAB>4T values per line, position-major, columns "
                  "A, C, G, T", "model", load),
    "mutant-scores": _query("the score of every single-base mutant of the sequences of query.fa, RBF models included: "
                            "name<TAB>4T values per line, position-major, columns A, C, G, T (the ism format)", "model", load),
    "hypothetical": _query("hypothetical importance of the sequences of query.fa: name<TAB>4T values per line, "
                           "position-major, columns A, C, G, T (the ism format)", "model", load),
    "weights": _Command("fold a model into its l-mer weight table: a `# key value` header, then LMER<TAB>weight per "
                        "canonical l-mer", (_DEVICE,), ("model", "output"), (), _run_weights, saves=True),
    "predict-table": _query("score the sequences of query.fa from an l-mer weight table: name<TAB>score per line, in file "
                            "order (the predict format)", "weights", load_lmer_table),
    "scan": _Command("score every window of --width bases of the sequences of seqs.fa (any length) from an l-mer weight "
                     "table: name<TAB>start<TAB>end<TAB>score per window, windows over a non-ACGT character left out",
                     _WINDOWS + (_DEVICE,), ("seqs_fa", "weights", "output"), ("seqs_fa",), _run_scan),
    "scan-regions": _Command("scan the sequences of seqs.fa with an l-mer weight table and report the regions whose windows "
                             "score at least --threshold: name<TAB>start<TAB>end<TAB>peak<TAB>summit<TAB>windows per region",
                             _regions("the score a window must reach (default: 0, the decision boundary)") + (_DEVICE,),
                             ("weights", "seqs_fa", "output"), ("seqs_fa",), _run_regions),
    "importance-table": _Command("fold a model into its per-base importance table: one value per (l-mer, offset), a binary "
                                 ".npz file", (_DEVICE,), ("model", "output"), (), _run_importance_table, saves=True),
    "explain-table": _query("per-base importance of the sequences of query.fa from an importance table: name<TAB>v0,v1,... "
                            "per line (the explain format)", "table", load_importance_table),
    "hypothetical-table": _query("hypothetical importance of the sequences of query.fa from an importance table: "
                                 "name<TAB>4T values per line (the ism format)", "table", load_importance_table),
    "delta": _Command("the effect of the variants of variants.tsv (name<TAB>pos<TAB>ref<TAB>alt[<TAB>id], pos 1-based) on "
                      "the sequences of seqs.fa (any length) from an l-mer weight table (deltaSVM): the same columns plus "
                      "the delta, nan over a non-ACGT character", (_CHUNK, _DEVICE),
                      ("weights", "seqs_fa", "variants", "output"), ("seqs_fa", "variants"), _run_delta),
    "delta-saturation": _Command("the effect of every single-base substitution of the sequences of seqs.fa from an l-mer "
                                 "weight table: name<TAB>pos<TAB>ref<TAB>dA<TAB>dC<TAB>dG<TAB>dT per position, positions "
                                 "near a non-ACGT character left out", (_CHUNK, _DEVICE), ("weights", "seqs_fa", "output"),
                                 ("seqs_fa",), _run_delta_saturation),
    "panel": _Command("join 1..64 l-mer weight tables that share their kernel parameters into a panel, a binary .npz file; "
                      "the members are named after the files",
                      (_opt("--names", default=None, help="comma-separated member names (default: the files' basenames)"),),
                      ("output", _opt("weights", nargs="+")), (), _run_panel, saves=True),
    "predict-panel": _Command("score the sequences of query.fa with every member of a panel: a header, then name<TAB>one "
                              "score per member", (_DEVICE, _BLOCK), ("query_fa", "panel", "output"), ("query_fa",),
                              _run_predict_panel, _check_block),
    "scan-panel": _Command("scan the sequences of seqs.fa with every member of a panel: a header, then "
                           "name<TAB>start<TAB>end<TAB>one score per member", _WINDOWS + (_DEVICE,),
                           ("seqs_fa", "panel", "output"), ("seqs_fa",), _run_scan),
    "scan-regions-panel": _Command("scan-regions for every member of a panel: the member's name, then scan-regions' columns",
                                   _regions("one value for all members or one per member, comma-separated (default: 0)")
                                   + (_DEVICE,), ("panel", "seqs_fa", "output"), ("seqs_fa",), _run_regions),
    "scan-tail": _Command("how many scored windows of a scan reach each of --thresholds, all records pooled: "
                          "#scored<TAB>n<TAB>unscored<TAB>m, then threshold<TAB>count", _TAIL + (_DEVICE,),
                          ("weights", "seqs_fa", "output"), ("seqs_fa",), _run_dist),
    "scan-quantiles": _Command("exact quantiles (--q) or order statistics (--ranks) of a scan's scores, all records pooled: "
                               "#scored<TAB>n<TAB>unscored<TAB>m, then q<TAB>rank<TAB>value", _QUANTILES + (_DEVICE,),
                               ("weights", "seqs_fa", "output"), ("seqs_fa",), _run_dist),
    "scan-tail-panel": _Command("scan-tail for every member of a panel: the member's name in front", _TAIL + (_DEVICE,),
                                ("panel", "seqs_fa", "output"), ("seqs_fa",), _run_dist),
    "scan-quantiles-panel": _Command("scan-quantiles for every member of a panel: the member's name in front",
                                     _QUANTILES + (_DEVICE,), ("panel", "seqs_fa", "output"), ("seqs_fa",), _run_dist),
    "delta-panel": _Command("the effect of the variants of variants.tsv on the sequences of seqs.fa for every member of a "
                            "panel: a header, then the variant's columns and one delta per member", (_CHUNK, _DEVICE),
                            ("seqs_fa", "variants", "panel", "output"), ("seqs_fa", "variants"), _run_delta),
}


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gkmqc_amd.gkmpredict",
                                description="train a gkm-SVM on all sequences / score FASTA sequences with it (MI355X)")
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, c in COMMANDS.items():
        s = sub.add_parser(name, help=c.help)
        for flags, kw in (_opt(x) if isinstance(x, str) else x for x in c.options + c.positionals):
            s.add_argument(*flags, **kw)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    c = COMMANDS[a.cmd]
    try:
        if c.check is not None:
            c.check(a)
        for path in (getattr(a, key) for key in c.files):
            if not os.path.isfile(path):
                raise ModelError("cannot read %s" % path)
        tmp = None if c.saves else a.output + ".tmp"
        line = c.run(a, tmp)
        if tmp is not None:
            os.replace(tmp, a.output)
        if line is not None:
            print(line, file=sys.stderr)
    except (ModelError, dv.GkmError, svmcv.SvmError, OSError) as e:
        print("gkmpredict: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
