"""Whole l-mer weight panels from one labelled pool: every task of a label file trained from one Gram
matrix, and any list of models that share their kernel parameters folded into a panel with one comparison pass.

    train_panel   one pool of sequences, one label column per task: one gram_matrix, one svmcv.train_tasks call, one Model
                  per task -- the model `train` gives on the task's own positives and negatives, byte for byte
    fold_panel    1..64 trained models -> LmerPanel: the union of their canonical classes, one coefficient column per
                  model, and k_panel_weights over all 4^L codes straight into the panel's device image; column m is
                  lmer_weights(models[m]).W bit for bit

    python -m gkmqc_amd.gkmpanels train [-t -L -k -d -M -H -G -C -e -u] [--class-weight none|balanced|W0:W1] [--panel out.npz] seqs.fa labels.tsv out_prefix
    python -m gkmqc_amd.gkmpanels fold [--names a,b,...] out.npz model.txt [model.txt ...]

`train` writes out_prefix.<task>.model.txt per task (and the folded panel with --panel); `fold` reads model files.  The
label file: a header line name<TAB>task..., then per FASTA record, in FASTA order, its name and per
task 1, 0 or . (not part of that task).
"""
import argparse
import collections
import logging
import os
import sys
import time

import numpy as np

from . import device as dv
from . import svmcv
from .gkmmodel import Model, ModelError, load, resolve_class_weight
from .gkmpredict import _DEVICE, _TRAIN, _opt, check_train_args
from .gkmselect import _CLASS_WEIGHT, parse_class_weight
from .gkmquery import _exact_norms
from .gkmtables import (_PANEL_SHARED, PANEL_MAX_MODELS, TABLE_PIECE, LmerPanel, _check_panel_names, _check_panel_size,
                        check_table_model, lmer_classes, panel_row_stride)

NOT_IN_TASK = -1     # read_labels' value for `.`


# ------------------------------------------------------------------ the label file
def read_labels(path, names):
    """The label file of `train_panel` -> (task names, Y): Y int8 (records, tasks) of 1, 0 and NOT_IN_TASK (`.`).  The
    header is name<TAB>task<TAB>...; every other line is a FASTA record's name (split off at the task columns: names may
    hold tabs) and one of 1, 0, . per task, the records in FASTA order (names: the headers the FASTA reader returned; the
    rule of read_targets).  Anything malformed raises ModelError with the line number; a task without both a 1 and a 0
    is refused by name."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines:
        raise ModelError("%s:1: no header line name<TAB>task..." % path)
    head = lines[0].split("\t")
    if head[0] != "name" or len(head) < 2:
        raise ModelError("%s:1: the header must be name<TAB>task..., with at least one task" % path)
    try:
        tasks = _check_panel_names(head[1:], len(head) - 1)
    except ModelError as e:
        raise ModelError("%s:1: %s" % (path, e))
    nt = len(tasks)
    Y = np.empty((len(names), nt), dtype=np.int8)
    value = {"1": 1, "0": 0, ".": NOT_IN_TASK}
    for j, line in enumerate(lines[1:]):
        at = j + 2
        if j >= len(names):
            raise ModelError("%s:%d: more label lines than FASTA records (%d)" % (path, at, len(names)))
        parts = line.rsplit("\t", nt)
        if len(parts) != nt + 1:
            raise ModelError("%s:%d: expected name<TAB>%d label(s)" % (path, at, nt))
        if parts[0] != names[j]:
            raise ModelError("%s:%d: name %r, but FASTA record %d is %r" % (path, at, parts[0], j + 1, names[j]))
        for t, x in enumerate(parts[1:]):
            if x not in value:
                raise ModelError("%s:%d: the label of task %s must be 1, 0 or ., not %r" % (path, at, tasks[t], x))
            Y[j, t] = value[x]
    if len(lines) - 1 < len(names):
        n = len(lines) - 1
        raise ModelError("%s:%d: no labels for FASTA record %d (%r): %d lines for %d records"
                         % (path, len(lines) + 1, n + 1, names[n], n, len(names)))
    check_labels(tasks, Y, path + ": ")
    return tasks, Y


def check_labels(tasks, Y, where=""):
    """Every task needs a 1 and a 0 among its labels; the first that lacks one is refused by name."""
    for t, task in enumerate(tasks):
        for lab, word in ((1, "positive (1)"), (0, "negative (0)")):
            if not (Y[:, t] == lab).any():
                raise ModelError("%stask %s has no %s record" % (where, task, word))


# ------------------------------------------------------------------ training all tasks from one Gram matrix
def task_problems(Y):
    """Per task the pool indices that take part, ascending, and their labels -> (trains, labels) as svmcv.train_tasks
    takes them."""
    trains = [np.flatnonzero(Y[:, t] != NOT_IN_TASK) for t in range(Y.shape[1])]
    return trains, [Y[tr, t].astype(np.int64) for t, tr in enumerate(trains)]


def train_panel(fasta, labels, kernel_type=4, L=10, k=6, d=3, M=50, H=50, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
                device=0, class_weight=None):
    """One C-SVC per task of a labelled pool -> (task names, [Model]).  fasta: the pool; labels: a label file
    (read_labels) or (task names, Y) with Y (records, tasks) of 1, 0 and NOT_IN_TASK.  One Gram matrix of the pool and
    one svmcv.train_tasks call: every task's kernel matrix is a sub-matrix of the pool's (K[i, j] depends on the pair
    alone, bit for bit), and a task is its index list in LIBSVM's order.  models[t].save writes the bytes that
    `train(pos_t.fa, neg_t.fa, ...)` writes for the task's label-1 and label-0 records in pool order.  A task that stops
    at the GPU solver's iteration cap is re-solved with scikit-learn, as `train` does, that task alone.
    class_weight (None, "balanced" or a pair (w0, w1), as `train`): "balanced" is resolved per task from the task's own
    counts, and the contract holds with the same argument: train(pos_t.fa, neg_t.fa, ..., class_weight=class_weight)."""
    import torch
    bad = dv.check_parameters(kernel_type, L, k, d)
    if bad:
        raise ModelError("kernel parameters rejected: %s" % bad)
    seqs, names, _, _ = dv.read_fasta(fasta)
    if len(seqs) == 0:
        raise ModelError("training needs at least one positive and one negative sequence")
    if isinstance(labels, (str, bytes, os.PathLike)):
        tasks, Y = read_labels(labels, names)
    else:
        tasks, Y = labels
        Y = np.asarray(Y, dtype=np.int8)
        if Y.ndim != 2 or Y.shape[0] != len(seqs):
            raise ModelError("labels: Y must be (records, tasks) = (%d, tasks)" % len(seqs))
        tasks = _check_panel_names(tasks, Y.shape[1])
        if not np.isin(Y, (0, 1, NOT_IN_TASK)).all():
            raise ModelError("labels: every entry of Y must be 1, 0 or NOT_IN_TASK")
        check_labels(tasks, Y)
    trains, labs = task_problems(Y)
    res = dv.gram_matrix(seqs, kernel_type, L, k, d, M, H, gamma, device, symmetric=True, keep_context=True)
    K = res["K"]
    weights = [resolve_class_weight(class_weight, lab) for lab in labs]
    sol, _ = svmcv.train_tasks(K, trains, labs, C, tol, shrinking, class_weight=None if class_weight is None else weights)
    models = []
    for t, (tr, lab) in enumerate(zip(trains, labs)):
        if sol.iters[t] >= 0:
            a, order = sol.alpha[t], sol.idx[t]
            sv = np.nonzero(a > 0)[0]
            idx, alpha, rho = order[sv], a[sv], float(sol.rho[t])
        else:   # the GPU solver's iteration cap: the reference's solver has none (as gkmmodel.train)
            from sklearn.svm import SVC
            logging.warning("task %s re-solved with scikit-learn (iteration cap of the GPU solver)", tasks[t])
            m = SVC(kernel="precomputed", C=C, tol=tol, shrinking=bool(shrinking),
                    class_weight=None if weights[t] is None else {0: weights[t][0], 1: weights[t][1]})
            m.fit(svmcv.device_block(K, tr, tr).cpu().numpy(), lab)
            idx, alpha, rho = tr[m.support_], np.abs(m.dual_coef_[0]), float(m.intercept_[0])
        n0 = int((Y[idx, t] == 0).sum())
        models.append(Model(kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, rho, n0, alpha,
                            [names[i] for i in idx], [seqs[i] for i in idx], class_weight=weights[t]))
    del K, res
    torch.cuda.empty_cache()
    return tasks, models


# ------------------------------------------------------------------ the fold
def check_fold(models, names=None):
    """What fold_panel refuses before it touches the device, in LmerPanel's words -> the member names."""
    models = list(models)
    for i, m in enumerate(models):
        if not isinstance(m, Model):
            raise ModelError("panel: member %d is no trained model (gkmpredict train)" % i)
    if not models:
        raise ModelError("panel: 0 members; a panel holds 1..%d tables" % PANEL_MAX_MODELS)
    names = _check_panel_names(["table%d" % i for i in range(len(models))] if names is None else names, len(models))
    for i, m in enumerate(models):
        check_table_model(m, "panel: member %d (%s)" % (i, names[i]))
        for key in _PANEL_SHARED:
            if getattr(m, key) != getattr(models[0], key):
                raise ModelError("panel: member %d (%s) has %s = %r where member 0 (%s) has %r; the members must share %s"
                                 % (i, names[i], key, getattr(m, key), names[0], getattr(models[0], key),
                                    ", ".join(_PANEL_SHARED)))
    _check_panel_size(models[0].L, len(models))
    return names


def panel_classes(models, sqs, ms=None):
    """(v, CV): the ascending union v of the models' canonical classes and CV float64 (len(v), ms), ms =
    panel_row_stride(len(models)) by default: per model m the classes (v_m, cv_m) of lmer_classes(models[m], sqs[m])
    scattered as CV[searchsorted(v, v_m), m] = cv_m, 0.0 elsewhere.  A class a model lacks adds +-0.0 to an accumulator
    that is never -0.0, so column m of the fold keeps the bits of the model's own table."""
    per = [lmer_classes(m, sq) for m, sq in zip(models, sqs)]
    v = np.unique(np.concatenate([p[0] for p in per])).astype(np.uint32)
    ms = panel_row_stride(len(models)) if ms is None else int(ms)
    CV = np.zeros((len(v), ms), dtype=np.float64)
    for m, (vm, cvm) in enumerate(per):
        CV[np.searchsorted(v, vm), m] = cvm
    return v, CV


def fold_panel(models, names=None, device=0, on_piece=None):
    """1..PANEL_MAX_MODELS trained models that share (kernel_type, L, k, d, M, H) -> LmerPanel: W[:, m]
    is lmer_weights(models[m]).W bit for bit and rho[m] = models[m].rho.  Per model the exact self norms of its support
    vectors (as lmer_weights takes them) and its classes on the host (panel_classes); then k_panel_weights over all 4^L
    codes in pieces of TABLE_PIECE, into the panel's device image: the comparisons once for all members.  RBF models are
    refused as `weights` refuses them, everything else in LmerPanel's words, before the device is touched.
    on_piece(dict) (measurements): called after every piece with lmer_weights' fields, n_models and classes_ms (the
    host's time in panel_classes, the same for every piece)."""
    import torch
    models = list(models)
    names = check_fold(models, names)
    first = models[0]
    L, d, nm = first.L, first.d, len(models)
    ms = panel_row_stride(nm)
    ctx = dv.cached_context(*first.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    c = dv.mismatch_weights(first.kernel_type, L, first.k)[:d + 1]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        sqs = []
        for m in models:
            ctx.set_sequences(m.flat_seqs(), stream)
            sq = torch.empty(m.n_sv, dtype=torch.float64, device=dev)
            _exact_norms(ctx, m.n_sv, c, sq, stream)
            sqs.append(sq.cpu().numpy())
        t0 = time.perf_counter()
        v, CV = panel_classes(models, sqs, ms)
        classes_ms = (time.perf_counter() - t0) * 1e3
        d_v = torch.from_numpy(v.view(np.int32)).to(dev)
        d_CV = torch.from_numpy(CV).to(dev)
        del CV
        P = torch.empty((4 ** L, ms), dtype=torch.float64, device=dev)
        for u0 in range(0, 4 ** L, TABLE_PIECE):
            u1 = min(4 ** L, u0 + TABLE_PIECE)
            ctx.panel_weights(c, d_v.data_ptr(), d_CV.data_ptr(), len(v), nm, ms, u0, u1, P.data_ptr() + 8 * ms * u0, stream)
            if on_piece is not None:
                on_piece(dict(codes=u1 - u0, classes=len(v), kernel_ms=ctx.last_kernel_ms(),
                              comparisons=ctx.last_comparisons(), kernel=ctx.last_kernel_name(), n_models=nm,
                              classes_ms=classes_ms))
        W = P[:, :nm].cpu().numpy()
    panel = LmerPanel.__new__(LmerPanel)
    panel._fill(W, names, [m.rho for m in models], *(getattr(first, key) for key in _PANEL_SHARED))
    return panel


# ------------------------------------------------------------------ command line
def model_path(prefix, task):
    return "%s.%s.model.txt" % (prefix, task)


def _run_train(a):
    bad = check_train_args(a)
    if bad:
        raise ModelError(bad)
    weights = parse_class_weight(a.class_weight)
    for path in (a.seqs_fa, a.labels):
        if not os.path.isfile(path):
            raise ModelError("cannot read %s" % path)
    _, names, _, _ = dv.read_fasta(a.seqs_fa)
    tasks, Y = read_labels(a.labels, names)
    for task in tasks:
        if os.sep in task or (os.altsep and os.altsep in task):
            raise ModelError("train: the task name %r cannot be part of a file name" % task)
    tasks, models = train_panel(a.seqs_fa, (tasks, Y), a.kernel_type, a.full_word_length, a.non_gap_length,
                                a.max_num_gaps, a.init_decay, a.half_life_decay, a.rbf_gamma, a.regularization,
                                a.precision, bool(a.shrinking), a.device,
                                **({} if weights is None else dict(class_weight=weights)))
    panel = fold_panel(models, tasks, a.device) if a.panel is not None else None
    for task, m in zip(tasks, models):     # (Model.save and LmerPanel.save put a complete file in place or none)
        m.save(model_path(a.out_prefix, task))
    if panel is not None:
        panel.save(a.panel)
    return "%d tasks, %d records -> %s%s" % (len(tasks), len(names), model_path(a.out_prefix, "<task>"),
                                            "" if panel is None else " and " + a.panel)


def _run_fold(a):
    names = None if a.names is None else a.names.split(",")
    if names is not None and len(names) != len(a.models):
        raise ModelError("fold: %d names for %d model files" % (len(names), len(a.models)))
    if len(a.models) > PANEL_MAX_MODELS:
        raise ModelError("fold: %d model files; a panel holds 1..%d tables" % (len(a.models), PANEL_MAX_MODELS))
    for path in a.models:
        if not os.path.isfile(path):
            raise ModelError("cannot read %s" % path)
    if names is None:
        names = [os.path.basename(path) for path in a.models]
    fold_panel([load(path) for path in a.models], names, a.device).save(a.output)
    return "%d models -> %s" % (len(a.models), a.output)


# A row of COMMANDS: the subparser's help, add_argument's arguments in order (from gkmpredict's _opt; a bare string is a
# positional of that name), and run(a) -> the line for stderr: it refuses a missing input by name before it computes, and
# puts every output in place through a save() that writes a complete file or none
Command = collections.namedtuple("Command", "help options positionals run")
COMMANDS = {
    "train": Command("train one model per task of labels.tsv on the pool seqs.fa from one Gram matrix: "
                     "out_prefix.<task>.model.txt per task",
                     _TRAIN + (_CLASS_WEIGHT, _DEVICE, _opt("--panel", default=None, help="also fold the models into this panel file")),
                     ("seqs_fa", "labels", "out_prefix"), _run_train),
    "fold": Command("fold 1..64 model files that share their kernel parameters into a panel file in one pass",
                    (_opt("--names", default=None, help="comma-separated member names (default: the files' basenames)"),
                     _DEVICE), ("output", _opt("models", nargs="+", metavar="model")), _run_fold),
}


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gkmqc_amd.gkmpanels", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, c in COMMANDS.items():
        s = sub.add_parser(name, help=c.help)
        for flags, kw in (_opt(x) if isinstance(x, str) else x for x in c.options + c.positionals):
            s.add_argument(*flags, **kw)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        print(COMMANDS[a.cmd].run(a), file=sys.stderr)
    except (ModelError, dv.GkmError, svmcv.SvmError, OSError) as e:
        print("gkmpanels: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
