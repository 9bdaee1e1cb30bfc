"""Class weights and the choice of C for a gkm-SVM: the command line of gkmmodel.train's `class_weight`
and of gkmmodel.select, the cross-validation of a whole grid of settings on one Gram matrix and one solver launch.

    python -m gkmqc_amd.gkmselect train [-t -L -k -d -M -H -G -C -e -u] [--class-weight none|balanced|W0:W1] pos.fa neg.fa model.txt
    python -m gkmqc_amd.gkmselect cv-grid [-t -L -k -d -M -H -G -e -u] -C 0.01,0.1,1,10 [--class-weight none,balanced,W0:W1]
                                          [--ncv 5 --repeats 1 --seed 1] pos.fa neg.fa out.tsv

`train` is gkmpredict's `train` with class weights: W0 weighs label 0 (neg.fa), W1 label 1 (pos.fa); alpha of a class is
bounded by C times its weight (scikit-learn's `class_weight`, LIBSVM's -wi).  A weighted model is a `gkmqc-model-2` file
(INTEGRATION.md §5b); `--class-weight none` writes the bytes gkmpredict's `train` writes.  (gkmpredict's own command
table is pinned as it is; gkmpanels' `train` takes the same option.)

`cv-grid` writes one line per setting, C outermost: C<TAB>class_weight<TAB>auc_mean<TAB>auc_std<TAB>capped under a header,
floats as repr(), and prints the best setting: the highest mean AUC, on a tie the smaller C, then the earlier weighting.
"""
import argparse
import collections
import os
import sys

import numpy as np

from . import device as dv
from . import svmcv
from .gkmmodel import ModelError, select, train
from .gkmpredict import _DEVICE, _TRAIN, _opt, check_train_args

GRID_HEADER = "C\tclass_weight\tauc_mean\tauc_std\tcapped"
_CLASS_WEIGHT = _opt("--class-weight", default="none",
                     help="none, balanced, or W0:W1 -- the weights of label 0 (negatives) and label 1 (default: none)")


def parse_class_weight(text):
    """--class-weight of a `train` -> None, "balanced" or (w0, w1); anything else raises ModelError."""
    if text == "none":
        return None
    if text == "balanced":
        return "balanced"
    parts = text.split(":")
    try:
        if len(parts) != 2:
            raise ValueError
        w = (float(parts[0]), float(parts[1]))
    except ValueError:
        raise ModelError("--class-weight: %r is not none, balanced or W0:W1" % text)
    if not all(np.isfinite(x) and x > 0 for x in w):
        raise ModelError("--class-weight: the weights must be finite and > 0, not %r" % text)
    return w


def parse_class_weights(text):
    """--class-weight of `cv-grid`: a comma-separated list of parse_class_weight's settings, at least one"""
    if not text:
        raise ModelError("--class-weight: an empty list")
    return [parse_class_weight(x) for x in text.split(",")]


def parse_Cs(text):
    """-C of `cv-grid`: comma-separated values of C, each finite and > 0, at least one"""
    try:
        Cs = [float(x) for x in text.split(",")]
    except ValueError:
        raise ModelError("-C: %r is no comma-separated list of numbers" % text)
    if not all(np.isfinite(C) and C > 0 for C in Cs):
        raise ModelError("-C: every value must be finite and > 0")
    return Cs


def class_weight_text(cw):
    """what parse_class_weight reads back to cw"""
    return "none" if cw is None else cw if isinstance(cw, str) else "%r:%r" % (float(cw[0]), float(cw[1]))


def write_grid(path, records):
    """cv-grid's output: GRID_HEADER, then one line per record of svmcv.cross_validate_grid, floats as repr()"""
    with open(path, "w") as f:
        f.write(GRID_HEADER + "\n")
        for r in records:
            f.write("%r\t%s\t%r\t%r\t%d\n" % (float(r["C"]), class_weight_text(r["class_weight"]), float(r["auc_mean"]),
                                              float(r["auc_std"]), int(r["capped"])))


def read_grid(path):
    """the records write_grid wrote, the same doubles"""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines or lines[0] != GRID_HEADER:
        raise ModelError("%s:1: expected the header %r" % (path, GRID_HEADER))
    out = []
    for j, line in enumerate(lines[1:]):
        parts = line.split("\t")
        try:
            if len(parts) != 5:
                raise ValueError("expected 5 columns")
            out.append(dict(C=float(parts[0]), class_weight=parse_class_weight(parts[1]), auc_mean=float(parts[2]),
                            auc_std=float(parts[3]), capped=int(parts[4])))
        except ValueError as e:
            raise ModelError("%s:%d: %s" % (path, j + 2, e))
    return out


def _kernel_args(a):
    return (a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps, a.init_decay, a.half_life_decay,
            a.rbf_gamma)


def _check(a):
    bad = check_train_args(a)
    if bad:
        raise ModelError(bad)
    for path in (a.pos_fa, a.neg_fa):
        if not os.path.isfile(path):
            raise ModelError("cannot read %s" % path)


def _run_train(a):
    weights = parse_class_weight(a.class_weight)
    _check(a)
    m = train(a.pos_fa, a.neg_fa, *_kernel_args(a), a.regularization, a.precision, bool(a.shrinking), a.device,
              class_weight=weights)
    m.save(a.model)
    return "%d support vectors (%d negative, %d positive), rho %r, class weights %s -> %s" % (
        m.n_sv, m.n0, m.n_sv - m.n0, m.rho, class_weight_text(m.class_weight), a.model)


def _run_cv_grid(a):
    Cs, weights = parse_Cs(a.regularization), parse_class_weights(a.class_weight)
    if a.ncv < 2 or a.repeats < 1:
        raise ModelError("--ncv must be at least 2 and --repeats at least 1")
    a.regularization = Cs[0]        # (check_train_args reads one C)
    _check(a)
    records, best = select(a.pos_fa, a.neg_fa, Cs, weights, a.ncv, a.repeats, a.seed, *_kernel_args(a), a.precision,
                           bool(a.shrinking), a.device)
    tmp = a.output + ".tmp"
    try:
        write_grid(tmp, records)
        os.replace(tmp, a.output)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    b = records[best]
    return "%d settings -> %s; best: C %r, class weights %s, mean AUC %r (std %r)" % (
        len(records), a.output, float(b["C"]), class_weight_text(b["class_weight"]), float(b["auc_mean"]),
        float(b["auc_std"]))


# A row of COMMANDS, as gkmpanels': the subparser's help, add_argument's arguments in order, the positionals, run(a) -> the
# line for stderr
Command = collections.namedtuple("Command", "help options positionals run")
_GRID = _TRAIN[:7] + (_opt("-C", "--regularization", default="0.01,0.1,1,10", help="comma-separated values of C "
                           "(default: 0.01,0.1,1,10)"),) + _TRAIN[8:] + (
    _opt("--class-weight", default="none", help="comma-separated weightings: none, balanced or W0:W1 (default: none)"),
    _opt("--ncv", type=int, default=5, help="folds (default: 5)"),
    _opt("--repeats", type=int, default=1, help="repeats of the cross-validation (default: 1)"),
    _opt("--seed", type=int, default=1, help="seed of the folds; negative: none (default: 1)"))
COMMANDS = {
    "train": Command("train on pos.fa + neg.fa with class weights and write a model file", _TRAIN + (_CLASS_WEIGHT, _DEVICE),
                     ("pos_fa", "neg_fa", "model"), _run_train),
    "cv-grid": Command("cross-validate every setting of -C x --class-weight on pos.fa + neg.fa from one Gram matrix and one "
                       "solver launch: C<TAB>class_weight<TAB>auc_mean<TAB>auc_std<TAB>capped per setting",
                       _GRID + (_DEVICE,), ("pos_fa", "neg_fa", "output"), _run_cv_grid),
}


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gkmqc_amd.gkmselect", description=__doc__.split("\n\n")[0])
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
        print("gkmselect: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
