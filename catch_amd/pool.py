#!/usr/bin/env python3
"""Pool probes across datasets: python -m catch_amd.pool COUNTS_TSV
TARGET_PROBE_COUNT PARAMS_TSV [--loss-coeffs C ...] [--dataset-weights TSV]

The middle step of the reference README's option #3, between
catch_amd.design_grid (which writes COUNTS_TSV and the probes of every grid
point) and catch_amd.combine_pooled (which reads PARAMS_TSV): one designed
grid point per dataset such that the pooled probe count fits the budget and
the loss  sum_d w_d * sum_j c_j * v_dj^2  is smallest.

The reference's bin/pool.py relaxes the choice to continuous parameters,
interpolates probe counts between grid points, runs a barrier-method optimiser
from a random start and rounds the result to a grid
(catch/pool/param_search.py).  Here the choice is made among the designed
points only -- a multiple-choice knapsack -- and the exact minimum is found by
a dynamic programme over (dataset, budget cell) on the GPU
(catchhip_pool_solve, csrc/pool.hip).  The answer is deterministic, always a
row of the table, and never worse than any on-grid answer within the budget.
"""
import argparse
import logging
import sys

import numpy as np

logger = logging.getLogger("catch_amd.pool")

# the reference's defaults (catch/pool/param_search.py:585-590 for the standard search; 1 for any other parameter,
# as its higher-dimensional search, :694-698)
DEFAULT_LOSS_COEFFS = {"mismatches": 1.0, "cover_extension": 1.0 / 100.0}


def read_probe_counts(fn):
    """The probe-count table (catch/utils/pool_probes_io.py:11-60; what
    catch_amd.design_grid --write-probe-count-table writes): first column
    'dataset', last column 'num_probes', parameter columns between them.
    Returns (param_names, {dataset: {param_values: num_probes}}), the values a
    tuple of floats in the order of param_names."""
    d = {}
    header = None
    with open(fn) as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            ls = line.rstrip("\n").rstrip("\r").split("\t")
            if header is None:
                header = ls
                if header[0] != "dataset":
                    raise ValueError("%s: the first column of a probe count table must be 'dataset'" % fn)
                if header[-1] != "num_probes":
                    raise ValueError("%s: the last column of a probe count table must be 'num_probes'" % fn)
                if len(header) < 3:
                    raise ValueError("%s: a probe count table needs at least one parameter column" % fn)
                if len(set(header)) != len(header):
                    raise ValueError("%s: a column name appears twice in the header" % fn)
                continue
            if len(ls) != len(header):
                raise ValueError("%s, line %d: %d columns, the header has %d" % (fn, lineno, len(ls), len(header)))
            try:
                values = tuple(float(x) for x in ls[1:-1])
                n = int(ls[-1])
            except ValueError:
                raise ValueError("%s, line %d: parameter values must be numbers and num_probes an integer"
                                 % (fn, lineno))
            if n < 0:
                raise ValueError("%s, line %d: negative num_probes" % (fn, lineno))
            if not all(np.isfinite(values)):
                raise ValueError("%s, line %d: a parameter value is not finite" % (fn, lineno))
            if values in d.setdefault(ls[0], {}):
                raise ValueError("%s, line %d: dataset %s is listed more than once with parameters %s"
                                 % (fn, lineno, ls[0], " ".join("%g" % v for v in values)))
            d[ls[0]][values] = n
    if header is None:
        raise ValueError("%s: empty table" % fn)
    return tuple(header[1:-1]), d


def read_dataset_weights(fn, datasets=None):
    """The weights table (catch/utils/pool_probes_io.py:63-115): header
    'dataset', 'weight'.  Returns {dataset: weight}; every name in `datasets`
    (if given) must have one."""
    d = {}
    header = None
    with open(fn) as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            ls = line.rstrip("\n").rstrip("\r").split("\t")
            if header is None:
                header = ls
                if header != ["dataset", "weight"]:
                    raise ValueError("%s: the header of a dataset weights table must be 'dataset', 'weight'" % fn)
                continue
            if len(ls) != 2:
                raise ValueError("%s, line %d: expected a dataset and a weight" % (fn, lineno))
            if ls[0] in d:
                raise ValueError("%s, line %d: dataset %s appears on more than one row" % (fn, lineno, ls[0]))
            try:
                d[ls[0]] = float(ls[1])
            except ValueError:
                raise ValueError("%s, line %d: the weight is not a number" % (fn, lineno))
    if header is None:
        raise ValueError("%s: empty table" % fn)
    for name in sorted(datasets or ()):
        if name not in d:
            raise ValueError("dataset %s needs a weight, but the dataset weights table %s gives none" % (name, fn))
    return d


def default_loss_coeffs(param_names):
    return tuple(DEFAULT_LOSS_COEFFS.get(name, 1.0) for name in param_names)


def options(counts, loss_coeffs, dataset_weights=None):
    """The instance the solver sees: datasets in sorted name order, each one's
    table rows sorted by parameter tuple ascending.  Returns (names, opt_off
    int64[D + 1], params per option, counts int64, losses float64): option k
    of dataset d costs w_d * (c_0 v_0^2 + c_1 v_1^2 + ...), float64, the terms
    added in column order."""
    names = sorted(counts)
    off = np.zeros(len(names) + 1, dtype=np.int64)
    params, cnt, loss = [], [], []
    for i, d in enumerate(names):
        w = 1.0 if dataset_weights is None else float(dataset_weights[d])
        for values in sorted(counts[d]):
            if len(values) != len(loss_coeffs):
                raise ValueError("dataset %s: %d parameter values for %d loss coefficients"
                                 % (d, len(values), len(loss_coeffs)))
            s = 0.0
            for c, v in zip(loss_coeffs, values):
                s = s + float(c) * (float(v) * float(v))       # c_j * v_j^2 with v_j^2 formed first
            params.append(values)
            cnt.append(int(counts[d][values]))
            loss.append(w * s)
        off[i + 1] = len(params)
    return names, off, params, np.asarray(cnt, dtype=np.int64), np.asarray(loss, dtype=np.float64)


def pool(counts, budget, loss_coeffs=None, dataset_weights=None, param_names=None, ctx=None):
    """One table row per dataset, minimum loss, total probes <= budget.

    counts: {dataset: {param_values: num_probes}} as read_probe_counts returns
    it.  loss_coeffs: one per parameter column (default: 1 for mismatches,
    1/100 for cover_extension -- the two columns when param_names is not given
    -- and 1 for any other parameter).  dataset_weights: {dataset: weight},
    default 1 each.  Returns ({dataset: param_values}, total probes, loss).
    Among equally good choices the one whose option indices, last dataset
    first, are lexicographically smallest.  ValueError when even the smallest
    point of every dataset exceeds the budget (the message names the smallest
    feasible budget)."""
    from catch_amd import engine
    widths = {len(v) for d in counts.values() for v in d}
    if len(widths) > 1:
        raise ValueError("the datasets' parameter tuples differ in length")
    width = widths.pop() if widths else 0
    if loss_coeffs is None:
        if param_names is None:
            param_names = ("mismatches", "cover_extension")
            if width not in (0, 2):
                raise ValueError("%d parameters per row: give param_names or loss_coeffs" % width)
        loss_coeffs = default_loss_coeffs(param_names)
    loss_coeffs = tuple(float(c) for c in loss_coeffs)
    if width and len(loss_coeffs) != width:
        raise ValueError("the number of loss coefficients (%d) must be the number of parameters in the table (%d)"
                         % (len(loss_coeffs), width))
    if dataset_weights is not None:
        for d in sorted(counts):
            if d not in dataset_weights:
                raise ValueError("dataset %s needs a weight, but none is given" % d)
    for d in sorted(counts):
        if not counts[d]:
            raise ValueError("dataset %s has no rows" % d)
    names, off, params, cnt, loss = options(counts, loss_coeffs, dataset_weights)
    if ctx is None:
        ctx = engine.default_context()
    choice, total, best = engine.pool_solve(ctx, off, cnt, loss, int(budget))
    chosen = {d: params[int(off[i]) + int(choice[i])] for i, d in enumerate(names)}
    for d in names:
        logger.info("%s: (%s)", d, ", ".join("%g" % v for v in chosen[d]))
    return chosen, total, best


def write_params(param_names, params_by_dataset, out_tsv):
    """The parameter table combine_pooled.read_params and the reference's
    readers take (catch/utils/pool_probes_io.py:118-148, type='int'): header
    'dataset' + the parameter names, one row per dataset in sorted order,
    values as %d.  Grid values are integers; a fractional one is an error
    rather than a silently truncated number."""
    lines = ["\t".join(["dataset"] + list(param_names))]
    for d in sorted(params_by_dataset):
        vals = params_by_dataset[d]
        if len(vals) != len(param_names):
            raise ValueError("dataset %s: %d values for %d parameters" % (d, len(vals), len(param_names)))
        for name, v in zip(param_names, vals):
            if v != int(v):
                raise ValueError("dataset %s: %s = %r is not an integer" % (d, name, v))
        lines.append("\t".join([d] + ["%d" % int(v) for v in vals]))
    with open(out_tsv, "w") as f:
        f.write("\n".join(lines) + "\n")


def _parser():
    p = argparse.ArgumentParser(prog="catch_amd.pool", description=__doc__.split("\n")[0].split(":")[0] + ".")
    p.add_argument("probe_count_tsv",
                   help="table of probe counts per dataset and grid point (first column 'dataset', last column "
                        "'num_probes', parameter columns between them)")
    p.add_argument("target_probe_count", type=int,
                   help="the budget: the chosen points' probe counts add up to at most this")
    p.add_argument("param_vals_tsv", help="output table of the chosen parameter values per dataset")
    p.add_argument("--loss-coeffs", nargs="+", type=float,
                   help="coefficients of the parameters in the loss, in the order of the table's parameter columns "
                        "(default: 1 for mismatches, 1/100 for cover_extension, 1 for any other parameter)")
    p.add_argument("--dataset-weights", dest="dataset_weights_tsv",
                   help="table with a weight per dataset (header 'dataset', 'weight'; default: 1 each)")
    p.add_argument("--verbose", action="store_true", help="log the chosen point of every dataset")
    # the reference's two switches for its continuous search: accepted so that the message can say why not
    p.add_argument("--round-params", nargs=2, type=int, help=argparse.SUPPRESS)
    p.add_argument("--use-nd", action="store_true", help=argparse.SUPPRESS)
    return p


def main(argv=None):
    """The command line; returns ({dataset: param_values}, total probes, loss)."""
    p = _parser()
    args = p.parse_args(argv)
    if args.round_params is not None:
        p.error("--round-params is not needed: the answer is always a designed grid point of the table, never a "
                "value between grid points")
    if args.use_nd:
        p.error("--use-nd is not needed: the answer is always a designed grid point, so a table with any number of "
                "parameter columns takes the same exact search")
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARNING,
                        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    try:
        param_names, counts = read_probe_counts(args.probe_count_tsv)
        if args.loss_coeffs and len(args.loss_coeffs) != len(param_names):
            raise ValueError("with --loss-coeffs, the number of coefficients (%d) must be the number of parameters "
                             "in the table (%d)" % (len(args.loss_coeffs), len(param_names)))
        weights = None
        if args.dataset_weights_tsv:
            weights = read_dataset_weights(args.dataset_weights_tsv, counts.keys())
        chosen, total, loss = pool(counts, args.target_probe_count, loss_coeffs=args.loss_coeffs,
                                   dataset_weights=weights, param_names=param_names)
        write_params(param_names, chosen, args.param_vals_tsv)
    except (ValueError, OSError) as exc:
        p.error(str(exc))
    print("Number of probes: %d" % total)
    print("Loss: %f" % loss)
    return chosen, total, loss


if __name__ == "__main__":
    main(sys.argv[1:])
