#!/usr/bin/env python3
"""Combine the probes of a pooled design: python -m catch_amd.combine_pooled
PARAMS_TSV OUTDIR -o pooled.fasta

PARAMS_TSV is what the reference's pool.py writes (catch/utils/pool_probes_io.py
:118-148: a header 'dataset', 'mismatches', 'cover_extension', then one row per
dataset, values as %d with --round-params, as %f without); OUTDIR holds the
<dataset>.m<M>.e<E>.fasta files of catch_amd.design_grid.  The chosen file of
every dataset is appended to the output in the table's row order.  Probes are
NOT de-duplicated: a probe chosen for two datasets appears twice.
"""
import argparse
import os
import sys

from catch_amd import design_grid


def _integral(text, dataset, column):
    try:
        v = float(text)
    except ValueError:
        v = None
    if v is None or v != int(v):
        raise ValueError("dataset %s: %s = %r is not an integer; run pool.py with "
                         "--round-params to get grid values" % (dataset, column, text))
    return int(v)


def read_params(fn):
    """[(dataset, mismatches, cover_extension)] in the table's row order."""
    out = []
    with open(fn) as f:
        header = None
        for line in f:
            ls = line.rstrip("\n").rstrip("\r").split("\t")
            if not line.strip():
                continue
            if header is None:
                header = ls
                if header[0] != "dataset" or sorted(header[1:]) != ["cover_extension", "mismatches"]:
                    raise ValueError("%s: the header must be 'dataset', 'mismatches', "
                                     "'cover_extension' (got %s)" % (fn, header))
                continue
            if len(ls) != len(header):
                raise ValueError("%s: row %r does not have %d columns" % (fn, line.rstrip(), len(header)))
            row = dict(zip(header, ls))
            d = row["dataset"]
            out.append((d, _integral(row["mismatches"], d, "mismatches"),
                        _integral(row["cover_extension"], d, "cover_extension")))
    if header is None:
        raise ValueError("%s: empty table" % fn)
    return out


def combine(params_tsv, outdir, out_fasta):
    """Concatenates the chosen point's FASTA of every dataset; returns the
    number of probes written."""
    rows = read_params(params_tsv)
    paths = []
    for d, m, e in rows:
        path = design_grid.output_path(outdir, d, m, e)
        if not os.path.exists(path):
            raise FileNotFoundError(
                "dataset %s: no probes for mismatches=%d cover_extension=%d (%s); "
                "were these values on the grid? (pool.py without --round-params "
                "can choose values between grid points)" % (d, m, e, path))
        paths.append(path)
    n = 0
    with open(out_fasta, "w") as out:
        for path in paths:
            with open(path) as f:
                text = f.read()
            if text and not text.endswith("\n"):
                text += "\n"
            n += sum(1 for line in text.splitlines() if line.startswith(">"))
            out.write(text)
    return n


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0] + ".",
                                epilog="Probes are not de-duplicated across datasets.")
    p.add_argument("params_tsv", help="pool.py's output table of parameter values")
    p.add_argument("outdir", help="the output directory of catch_amd.design_grid")
    p.add_argument("-o", "--output", required=True, help="combined FASTA")
    args = p.parse_args(argv)
    try:
        n = combine(args.params_tsv, args.outdir, args.output)
    except (ValueError, FileNotFoundError) as exc:
        p.exit(2, "%s: error: %s\n" % (p.prog, exc))
    print(n)
    return n


if __name__ == "__main__":
    main(sys.argv[1:])
