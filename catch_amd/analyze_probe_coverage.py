#!/usr/bin/env python3
"""Analyze the coverage of a probe set on the GPU:  python -m catch_amd.analyze_probe_coverage -d a.fasta [b.fasta ...] -f probes.fasta -m M -l L --print-analysis

The reference's bin/analyze_probe_coverage.py (:17-93, options :96-220) with
its option names and defaults: every dataset is a FASTA file, one group of
target genomes named by the file's basename, one Genome per record; the probes
are the records of --probes-fasta (records that repeat a header collapse, as
seq_io.read_fasta returns a dict); both strands of every genome are analysed.

One option the reference does not have: --params PARAMS_TSV (instead of -m and
-e) reads the table of parameter values that pool writes and analyses every
dataset under its own row's (mismatches, cover_extension) -- the check of a
pooled design.  A dataset is named by its file (grid.dataset_name, as in
design_grid); each dataset's rows of the report, of the TSV and of the
sliding-window file are those of that dataset analysed alone under its row,
in -d order; a probe's map count is the sum over the datasets.
"""
import argparse
from collections import Counter
import logging
import os
import sys

from catch_amd import combine_pooled
from catch_amd import coverage_analysis
from catch_amd import grid
from catch_amd import probe
from catch_amd import target_regions
from catch_amd.utils import seq_io

logger = logging.getLogger("catch_amd.analyze_probe_coverage")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-d", "--dataset", nargs="+", required=True,
                   help="one or more target datasets, each a FASTA file")
    p.add_argument("-f", "--probes-fasta", required=True,
                   help="FASTA file of the probes (one per record)")
    p.add_argument("-m", "--mismatches", type=int,
                   help="mismatches allowed when a probe covers a sequence "
                        "(required unless --params is given)")
    p.add_argument("-l", "--lcf-thres", required=True, type=int,
                   help="a probe covers a stretch it shares at least LCF_THRES "
                        "bp with, within MISMATCHES mismatches")
    p.add_argument("--island-of-exact-match", type=int, default=0)
    p.add_argument("-e", "--cover-extension", type=int,
                   help="bp by which a probe's coverage extends on each side "
                        "(default 0)")
    p.add_argument("--params",
                   help="table of parameter values written by pool: every "
                        "dataset is analysed under its own mismatches and "
                        "cover_extension (instead of -m / -e)")
    p.add_argument("--limit-target-genomes", type=int,
                   help="use only the first N target genomes of each dataset")
    p.add_argument("--either-strand", action="store_true",
                   help="the probes capture a locus whichever strand of it was "
                        "deposited (design --either-strand): analyse the "
                        "forward strands only, under the probes followed by "
                        "their reverse complements; a probe's map count is the "
                        "sum over its two orientations")
    p.add_argument("--print-analysis", action="store_true")
    p.add_argument("--write-analysis-to-tsv")
    p.add_argument("--write-sliding-window-coverage")
    p.add_argument("--write-probe-map-counts-to-tsv",
                   help="sequences each probe maps to, not counting reverse "
                        "complements")
    coverage_analysis.add_uncovered_arguments(p)
    target_regions.add_arguments(p)     # --target-regions, --exclude-regions: the uncovered-region outputs list wanted bases only

    def check_max_num_processes(val):
        ival = int(val)
        if ival >= 1:
            return ival
        raise argparse.ArgumentTypeError("MAX_NUM_PROCESSES must be an int >= 1")
    p.add_argument("--max-num-processes", type=check_max_num_processes,
                   help="accepted for compatibility; the scans run on the GPU")
    p.add_argument("--kmer-probe-map-k", type=int, default=10)
    p.add_argument("--debug", dest="log_level", action="store_const",
                   const=logging.DEBUG, default=logging.WARNING)
    p.add_argument("--verbose", dest="log_level", action="store_const",
                   const=logging.INFO)
    args = p.parse_args(argv)
    if args.params is not None:
        if args.mismatches is not None or args.cover_extension is not None:
            p.error("--params gives every dataset its own mismatches and cover "
                    "extension: it cannot be combined with -m / -e")
    else:
        if args.mismatches is None:
            p.error("the following arguments are required: -m/--mismatches "
                    "(or --params)")
        if args.cover_extension is None:
            args.cover_extension = 0
    if target_regions.given(args) and not (args.write_uncovered_regions or args.write_uncovered_fasta):
        p.error("--target-regions / --exclude-regions say which bases the uncovered-region outputs list: they "
                "need --write-uncovered-regions or --write-uncovered-fasta (every other output describes "
                "whole genomes)")
    return args


def read_genomes(datasets, limit_target_genomes=None):
    """(genomes per dataset, their names), bin/analyze_probe_coverage.py:19-43."""
    return read_named_genomes(datasets, limit_target_genomes)[:2]


def read_named_genomes(datasets, limit_target_genomes=None):
    """read_genomes and, third, the FASTA headers of every dataset's genomes (what target regions name)."""
    genomes_grouped, names, records_grouped = [], [], []
    for ds in datasets:
        if ds.startswith("download:"):
            raise ValueError("dataset '%s': downloading a taxonomy ID from NCBI is "
                             "not supported (this package does no network access); "
                             "give the FASTA file instead" % ds)
        if not os.path.isfile(ds):
            raise ValueError("dataset '%s' is not a file: only FASTA files are "
                             "accepted as datasets; please check that the path "
                             "is valid" % ds)
        genomes, records = seq_io.read_named_genomes_from_fasta(ds)
        genomes_grouped.append(genomes)
        records_grouped.append(records)
        names.append(os.path.basename(ds))
    if limit_target_genomes:
        genomes_grouped = [g[:limit_target_genomes] for g in genomes_grouped]
    return genomes_grouped, names, records_grouped


def params_per_dataset(params_tsv, datasets):
    """[(mismatches, cover_extension)] per dataset, from pool's table: every
    dataset needs its row and every row its dataset."""
    rows = {}
    for d, m, e in combine_pooled.read_params(params_tsv):
        if d in rows:
            raise ValueError("%s: dataset %s has two rows" % (params_tsv, d))
        rows[d] = (m, e)
    names = [grid.dataset_name(ds) for ds in datasets]
    if len(set(names)) != len(names):
        raise ValueError("two datasets share a name (%s): the rows of %s cannot "
                         "be told apart" % (", ".join(sorted(
                             n for n in set(names) if names.count(n) > 1)), params_tsv))
    for n in names:
        if n not in rows:
            raise ValueError("%s has no row for dataset %s" % (params_tsv, n))
    extra = sorted(set(rows) - set(names))
    if extra:
        raise ValueError("%s has rows for datasets that were not given with -d: %s"
                         % (params_tsv, ", ".join(extra)))
    return [rows[n] for n in names]


def main(args):
    logging.basicConfig(
        level=args.log_level,
        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    genomes_grouped, names, records_grouped = read_named_genomes(args.dataset)
    # (resolved against every record read; the regions then follow the records that --limit-target-genomes keeps)
    regions = target_regions.from_args(args, records_grouped, genomes_grouped)
    if args.limit_target_genomes:
        genomes_grouped = [g[:args.limit_target_genomes] for g in genomes_grouped]
        if regions is not None:
            regions = regions.select([range(len(g)) for g in genomes_grouped])
    if args.params is not None:
        params = params_per_dataset(args.params, args.dataset)
    else:
        params = [(args.mismatches, args.cover_extension)] * len(genomes_grouped)

    fasta = seq_io.read_fasta(args.probes_fasta)
    probes = [probe.Probe.from_str(seq) for _, seq in fasta.items()]

    # one analyzer per distinct (mismatches, cover_extension), over the
    # datasets that share it; where[d] = (analyzer, its index of dataset d)
    members = {}
    for d, me in enumerate(params):
        members.setdefault(me, []).append(d)
    analyzers, where = [], {}
    for (m, e), ds in members.items():
        a = coverage_analysis.Analyzer(
            probes, m, args.lcf_thres, [genomes_grouped[d] for d in ds],
            [names[d] for d in ds],
            island_of_exact_match=args.island_of_exact_match,
            cover_extension=e, kmer_probe_map_k=args.kmer_probe_map_k,
            target_regions=None if regions is None else regions.select_groups(ds),
            **(dict(rc_too=False, either_strand=True) if args.either_strand else {}))
        a.run()
        analyzers.append(a)
        for local, d in enumerate(ds):
            where[d] = (a, local)
    order = [where[d] for d in range(len(genomes_grouped))]

    if len(analyzers) == 1:
        a = analyzers[0]
        if args.write_analysis_to_tsv:
            a.write_data_matrix_as_tsv(args.write_analysis_to_tsv)
        if args.write_sliding_window_coverage:
            a.write_sliding_window_coverage(args.write_sliding_window_coverage)
        if args.write_probe_map_counts_to_tsv:
            a.write_probe_map_counts(args.write_probe_map_counts_to_tsv)
        if args.print_analysis:
            a.print_analysis()
        coverage_analysis.write_uncovered(a, args)
        return analyzers

    if args.write_analysis_to_tsv:
        with open(args.write_analysis_to_tsv, "w") as f:
            rows = [coverage_analysis.Analyzer._TSV_HEADER]
            for a, local in order:
                rows += a._data_matrix_rows([local])
            for row in rows:
                f.write("\t".join(str(entry) for entry in row) + "\n")
    if args.write_sliding_window_coverage:
        with open(args.write_sliding_window_coverage, "w") as f:
            for a, local in order:
                a._write_sliding_rows(f, [local])
    if args.write_probe_map_counts_to_tsv:
        counts = Counter()
        for a in analyzers:
            counts.update(dict(a.ordered_probe_map_counts()))
        coverage_analysis.write_probe_map_counts(
            counts.items(), args.write_probe_map_counts_to_tsv)
    if args.print_analysis:
        data = [coverage_analysis.Analyzer._TABLE_HEADER]
        for a, local in order:
            data += a._make_data_matrix_string([local])
        print("NUMBER OF PROBES: %d" % len(probes))
        print()
        coverage_analysis.print_table(data)
    _write_uncovered(args, [(a, [local]) for a, local in order])
    return analyzers


def _write_uncovered(args, order):
    """--write-uncovered-regions / --write-uncovered-fasta: every (analyzer,
    its groupings to write; None = all) in turn, one shared file each."""
    if not (args.write_uncovered_regions or args.write_uncovered_fasta):
        return
    filters = coverage_analysis.uncovered_filters(args)
    if args.write_uncovered_regions:
        with open(args.write_uncovered_regions, "w") as f:
            f.write("\t".join(coverage_analysis.Analyzer._UNCOVERED_HEADER) + "\n")
            for a, groups in order:
                a._write_uncovered_rows(f, groups, *filters)
    if args.write_uncovered_fasta:
        with open(args.write_uncovered_fasta, "w") as f:
            for a, groups in order:
                a._write_uncovered_fasta_rows(f, groups, *filters)
    for a in dict.fromkeys(a for a, _groups in order):
        a.log_uncovered_summary("", *filters)


def _cli(argv):
    args = parse_args(argv)
    try:
        main(args)
    except ValueError as exc:
        sys.stderr.write("analyze_probe_coverage: error: %s\n" % exc)
        sys.exit(2)


if __name__ == "__main__":
    _cli(sys.argv[1:])
