#!/usr/bin/env python3
"""Drop the probes of an existing set that cover nothing alone:  python -m catch_amd.prune_probes -d a.fasta [b.fasta ...] -f probes.fasta -o kept.fasta

For a probe set that no greedy produced -- a pooled design, two panels merged,
a vendor's list: which probes can one stop ordering without uncovering a base?
The reference has no such command.  Every record of --probes-fasta is one
probe (of any length; records that repeat a sequence stay separate probes),
every record of the datasets one target genome.  The probes are scanned once
against all the genomes under the set cover filter's definition of coverage
(-m, -l, -e, --island-of-exact-match); then they are examined from the last
record to the first, and one is dropped when every base it covers is covered
by more than --coverage-depth of the probes still there
(SetCoverFilter.prune_probe_strs); with --either-strand a probe covers what its
sequence or its reverse complement hybridises to.  Every base the set covered D times stays
covered D times; the kept records are written in file order, and the two
counts (kept, dropped) are printed.
"""
import argparse
import logging
import sys

from catch_amd import probe
from catch_amd.analyze_probe_coverage import read_genomes
from catch_amd.filter import set_cover_filter
from catch_amd.utils import seq_io

logger = logging.getLogger("catch_amd.prune_probes")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-d", "--dataset", nargs="+", required=True,
                   help="one or more target datasets, each a FASTA file")
    p.add_argument("-f", "--probes-fasta", required=True,
                   help="FASTA file of the probes (one per record)")
    p.add_argument("-o", "--write-probe-fasta", required=True,
                   help="output FASTA: the probes kept, in file order")
    p.add_argument("--write-removed", metavar="FASTA",
                   help="output FASTA: the probes dropped, in the order they "
                        "were dropped")
    p.add_argument("-m", "--mismatches", type=int, default=0)
    p.add_argument("-l", "--lcf-thres", type=int,
                   help="a probe covers a stretch it shares at least LCF_THRES "
                        "bp with, within MISMATCHES mismatches (default: the "
                        "length of the first probe)")
    p.add_argument("--island-of-exact-match", type=int, default=0)
    p.add_argument("-e", "--cover-extension", type=int, default=0)
    p.add_argument("--kmer-probe-map-k", type=int, default=20)
    p.add_argument("--coverage-depth", type=int, default=1, metavar="D",
                   help="keep every base covered by D probes that is covered "
                        "by D now (and every base covered by fewer as it is)")
    p.add_argument("--either-strand", action="store_true",
                   help="a probe covers a base when its sequence or its reverse "
                        "complement hybridises there (double-stranded "
                        "libraries): a record is redundant when the others "
                        "cover its bases in either orientation")
    p.add_argument("--verbose", action="store_true")
    return p.parse_args(argv)


def main(args):
    logging.basicConfig(
        level=logging.INFO if args.verbose else logging.WARNING,
        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    if args.coverage_depth < 1:
        raise ValueError("--coverage-depth must be at least 1, not %d" % args.coverage_depth)
    genomes_grouped, _names = read_genomes(args.dataset)
    strs = list(seq_io.iterate_fasta(args.probes_fasta))
    if len(strs) == 0:
        raise ValueError("--probes-fasta: %s holds no sequence" % args.probes_fasta)
    scf = set_cover_filter.SetCoverFilter(
        mismatches=args.mismatches,
        lcf_thres=args.lcf_thres if args.lcf_thres is not None else len(strs[0]),
        island_of_exact_match=args.island_of_exact_match,
        cover_extension=args.cover_extension,
        kmer_probe_map_k=args.kmer_probe_map_k,
        coverage_depth=args.coverage_depth, either_strand=args.either_strand)
    kept, removed = scf.prune_probe_strs(strs, [g for genomes in genomes_grouped for g in genomes])
    logger.info("%d probes, %d redundant; %s", len(strs), len(removed), scf.last_timings)
    seq_io.write_probe_fasta([probe.Probe.from_str(strs[i]) for i in kept], args.write_probe_fasta)
    if args.write_removed:
        seq_io.write_probe_fasta([probe.Probe.from_str(strs[i]) for i in removed], args.write_removed)
    print(len(kept), len(removed))
    return kept, removed


def _cli(argv):
    args = parse_args(argv)
    try:
        main(args)
    except ValueError as exc:
        sys.stderr.write("prune_probes: error: %s\n" % exc)
        sys.exit(2)


if __name__ == "__main__":
    _cli(sys.argv[1:])
