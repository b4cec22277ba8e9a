"""Design probes in naive ways: the baseline a design is compared against.

    python -m catch_amd.design_naively DATASET.fasta [-pl 100] [-ps 50]
        [-nrf MISMATCHES LCF_THRES | -dsf MISMATCHES LCF_THRES]
        [--add-reverse-complements] [--limit-target-genomes N]
        [--limit-target-genomes-randomly-with-replacement N]
        [--print-analysis] [-o PROBES.fasta]

Mirrors bin/design_naively.py of the reference: candidate probes of every
genome, DuplicateFilter, then optionally the naive redundant filter (-nrf) or
the dominating set filter (-dsf) under the longest-common-substring predicate,
then optionally the reverse complements.  Prints the number of probes, or with
--print-analysis the coverage analysis at -nrf / -dsf's mismatches (0 without
either) and lcf_thres = the probe length.

Two differences.  The redundancy predicate is always the exact one -- the
reference's randomised k-mer heuristic in front of it is not reproduced
(catch_amd/filter/naive_redundant_filter.py says why) -- and it is evaluated for
all pairs on the GPU.  And -o/--write-probe-fasta writes the probes, which the
reference's command never does.
"""
import argparse
import logging
import os
import random
import sys

from catch_amd.filter import dominating_set_filter, duplicate_filter
from catch_amd.filter import naive_redundant_filter, probe_designer
from catch_amd.filter import reverse_complement_filter
from catch_amd.utils import seq_io

VERSION = "catch_amd design_naively (after bin/design_naively.py of catch 1.5.2)"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("dataset", help="Path to fasta file")
    p.add_argument("-o", "--write-probe-fasta", help="write the probes to this FASTA file")
    p.add_argument("-pl", "--probe-length", type=int, default=100,
                   help="(Optional) The number of bp in each probe")
    p.add_argument("-ps", "--probe-stride", type=int, default=50,
                   help="(Optional) Generate candidate probes from the input that are separated by this "
                        "number of bp")
    p.add_argument("-nrf", "--naive-redundant-filter", nargs=2, type=int,
                   help="Args: <MISMATCHES> <LCF_THRES>. Walk the probes in order and, for each probe p that is "
                        "kept, drop the later probes redundant to p: those whose longest common substring "
                        "with p, up to MISMATCHES mismatches, is >= LCF_THRES.")
    p.add_argument("-dsf", "--dominating-set-filter", nargs=2, type=int,
                   help="Args: <MISMATCHES> <LCF_THRES>. Connect redundant probes (same rule as -nrf) and "
                        "approximate the smallest dominating set of that graph.")
    p.add_argument("--add-reverse-complements", dest="add_reverse_complements", action="store_true",
                   help="Add to the output the reverse complement of each probe")
    p.add_argument("--limit-target-genomes", type=int,
                   help="(Optional) Use only the first N target genomes in the dataset")
    p.add_argument("--limit-target-genomes-randomly-with-replacement", type=int,
                   help="(Optional) Randomly select N target genomes in the dataset with replacement")
    p.add_argument("--print-analysis", dest="print_analysis", action="store_true",
                   help="Print analysis of the probe set's coverage")
    from catch_amd import coverage_analysis
    coverage_analysis.add_uncovered_arguments(p)
    p.add_argument("--debug", dest="log_level", action="store_const", const=logging.DEBUG,
                   default=logging.WARNING, help="Debug output")
    p.add_argument("--verbose", dest="log_level", action="store_const", const=logging.INFO,
                   help="Verbose output")
    p.add_argument("-V", "--version", action="version", version=VERSION)
    return p.parse_args(argv)


def main(args):
    logging.basicConfig(level=args.log_level,
                        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    ds = args.dataset
    if not os.path.isfile(ds):
        raise ValueError("Datasets labels are no longer allowed as input. Please specify a FASTA file or, "
                         "if you already did, check that the file path is correct.")
    seqs = [seq_io.read_genomes_from_fasta(ds)]

    if args.limit_target_genomes and args.limit_target_genomes_randomly_with_replacement:
        raise Exception("Cannot --limit-target-genomes and --limit-target-genomes-randomly-with-replacement "
                        "at the same time")
    elif args.limit_target_genomes:
        seqs = [genomes[:args.limit_target_genomes] for genomes in seqs]
    elif args.limit_target_genomes_randomly_with_replacement:
        k = args.limit_target_genomes_randomly_with_replacement
        seqs = [random.choices(genomes, k=k) for genomes in seqs]

    # DuplicateFilter first: not needed for the result, but it shrinks the all-pairs step
    filters = [duplicate_filter.DuplicateFilter()]
    mismatches = 0
    if args.naive_redundant_filter and args.dominating_set_filter:
        raise Exception("Cannot use both 'naive_redundant_filter' and 'dominating_set_filter' at the same "
                        "time. (You could of course do one after the other, but it was probably a mistake "
                        "to specify both.)")
    elif args.naive_redundant_filter or args.dominating_set_filter:
        if args.naive_redundant_filter:
            mismatches, lcf_thres = args.naive_redundant_filter
            filt_class = naive_redundant_filter.NaiveRedundantFilter
        else:
            mismatches, lcf_thres = args.dominating_set_filter
            filt_class = dominating_set_filter.DominatingSetFilter
        redundant_fn = naive_redundant_filter.redundant_longest_common_substring(mismatches, lcf_thres)
        filters.append(filt_class(redundant_fn))
    if args.add_reverse_complements:
        filters.append(reverse_complement_filter.ReverseComplementFilter())

    pb = probe_designer.ProbeDesigner(seqs, filters, probe_length=args.probe_length,
                                      probe_stride=args.probe_stride)
    pb.design()
    if getattr(args, "write_probe_fasta", None):
        seq_io.write_probe_fasta(pb.final_probes, args.write_probe_fasta)
    if args.print_analysis or args.write_uncovered_regions or args.write_uncovered_fasta:
        from catch_amd import coverage_analysis
        analyzer = coverage_analysis.Analyzer(pb.final_probes, mismatches, args.probe_length, seqs,
                                              [args.dataset])
        analyzer.run()
        if args.print_analysis:
            analyzer.print_analysis()
        coverage_analysis.write_uncovered(analyzer, args)
    else:
        print(len(pb.final_probes))
    return pb


if __name__ == "__main__":
    main(parse_args(sys.argv[1:]))
