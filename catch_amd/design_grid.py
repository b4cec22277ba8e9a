#!/usr/bin/env python3
"""Design probes over a grid of mismatches x cover extensions, per dataset:
python -m catch_amd.design_grid a.fasta [b.fasta ...] --grid-mismatches 0 1 2
--grid-cover-extension 0 10 20 -o OUTDIR [--write-probe-count-table T.tsv]

The first step of the reference README's option #3: design.py run once per
dataset and grid point, the probe counts written as the table pool.py reads
(catch/utils/pool_probes_io.py:11-60).  Every FASTA file is one dataset, named
after its basename without .fasta / .fa / .fna (and .gz); point (d, m, e) goes
to OUTDIR/<d>.m<m>.e<e>.fasta and holds exactly what `python -m
catch_amd.design d.fasta -m m -e e` writes with the same other options.  Each
dataset is read and filtered once, scanned once per m, and the cover
extensions are derived from that scan on the GPU (catch_amd.grid).
"""
import argparse
import logging
import os
import sys

from catch_amd import grid
from catch_amd.filter import background_filter, composition_filter, quality, structure_filter, tm_filter
from catch_amd.utils import seq_io

logger = logging.getLogger("catch_amd.design_grid")

# catch_amd.design options that a pooled design does not take: they couple the
# datasets (identification, avoided genomes, clustering), need a second probe
# model (the tolerant options), belong after pooling (adapters, analyses, N
# expansion, reverse complements), or are not part of a grid (a FASTA filter,
# no set cover, limited input)
_REFUSED = (
    ("identify", "-i/--identify"),
    ("avoid_genomes", "--avoid-genomes"),
    ("mismatches_tolerant", "-mt/--mismatches-tolerant"),
    ("lcf_thres_tolerant", "-lt/--lcf-thres-tolerant"),
    ("island_of_exact_match_tolerant", "--island-of-exact-match-tolerant"),
    ("cluster_and_design_separately", "--cluster-and-design-separately"),
    ("cluster_and_design_separately_method", "--cluster-and-design-separately-method"),
    ("cluster_from_fragments", "--cluster-from-fragments"),
    ("add_adapters", "--add-adapters"),
    ("adapter_a", "--adapter-a"),
    ("adapter_b", "--adapter-b"),
    ("print_analysis", "--print-analysis"),
    ("write_analysis_to_tsv", "--write-analysis-to-tsv"),
    ("write_sliding_window_coverage", "--write-sliding-window-coverage"),
    ("write_probe_map_counts_to_tsv", "--write-probe-map-counts-to-tsv"),
    ("expand_n", "--expand-n"),
    ("add_reverse_complements", "--add-reverse-complements"),
    ("filter_from_fasta", "--filter-from-fasta"),
    ("skip_set_cover", "--skip-set-cover"),
    ("limit_target_genomes", "--limit-target-genomes"),
    ("limit_target_genomes_randomly_with_replacement",
     "--limit-target-genomes-randomly-with-replacement"),
)


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description=__doc__.split("\n")[0],
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset", nargs="+", help="FASTA file(s); one dataset each")
    p.add_argument("--grid-mismatches", type=int, nargs="+", required=True,
                   help="values of -m/--mismatches")
    p.add_argument("--grid-cover-extension", type=int, nargs="+", required=True,
                   help="values of -e/--cover-extension")
    p.add_argument("-o", "--output-dir", required=True,
                   help="directory for <dataset>.m<M>.e<E>.fasta")
    p.add_argument("--write-probe-count-table",
                   help="TSV of probe counts for pool.py (default: stdout)")
    p.add_argument("-pl", "--probe-length", type=int, default=100)
    p.add_argument("-ps", "--probe-stride", type=int, default=50)
    p.add_argument("-l", "--lcf-thres", type=int, default=None,
                   help="default: the probe length")
    p.add_argument("--island-of-exact-match", type=int, default=0)
    p.add_argument("-c", "--coverage", type=float, default=1.0,
                   help="fraction (<= 1) or number of bp (> 1) per genome")
    p.add_argument("--filter-with-lsh-hamming", type=int,
                   help="Hamming threshold of the near-duplicate filter")
    p.add_argument("--filter-with-lsh-minhash", type=float,
                   help="Jaccard-distance threshold of the MinHash "
                        "near-duplicate filter")
    p.add_argument("--filter-polya", nargs=2, type=int,
                   help="<X> <Y>: drop candidate probes with a stretch of X or "
                        "more 'A' bases, tolerating up to Y mismatches (likewise 'T')")
    composition_filter.add_arguments(p)     # as catch_amd.design's
    structure_filter.add_arguments(p)       # likewise
    tm_filter.add_arguments(p)              # likewise
    background_filter.add_arguments(p)      # likewise
    quality.add_arguments(p)                # likewise (--write-candidate-profile)
    p.add_argument("--small-seq-skip", type=int)
    p.add_argument("--small-seq-min", type=int)
    p.add_argument("--kmer-probe-map-k", type=int)
    p.add_argument("--verbose", action="store_true")
    # refused (see _REFUSED): accepted by the parser so that the message can say why
    S = argparse.SUPPRESS
    p.add_argument("-i", "--identify", action="store_true", help=S)
    p.add_argument("--avoid-genomes", nargs="+", help=S)
    p.add_argument("-mt", "--mismatches-tolerant", type=int, help=S)
    p.add_argument("-lt", "--lcf-thres-tolerant", type=int, help=S)
    p.add_argument("--island-of-exact-match-tolerant", type=int, help=S)
    p.add_argument("--cluster-and-design-separately", help=S)
    p.add_argument("--cluster-and-design-separately-method", help=S)
    p.add_argument("--cluster-from-fragments", help=S)
    p.add_argument("--add-adapters", action="store_true", help=S)
    p.add_argument("--adapter-a", nargs=2, help=S)
    p.add_argument("--adapter-b", nargs=2, help=S)
    p.add_argument("--print-analysis", action="store_true", help=S)
    p.add_argument("--write-analysis-to-tsv", help=S)
    p.add_argument("--write-sliding-window-coverage", help=S)
    p.add_argument("--write-probe-map-counts-to-tsv", help=S)
    p.add_argument("--expand-n", nargs="?", type=int, default=None, const=3, help=S)
    p.add_argument("--add-reverse-complements", action="store_true", help=S)
    p.add_argument("--filter-from-fasta", help=S)
    p.add_argument("--skip-set-cover", action="store_true", help=S)
    p.add_argument("--limit-target-genomes", type=int, help=S)
    p.add_argument("--limit-target-genomes-randomly-with-replacement", type=int, help=S)
    # the grid values are given with --grid-*: the single-value options are refused
    p.add_argument("-m", "--mismatches", type=int, help=S)
    p.add_argument("-e", "--cover-extension", type=int, help=S)
    args = p.parse_args(argv)
    check_args(args, p.error)
    composition_filter.from_args(args, p.error)     # (bad values are argparse errors; main builds the filter)
    structure_filter.from_args(args, p.error)
    tm_filter.from_args(args, p.error)
    background_filter.from_args(args, p.error, load=False)      # (the options alone: main reads the background)
    return args


def check_args(args, error):
    """Refuses what a grid does not take; checks names and grid values."""
    for attr, flag in _REFUSED:
        value = getattr(args, attr, None)
        if value or (attr == "expand_n" and value is not None):     # (--expand-n 0 is given, too)
            error("%s is not supported by a grid design: a pooled design designs "
                  "each dataset on its own, and this option either couples the "
                  "datasets or belongs after pooling" % flag)
    if args.mismatches is not None or args.cover_extension is not None:
        error("give the grid values with --grid-mismatches and "
              "--grid-cover-extension (-m/-e are single values)")
    try:
        grid.check_grid_values("--grid-mismatches", args.grid_mismatches)
        grid.check_grid_values("--grid-cover-extension", args.grid_cover_extension)
    except ValueError as exc:
        error(str(exc))
    names = [grid.dataset_name(fn) for fn in args.dataset]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        error("datasets with the same name: %s (names are the FASTA basenames "
              "without .fasta/.fa/.fna and .gz)" % ", ".join(dup))
    args.names = names


def output_path(outdir, name, m, e):
    return os.path.join(outdir, "%s.m%d.e%d.fasta" % (name, m, e))


def main(args):
    logging.basicConfig(
        level=logging.INFO if args.verbose else logging.WARNING,
        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    from catch_amd import probe
    datasets = [seq_io.read_genomes_from_fasta(fn) for fn in args.dataset]
    composition = composition_filter.from_args(args)
    structure = structure_filter.from_args(args)
    tm = tm_filter.from_args(args)
    background = background_filter.from_args(args)
    profile = quality.from_args(args)
    got = grid.design_grid(
        datasets, args.grid_mismatches, args.grid_cover_extension,
        probe_length=args.probe_length, probe_stride=args.probe_stride,
        lcf_thres=args.lcf_thres, island_of_exact_match=args.island_of_exact_match,
        coverage=args.coverage, filter_with_lsh_hamming=args.filter_with_lsh_hamming,
        filter_with_lsh_minhash=args.filter_with_lsh_minhash,
        small_seq_skip=args.small_seq_skip, small_seq_min=args.small_seq_min,
        kmer_probe_map_k=args.kmer_probe_map_k, filter_polya=args.filter_polya,
        filter_composition=composition, filter_structure=structure,
        filter_tm=tm, filter_background=background, candidate_profile=profile)
    if profile is not None:
        quality.finish(profile, args, logger)
    if composition is not None:
        logger.info("composition filter: %d candidates dropped (GC %d, homopolymer %d, low complexity %d)",
                    composition.dropped[3], *composition.dropped[:3])
    if structure is not None:
        logger.info("structure filter: %d candidates dropped (hairpin %d, self-dimer %d)",
                    structure.dropped[2], *structure.dropped[:2])
    if tm is not None:
        logger.info("tm filter: %d candidates dropped (below %d, above %d)", tm.dropped[2], *tm.dropped[:2])
        if args.write_tm_histogram:
            tm.write_histogram(args.write_tm_histogram)
    if background is not None:
        if logger.isEnabledFor(logging.INFO):       # (counting the k-mers can mean building an index)
            logger.info(background.summary())
        if args.write_background_histogram:
            background.write_histogram(args.write_background_histogram)
        background.close()
    os.makedirs(args.output_dir, exist_ok=True)
    counts = []
    for di, name in enumerate(args.names):
        for m in args.grid_mismatches:
            for e in args.grid_cover_extension:
                strs = list(dict.fromkeys(got[(di, m, e)]))
                seq_io.write_probe_fasta([probe.Probe.from_str(s) for s in strs],
                                         output_path(args.output_dir, name, m, e))
                counts.append((name, m, e, len(strs)))
    grid.write_probe_count_table(counts, args.write_probe_count_table or sys.stdout)
    return counts


if __name__ == "__main__":
    main(parse_args(sys.argv[1:]))
