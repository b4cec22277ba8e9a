#!/usr/bin/env python3
"""Design probes on the GPU:  python -m catch_amd.design a.fasta [b.fasta ...] -o probes.fasta

The hot-path subset of the reference CLI (bin/design.py:448-980), same option
names and defaults ("basic" profile): every FASTA file is one dataset = one
group of target genomes (bin/design.py:91-99), one Genome per record.  Filter
list as bin/design.py:296-340 builds it: exact duplicate filter (or a
near-duplicate filter with --filter-with-lsh-hamming / --filter-with-lsh-
minhash), then the set cover filter; --cluster-and-design-separately clusters
the input sequences first and designs per cluster (:387-411).  The optional
filters stand where bin/design.py:255-385 puts them: --filter-from-fasta and
--filter-polya before the duplicate filter, --add-adapters, --expand-n and
--add-reverse-complements after the set cover, which --skip-set-cover leaves
out; --limit-target-genomes[-randomly-with-replacement] cut the input down
right after it is read (:101-112).  Custom hybridization functions and
download: labels are not offered.  --extend-probes (no counterpart in the
reference) keeps an existing probe set and designs only the probes that bring
the targets up to the required coverage next to it; --coverage-depth D (no
counterpart either) designs a set in which D probes cover every base, one
greedy layer per unit of depth; --prune-redundant (nor this) drops the selected
probes that cover nothing alone; --max-probes N (nor this) keeps, over all
datasets, the N set cover picks that added the most coverage when they were
taken, and --write-coverage-curve writes how coverage grows with the number
of probes; --filter-gc, --max-homopolymer and --filter-low-complexity (nor
these) drop candidates by their composition, one filter right after the
poly(A) filter (catch_amd/filter/composition_filter.py has the rules);
--max-hairpin-stem (with --hairpin-min-loop) and --max-self-dimer (nor these)
drop candidates that fold on themselves or bind a second copy, one filter
right after that one (catch_amd/filter/structure_filter.py has the rules);
--filter-tm (with --tm-sodium, --tm-oligo, --tm-formamide; nor these) drops
candidates by their nearest-neighbour melting temperature and
--write-tm-histogram writes its distribution, one filter right after that one
(catch_amd/filter/tm_filter.py has the rule); --background (with
--background-kmer, --background-mismatches, --background-max-hits; nor these) drops candidates that
share k-mers with a host genome or another background and
--write-background-histogram writes how many share how many, one filter right
after that one (catch_amd/filter/background_filter.py has the rule);
--write-candidate-profile (nor this) measures the candidates instead of
judging them, one QualityProfile right after the poly(A) filter that drops
nothing (catch_amd/filter/quality.py has the quantities), and
--write-probe-report (nor this) writes what the designed probes are like, the
report of catch_amd.probe_report for the output FASTA.
--target-regions / --exclude-regions (nor these) say which bases are to be
covered at all: BED intervals per FASTA record, the cover rows cut to them
after the scan (catch_amd/target_regions.py has the rules).
--either-strand (nor this) lets a candidate cover what its reverse complement
hybridises to as well: targets filed in mixed orientations get one probe set.
--max-cross-dimer (nor this) drops picked probes that anneal to an earlier
kept one, one CrossDimerFilter right after the set cover filter over the picks
of all datasets (catch_amd/filter/cross_dimer.py has the rule); --cross-dimer
adds its two columns to --write-probe-report.
--cross-dimer-redesign (nor this; with --max-cross-dimer) designs around the
conflicts instead: the set cover filter never offers a candidate that anneals
to a kept or an existing probe and covers again what a dropped pick would have
covered, in at most --cross-dimer-rounds solves per dataset.
--max-cross-dimer-dg G (nor this) is --max-cross-dimer with another unit: a
pair conflicts when its firmest stretch has a nearest-neighbour dG below -G
kcal/mol (catch_amd/filter/cross_duplex.py has the rule); one of the two per
design, the same filter, the same redesign; --cross-dimer-dg adds its two
columns to --write-probe-report.
--print-analysis and the
three --write-... options run the coverage analysis of the designed probes
(bin/design.py:417-442).
"""
import argparse
import logging
import os
import random
import sys

from catch_amd.filter import background_filter, composition_filter
from catch_amd.filter import duplicate_filter, near_duplicate_filter
from catch_amd.filter import probe_designer, quality, set_cover_filter
from catch_amd.filter import cross_dimer, cross_duplex, structure_filter, tm_filter
from catch_amd.utils import seq_io

logger = logging.getLogger("catch_amd.design")


# defaults that differ between design.py ("basic") and design_large.py ("large"),
# bin/design.py:502, :583, :753, :794, :846
_PROFILES = {
    "basic": dict(mismatches=0, cover_extension=0, cluster=None,
                  fragments=None, minhash=None),
    "large": dict(mismatches=5, cover_extension=50, cluster=0.15,
                  fragments=50000, minhash=0.6),
}


def parse_args(argv=None, args_type="basic"):
    if args_type not in _PROFILES:
        raise ValueError("Argument type '%s' is invalid; it must be one of %s"
                         % (args_type, tuple(_PROFILES)))
    prof = _PROFILES[args_type]
    p = argparse.ArgumentParser(
        description=__doc__.split("\n")[0],
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset", nargs="+", help="FASTA file(s); one group each")
    p.add_argument("-o", "--write-probe-fasta", help="output FASTA")
    p.add_argument("-pl", "--probe-length", type=int, default=100)
    p.add_argument("-ps", "--probe-stride", type=int, default=50)
    p.add_argument("-m", "--mismatches", type=int,
                   default=prof["mismatches"])
    p.add_argument("-l", "--lcf-thres", type=int, default=None,
                   help="default: the probe length")
    p.add_argument("--island-of-exact-match", type=int, default=0)
    p.add_argument("-c", "--coverage", type=float, default=1.0,
                   help="fraction (<= 1) or number of bp (> 1) per genome")
    p.add_argument("-e", "--cover-extension", type=int,
                   default=prof["cover_extension"])
    p.add_argument("-i", "--identify", action="store_true")
    p.add_argument("--avoid-genomes", nargs="+", default=[])
    p.add_argument("-mt", "--mismatches-tolerant", type=int)
    p.add_argument("-lt", "--lcf-thres-tolerant", type=int)
    p.add_argument("--island-of-exact-match-tolerant", type=int, default=0)
    p.add_argument("--filter-with-lsh-hamming", type=int,
                   help="Hamming threshold of the near-duplicate filter")
    p.add_argument("--filter-with-lsh-minhash", type=float,
                   default=prof["minhash"],
                   help="Jaccard-distance threshold of the MinHash "
                        "near-duplicate filter")
    p.add_argument("--small-seq-skip", type=int)
    p.add_argument("--small-seq-min", type=int)
    p.add_argument("--kmer-probe-map-k", type=int)
    p.add_argument("--print-analysis", action="store_true",
                   help="print coverage of the target genomes by the probes")
    p.add_argument("--write-analysis-to-tsv")
    p.add_argument("--write-sliding-window-coverage")
    p.add_argument("--write-probe-map-counts-to-tsv")
    from catch_amd import coverage_analysis
    coverage_analysis.add_uncovered_arguments(p)
    from catch_amd import target_regions
    target_regions.add_arguments(p)         # --target-regions, --exclude-regions (not in the reference)
    def dissimilarity(val):
        fval = float(val)
        if fval == 0:
            return None      # no clustering: the way to switch design_large.py's default off (--extend-probes needs it)
        if 0 < fval <= 0.5:
            return fval
        raise argparse.ArgumentTypeError(
            "%s is an invalid average nucleotide dissimilarity" % val)
    p.add_argument("--cluster-and-design-separately", type=dissimilarity,
                   default=prof["cluster"],
                   help="cluster all input sequences by MinHash signature "
                        "(threshold in 1-ANI, (0, 0.5]), design per cluster "
                        "and merge; 0: do not cluster")
    p.add_argument("--cluster-and-design-separately-method",
                   choices=["choose", "simple", "hierarchical"],
                   default="choose")
    p.add_argument("--cluster-from-fragments", type=int,
                   default=prof["fragments"],
                   help="cluster fragments of this length instead of whole "
                        "sequences")
    # bin/design.py:660-742
    p.add_argument("--filter-from-fasta",
                   help="keep only the candidate probes that are a sequence of "
                        "this FASTA file (records whose header contains "
                        "'reverse complement' do not count), in the file's order")
    p.add_argument("--skip-set-cover", dest="skip_set_cover", action="store_true",
                   help="leave the set cover filter out")
    p.add_argument("--filter-polya", nargs=2, type=int,
                   help="<X> <Y>: drop candidate probes with a stretch of X or "
                        "more 'A' bases, tolerating up to Y mismatches (likewise 'T')")
    composition_filter.add_arguments(p)     # --filter-gc, --max-homopolymer, --filter-low-complexity (not in the reference)
    structure_filter.add_arguments(p)       # --max-hairpin-stem, --hairpin-min-loop, --max-self-dimer (not in the reference)
    tm_filter.add_arguments(p)              # --filter-tm, --tm-..., --write-tm-histogram (not in the reference)
    background_filter.add_arguments(p)      # --background, --background-..., --write-background-histogram (not in the reference)
    quality.add_arguments(p)                # --write-candidate-profile (not in the reference)
    cross_dimer.add_arguments(p)            # --cross-dimer, --max-cross-dimer (not in the reference)
    cross_duplex.add_arguments(p)           # --cross-dimer-dg, --max-cross-dimer-dg (not in the reference)
    p.add_argument("--cross-dimer-redesign", action="store_true",
                   help="with --max-cross-dimer X (or --max-cross-dimer-dg "
                        "G, with `firmer than G` for `over more than X "
                        "bases`): instead of dropping "
                        "conflicting probes behind the set cover, design "
                        "around them.  Candidates that anneal to a probe "
                        "already kept (of any dataset, or of --extend-probes) "
                        "over more than X bases are never offered to the set "
                        "cover; its picks are walked in pick order, a pick that "
                        "conflicts with an earlier one is dropped for good, and "
                        "the set cover runs again on what the kept picks leave "
                        "uncovered, until no pick is dropped.  The output is "
                        "free of conflicts and covers what the remaining "
                        "candidates can cover "
                        "(catch_amd/filter/set_cover_filter.py: _cross_rounds)")
    p.add_argument("--cross-dimer-rounds", type=int, metavar="R",
                   help="with --cross-dimer-redesign: at most R set cover "
                        "solves per dataset (default 8); picks the last one "
                        "drops stay dropped, with a warning")
    p.add_argument("--write-probe-report", metavar="FILE",
                   help="write what the designed probes are like to FILE: the "
                        "report python -m catch_amd.probe_report -f writes "
                        "for the output FASTA with the same parameters and "
                        "thresholds, byte for byte -- the records written to "
                        "-o, in their order, adapters and N expansion "
                        "included (design without adapters to judge the "
                        "target part alone)")
    p.add_argument("--add-reverse-complements", dest="add_reverse_complements",
                   action="store_true",
                   help="add the reverse complement of each probe to the output")
    p.add_argument("--expand-n", nargs="?", type=int, default=None, const=3,
                   help="replace 'N' bases by real bases, combinatorially; with "
                        "INT, expand at most INT randomly chosen N per probe and "
                        "replace the others by random bases")
    p.add_argument("--limit-target-genomes", type=int,
                   help="use only the first LIMIT_TARGET_GENOMES genomes of "
                        "every dataset")
    p.add_argument("--limit-target-genomes-randomly-with-replacement", type=int,
                   help="draw this many genomes of every dataset, with replacement")
    p.add_argument("--extend-probes", metavar="FASTA",
                   help="probes that exist already (adapter-free sequences, "
                        "every record one probe): design only the additional "
                        "probes that bring the targets up to the required "
                        "coverage beside them; the output holds the new "
                        "probes, an analysis covers the existing and the new "
                        "ones together")
    p.add_argument("--coverage-depth", type=int, default=1, metavar="D",
                   help="design a probe set in which D selected probes cover "
                        "every base that D candidates can cover (default 1: "
                        "the ordinary set cover): D greedy layers, each over "
                        "what the layers before it leave below its depth; the "
                        "output lists the probes layer by layer, and its "
                        "first k layers are the design at depth k")
    p.add_argument("--prune-redundant", action="store_true",
                   help="look back at the selected probes once the set cover "
                        "is complete, from the last pick to the first, and "
                        "drop each one whose bases are all covered often "
                        "enough without it (more than --coverage-depth times "
                        "with it); the bases covered stay the same, the output "
                        "holds the probes kept; with --extend-probes the "
                        "existing probes count and stay; with --coverage-depth "
                        "above 1 the first k layers are no longer the design "
                        "at depth k")
    p.add_argument("--either-strand", action="store_true",
                   help="design for double-stranded libraries: a candidate "
                        "covers a base when its own sequence OR its reverse "
                        "complement hybridises there (both under -m, -l, "
                        "--island-of-exact-match and -e), so that targets "
                        "deposited in mixed orientations are not covered "
                        "twice, once per strand; the output holds the picked "
                        "candidates as they are (--add-reverse-complements "
                        "still adds the other orientation); an analysis then "
                        "describes the targets under either orientation of "
                        "the probes")
    p.add_argument("--max-probes", type=int, default=None, metavar="N",
                   help="a probe budget: after the set cover, keep only N of "
                        "its picks over all datasets -- the picks are merged "
                        "by the number of bases each covered first when it was "
                        "taken (ties to the earlier dataset), so every dataset "
                        "keeps the first picks of its own order; with -c 1.0 "
                        "and neither --identify nor --avoid-genomes this is "
                        "the greedy choice of N probes for maximum coverage "
                        "over all datasets together, otherwise a prefix rule; "
                        "N counts set cover picks, a probe picked for several "
                        "datasets once (--expand-n and "
                        "--add-reverse-complements change the final count)")
    p.add_argument("--write-coverage-curve", metavar="FILE",
                   help="write a TSV of the coverage reached by the first k "
                        "picks of every dataset (columns dataset, probes, "
                        "bases_covered, bases_coverable, fraction, "
                        "worst_genome, worst_genome_fraction); with several "
                        "datasets a block '*' follows for the picks merged by "
                        "gain, totals only; the probes column counts set cover "
                        "PICKS in every block -- in '*' a probe picked for two "
                        "datasets is two picks, so row k there can stand for "
                        "fewer than k probes written, and --max-probes N may "
                        "cut at a row beyond N")
    p.add_argument("--coverage-curve-points", type=int, default=100, metavar="P",
                   help="about how many pick counts per dataset the coverage "
                        "curve is measured at (the last pick always is)")
    p.add_argument("--add-adapters", action="store_true",
                   help="add PCR adapters to both ends of every probe")
    p.add_argument("--adapter-a", nargs=2,
                   help="<5' end> <3' end> of the A adapter")
    p.add_argument("--adapter-b", nargs=2,
                   help="<5' end> <3' end> of the B adapter")
    p.add_argument("--verbose", action="store_true")
    args = p.parse_args(argv)
    args.args_type = args_type
    composition_filter.from_args(args, p.error)     # (bad values are argparse errors; main builds the filter)
    structure_filter.from_args(args, p.error)
    tm_filter.from_args(args, p.error)
    background_filter.from_args(args, p.error, load=False)      # (the options alone: main reads the background)
    cross_dimer.check_args(args, p.error)
    cross_duplex.check_args(args, p.error)
    if args.cross_dimer and args.write_probe_report is None:
        p.error("--cross-dimer adds columns to --write-probe-report and needs it (--max-cross-dimer X filters)")
    if args.cross_dimer_dg and args.write_probe_report is None:
        p.error("--cross-dimer-dg adds columns to --write-probe-report and needs it (--max-cross-dimer-dg G filters)")
    if args.max_cross_dimer is not None and args.max_cross_dimer_dg is not None:
        p.error("--max-cross-dimer and --max-cross-dimer-dg are two conflict rules: a design applies one")
    for given, opt in ((args.max_cross_dimer, "--max-cross-dimer"), (args.max_cross_dimer_dg, "--max-cross-dimer-dg")):
        if given is not None:
            if args.add_reverse_complements:
                p.error("%s cannot go with --add-reverse-complements: every probe then has a perfect "
                        "partner by construction" % opt)
            if args.skip_set_cover:
                p.error("%s cannot go with --skip-set-cover: it would pair all candidates with each "
                        "other, a quadratic pass" % opt)
    if args.cross_dimer_redesign and args.max_cross_dimer is None and args.max_cross_dimer_dg is None:
        p.error("--cross-dimer-redesign needs --max-cross-dimer X (or --max-cross-dimer-dg G): the threshold of a conflict")
    if args.cross_dimer_rounds is not None:
        if not args.cross_dimer_redesign:
            p.error("--cross-dimer-rounds needs --cross-dimer-redesign")
        if args.cross_dimer_rounds < 1:
            p.error("--cross-dimer-rounds must be at least 1, not %d" % args.cross_dimer_rounds)
    if args.cross_dimer_redesign:
        for given, opt in ((args.coverage_depth > 1, "--coverage-depth above 1"),
                           (args.prune_redundant, "--prune-redundant"),
                           (args.max_probes is not None, "--max-probes"),
                           (bool(args.write_coverage_curve), "--write-coverage-curve")):
            if given:
                p.error("--cross-dimer-redesign cannot go with %s: the repair rounds are one greedy cover each, "
                        "without a second look at the picks" % opt)
        if args.cross_dimer_rounds is None:
            args.cross_dimer_rounds = 8
    return args


def write_coverage_curve(path, names, scf):
    """--write-coverage-curve: per dataset the rows of scf.last_coverage_curve
    (measured on the device at the dataset's checkpoints); with several
    datasets a block '*' for the picks of all datasets merged by gain
    (set_cover_filter.allocate_budget's order), totals only: the cumulative sum
    of the merged gains on top of what was covered before the first pick.
    The `probes` column counts PICKS in every block.  In '*' a probe picked
    for two datasets counts twice, while the designer writes it once and
    --max-probes counts it once: the cut of a budget N is the row
    sum(scf.last_budget_kept) of '*', which can lie beyond N."""
    def frac(a, b):
        return "%.6f" % (a / b) if b else "NA"
    with open(path, "w") as f:
        f.write("\t".join(("dataset", "probes", "bases_covered", "bases_coverable", "fraction",
                           "worst_genome", "worst_genome_fraction")) + "\n")
        for name, curve in zip(names, scf.last_coverage_curve):
            for k, cov, coverable, wu, wc, wd in curve:
                f.write("%s\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
                    name, k, cov, coverable, frac(cov, coverable),
                    "NA" if wu < 0 else str(wu), "NA" if wu < 0 else frac(wc, wd)))
        if len(names) > 1:
            gains = [[int(x) for x in g] for g in scf.last_pick_gains]
            total = sum(len(g) for g in gains)
            coverable = before = 0
            for g, curve in zip(gains, scf.last_coverage_curve):
                if curve:
                    coverable += curve[-1][2]
                    before += curve[-1][1] - sum(g[:curve[-1][0]])
            cov, taken = before, [0] * len(gains)
            for k in range(1, total + 1):
                # the next pick of the merge: the largest next gain, the earlier dataset among equals
                gi = max((i for i in range(len(gains)) if taken[i] < len(gains[i])),
                         key=lambda i: (gains[i][taken[i]], -i))
                cov += gains[gi][taken[gi]]
                taken[gi] += 1
                f.write("*\t%d\t%d\t%d\t%s\tNA\tNA\n" % (k, cov, coverable, frac(cov, coverable)))


def limit_target_genomes(args, genomes_grouped, regions=None):
    """--limit-target-genomes / --limit-target-genomes-randomly-with-replacement
    (bin/design.py:101-112: before anything else draws from `random`) ->
    (genomes_grouped, regions): the target regions (or None) follow the records
    kept.  The draws from `random` are those of the reference's
    random.choices(genomes, k=k) per dataset: it draws the same numbers for a
    population of the same size, whatever it holds."""
    if (args.limit_target_genomes and
            args.limit_target_genomes_randomly_with_replacement):
        raise Exception(("Cannot --limit-target-genomes and "
                         "--limit-target-genomes-randomly-with-replacement at "
                         "the same time"))
    kept = None
    if args.limit_target_genomes:
        kept = [list(range(len(genomes)))[:args.limit_target_genomes]
                for genomes in genomes_grouped]
    elif args.limit_target_genomes_randomly_with_replacement:
        k = args.limit_target_genomes_randomly_with_replacement
        kept = [random.choices(range(len(genomes)), k=k)
                for genomes in genomes_grouped]
    if kept is not None:
        genomes_grouped = [[genomes[i] for i in idx] for genomes, idx in zip(genomes_grouped, kept)]
        if regions is not None:
            regions = regions.select(kept)
    return genomes_grouped, regions


def main(args):
    logging.basicConfig(
        level=logging.INFO if args.verbose else logging.WARNING,
        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    if getattr(args, "args_type", "basic") == "large":   # bin/design.py:52-57
        logger.warning("With design_large.py, the default values for some "
                       "arguments --- such as mismatches (-m) or cover "
                       "extension (-e) --- might be more relaxed than "
                       "desired. Run 'design_large.py --help' to see the "
                       "default values; they can be overridden by specifying "
                       "the argument.")
    lcf_thres = args.lcf_thres if args.lcf_thres is not None else args.probe_length
    if args.coverage > 1:
        args.coverage = int(args.coverage)
    # bin/design.py:236-244
    if args.cluster_and_design_separately and args.identify:
        raise Exception(("Cannot use --cluster-and-design-separately with "
                         "--identify, because clustering collapses genome "
                         "groupings into one"))
    existing_probes = []
    if args.extend_probes:
        if args.skip_set_cover:
            raise Exception(("Cannot use --extend-probes with --skip-set-cover: "
                             "the set cover is what decides which probes the "
                             "existing ones leave to be designed"))
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use --extend-probes with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the existing probes are set "
                             "against each dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)"))
        if args.cluster_from_fragments:
            raise Exception(("Cannot use --extend-probes with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well"))
        existing_probes = list(seq_io.iterate_fasta(args.extend_probes))
        if len(existing_probes) == 0:
            raise Exception("--extend-probes: %s holds no sequence"
                            % args.extend_probes)
    if args.coverage_depth < 1:
        raise Exception("--coverage-depth must be at least 1, not %d"
                        % args.coverage_depth)
    if args.coverage_depth > 1:
        if args.extend_probes:
            raise Exception(("Cannot use --coverage-depth above 1 with "
                             "--extend-probes: the depth that existing probes "
                             "reach already is not taken into account"))
        if args.skip_set_cover:
            raise Exception(("Cannot use --coverage-depth above 1 with "
                             "--skip-set-cover: the depth is what the set "
                             "cover's layers design for"))
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use --coverage-depth above 1 with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the layers are designed "
                             "against each dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)"))
        if args.cluster_from_fragments:
            raise Exception(("Cannot use --coverage-depth above 1 with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well"))
    if args.prune_redundant:
        if args.skip_set_cover:
            raise Exception(("Cannot use --prune-redundant with "
                             "--skip-set-cover: it is the set cover's picks "
                             "that are looked at again"))
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use --prune-redundant with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the picks are set against each "
                             "dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)"))
        if args.cluster_from_fragments:
            raise Exception(("Cannot use --prune-redundant with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well"))
    if args.either_strand:
        if args.skip_set_cover:
            raise Exception(("Cannot use --either-strand with "
                             "--skip-set-cover: it is the set cover's sets "
                             "that take in the other strand"))
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use --either-strand with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the two strands are set against "
                             "each dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)"))
        if args.cluster_from_fragments:
            raise Exception(("Cannot use --either-strand with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well"))
    if args.cross_dimer_redesign:
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use --cross-dimer-redesign with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the repair rounds run on each "
                             "dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)"))
        if args.cluster_from_fragments:
            raise Exception(("Cannot use --cross-dimer-redesign with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well"))
    from catch_amd import target_regions
    if target_regions.given(args):
        opt = "--target-regions" if args.target_regions else "--exclude-regions"
        if args.skip_set_cover:
            raise Exception(("Cannot use %s with --skip-set-cover: it is the "
                             "set cover that designs for the wanted bases") % opt)
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use %s with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the regions are set against "
                             "each dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)") % opt)
        if args.cluster_from_fragments:
            raise Exception(("Cannot use %s with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well") % opt)
    want_gains = args.max_probes is not None or bool(args.write_coverage_curve)
    if args.coverage_curve_points < 1:
        raise Exception("--coverage-curve-points must be at least 1, not %d"
                        % args.coverage_curve_points)
    if args.max_probes is not None and args.max_probes < 1:
        raise Exception("--max-probes must be at least 1, not %d" % args.max_probes)
    if want_gains:
        opt = "--max-probes" if args.max_probes is not None else "--write-coverage-curve"
        if args.skip_set_cover:
            raise Exception(("Cannot use %s with --skip-set-cover: it is the "
                             "set cover's picks whose gains are measured") % opt)
        if args.cluster_and_design_separately:
            raise Exception(("Cannot use %s with "
                             "--cluster-and-design-separately (a default of "
                             "design_large.py): the gains are measured against "
                             "each dataset as a whole; set "
                             "--cluster-and-design-separately to 0 (and, where "
                             "it is set, --cluster-from-fragments to 0 too)") % opt)
        if args.cluster_from_fragments:
            raise Exception(("Cannot use %s with "
                             "--cluster-from-fragments (a default of "
                             "design_large.py): nothing is clustered; set "
                             "--cluster-from-fragments to 0 as well") % opt)
        if args.coverage_depth > 1:
            raise Exception(("Cannot use %s with --coverage-depth above 1: "
                             "what a pick adds is then no longer the bases it "
                             "covers first") % opt)
    if args.cluster_from_fragments and not args.cluster_and_design_separately:
        raise Exception(("Cannot use --cluster-from-fragments without also "
                         "setting --cluster-and-design-separately"))
    if args.add_adapters:
        if not (args.adapter_a or args.adapter_b):
            logger.warning("Adapter sequences will be added, but default "
                           "sequences will be used; to provide adapter "
                           "sequences, use --adapter-a and --adapter-b")
    elif args.adapter_a or args.adapter_b:
        raise Exception(("Adapter sequences were provided with --adapter-a "
                         "and --adapter-b, but --add-adapters is required to "
                         "add adapter sequences onto the ends of probes"))
    named = [seq_io.read_named_genomes_from_fasta(fn) for fn in args.dataset]
    genomes_grouped = [genomes for genomes, _names in named]
    # the wanted bases, resolved against every record read: the regions then follow the records the limits keep
    regions = target_regions.from_args(args, [names for _genomes, names in named], genomes_grouped)
    genomes_grouped, regions = limit_target_genomes(args, genomes_grouped, regions)

    # bin/design.py:180-205, :232: argument checks and the k-mer length each
    # consumer of the probe map uses (20 / 20 / 10 unless given)
    if args.small_seq_skip is not None and args.small_seq_min is not None:
        raise Exception("Both --small-seq-skip and --small-seq-min were given: "
                        "one skips short sequences, the other designs on them")
    if args.kmer_probe_map_k:
        if args.kmer_probe_map_k > args.probe_length:
            raise Exception("--kmer-probe-map-k (%d) exceeds the probe length (%d)"
                            % (args.kmer_probe_map_k, args.probe_length))
        k_scf = k_af = k_analyzer = args.kmer_probe_map_k
    else:
        if args.probe_length <= 20:
            logger.warning("The probe length (%d) is small: consider a "
                           "--kmer-probe-map-k below it", args.probe_length)
        k_scf, k_af, k_analyzer = 20, 20, 10
    filters = []
    if args.filter_from_fasta:      # bin/design.py:261-264
        from catch_amd.filter import fasta_filter
        filters.append(fasta_filter.FastaFilter(args.filter_from_fasta,
                                                skip_reverse_complements=True))
    if args.filter_polya:           # bin/design.py:268-284
        from catch_amd.filter import polya_filter
        polya_length, polya_mismatches = args.filter_polya
        if polya_length > args.probe_length:
            logger.warning(("Length of poly(A) stretch to filter (%d) is "
                            "greater than PROBE_LENGTH (%d), which is usually "
                            "undesirable"), polya_length, args.probe_length)
        if polya_length < 10:
            logger.warning(("Length of poly(A) stretch to filter (%d) is "
                            "short, and may lead to many probes being "
                            "filtered"), polya_length)
        if polya_mismatches > 10:
            logger.warning(("Number of mismatches to tolerate when searching "
                            "for poly(A) stretches (%d) is high, and may "
                            "lead to many probes being filtered"),
                           polya_mismatches)
        filters.append(polya_filter.PolyAFilter(polya_length, polya_mismatches))
    profile = quality.from_args(args)
    if profile is not None:         # --write-candidate-profile: looks at what the filters below are about to judge
        filters.append(profile)
    composition = composition_filter.from_args(args)
    if composition is not None:     # one filter for the three rules: a function of the candidate alone, like poly(A)
        filters.append(composition)
    structure = structure_filter.from_args(args)
    if structure is not None:       # one filter for both rules, likewise a function of the candidate alone
        filters.append(structure)
    tm = tm_filter.from_args(args)
    if tm is not None:              # melting temperature: a filter, a measurement (--write-tm-histogram), or both
        filters.append(tm)
    background = background_filter.from_args(args)
    if background is not None:      # k-mers shared with a background: a filter, a measurement, or both, likewise
        filters.append(background)
    if (args.filter_with_lsh_hamming is not None and
            args.filter_with_lsh_minhash is not None):
        raise Exception("Cannot use both --filter-with-lsh-hamming "
                        "and --filter-with-lsh-minhash")
    if args.filter_with_lsh_hamming is not None:
        if args.filter_with_lsh_hamming > args.mismatches:
            logger.warning("Nearly duplicate probes are filtered by calling "
                           "near-duplicates probes within a Hamming distance "
                           "that exceeds --mismatches")
        filters.append(near_duplicate_filter.NearDuplicateFilterWithHammingDistance(
            args.filter_with_lsh_hamming, args.probe_length))
    elif args.filter_with_lsh_minhash is not None:
        if args.mismatches < 3:
            logger.warning("MISMATCHES is set to %d; at low values using "
                           "--filter-with-lsh-minhash may cause the probes to "
                           "achieve less than the desired coverage",
                           args.mismatches)
        filters.append(near_duplicate_filter.NearDuplicateFilterWithMinHash(
            args.filter_with_lsh_minhash))
    else:
        filters.append(duplicate_filter.DuplicateFilter())
    scf = set_cover_filter.SetCoverFilter(
        mismatches=args.mismatches, lcf_thres=lcf_thres,
        island_of_exact_match=args.island_of_exact_match,
        mismatches_tolerant=args.mismatches_tolerant,
        lcf_thres_tolerant=args.lcf_thres_tolerant,
        island_of_exact_match_tolerant=args.island_of_exact_match_tolerant,
        identify=args.identify, avoided_genomes=args.avoid_genomes,
        coverage=args.coverage, cover_extension=args.cover_extension,
        kmer_probe_map_k=k_scf, fixed_probes=existing_probes,
        coverage_depth=args.coverage_depth,
        prune_redundant=args.prune_redundant,
        max_probes=args.max_probes, pick_gains=want_gains,
        curve_points=args.coverage_curve_points,
        target_regions=regions, either_strand=args.either_strand,
        **(dict(max_cross_dimer=args.max_cross_dimer, max_cross_dimer_dg=args.max_cross_dimer_dg,
                cross_dimer_rounds=args.cross_dimer_rounds)
           if args.cross_dimer_redesign else {}))
    filters.append(scf)
    cross = None
    # (not in the reference) one filter over the picks of all datasets; under --cross-dimer-redesign the set cover
    # filter keeps its picks free of conflicts itself
    if (args.max_cross_dimer is not None or args.max_cross_dimer_dg is not None) and not args.cross_dimer_redesign:
        cross = cross_dimer.CrossDimerFilter(args.max_cross_dimer, max_cross_dimer_dg=args.max_cross_dimer_dg)
        filters.append(cross)
    if args.add_adapters:      # bin/design.py:345-365 (default sequences :350, :354)
        from catch_amd.filter import adapter_filter
        filters.append(adapter_filter.AdapterFilter(
            tuple(args.adapter_a) if args.adapter_a else
            ("ATACGCCATGCTGGGTCTCC", "CGTACTTGGGAGTCGGCCAT"),
            tuple(args.adapter_b) if args.adapter_b else
            ("AGGCCCTGGCTGCTGATATG", "GACCTTTTGGGACAGCGGTG"),
            mismatches=args.mismatches, lcf_thres=lcf_thres,
            island_of_exact_match=args.island_of_exact_match,
            kmer_probe_map_k=k_af))
    if args.expand_n is not None:           # bin/design.py:370-373
        from catch_amd.filter import n_expansion_filter
        filters.append(n_expansion_filter.NExpansionFilter(
            limit_n_expansion_randomly=args.expand_n))
    if args.add_reverse_complements:        # bin/design.py:378-380
        from catch_amd.filter import reverse_complement_filter
        filters.append(reverse_complement_filter.ReverseComplementFilter())
    merge_after = scf
    if args.skip_set_cover:                 # bin/design.py:383-393
        merge_after = filters[filters.index(scf) - 1]
        filters.remove(scf)

    pb = probe_designer.ProbeDesigner(
        genomes_grouped, filters, probe_length=args.probe_length,
        probe_stride=args.probe_stride, allow_small_seqs=args.small_seq_min,
        seq_length_to_skip=args.small_seq_skip,
        cluster_threshold=args.cluster_and_design_separately,
        cluster_merge_after=(merge_after if args.cluster_and_design_separately
                             else None),
        cluster_method=(args.cluster_and_design_separately_method
                        if args.cluster_and_design_separately else None),
        cluster_fragment_length=(args.cluster_from_fragments
                                 if args.cluster_and_design_separately
                                 else None))
    pb.design()
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
    if cross is not None:
        logger.info("cross-dimer filter: %d of %d probes dropped (largest %s %d before, %d after)",
                    cross.dropped, cross.seen, cross.rule.noun, cross.largest_before, cross.largest_after)
    if args.cross_dimer_redesign:
        for gi, fn in enumerate(args.dataset):
            logger.info("%s: cross-dimer redesign: %d rounds, %d candidates banned, %d picks dropped, %d probes kept",
                        os.path.basename(fn), scf.last_cross_rounds[gi], scf.last_cross_banned[gi],
                        scf.last_cross_dropped[gi], scf.last_cross_kept[gi])
    if regions is not None:
        for gi, fn in enumerate(args.dataset):
            coverable = scf.last_coverable_bases[gi] if gi < len(scf.last_coverable_bases) else 0
            logger.info("%s: target regions: %d intervals, %d wanted bases of %d in %d of %d sequences; %d coverable",
                        *((os.path.basename(fn),) + regions.summary(gi, genomes_grouped[gi]) + (coverable,)))
    if args.coverage_depth > 1:
        for fn, sizes in zip(args.dataset, scf.last_layer_sizes):
            logger.info("%s: %s probes in the layers of depth 1 to %d",
                        os.path.basename(fn), " / ".join(str(x) for x in sizes),
                        len(sizes))
    if args.prune_redundant:
        for fn, sizes, gone in zip(args.dataset, scf.last_layer_sizes, scf.last_pruned):
            logger.info("%s: %d picked, %d redundant", os.path.basename(fn), sum(sizes), len(gone))
    if want_gains:
        names = [os.path.basename(fn) for fn in args.dataset]
        for name, gains, kept, curve in zip(names, scf.last_pick_gains, scf.last_budget_kept,
                                            scf.last_coverage_curve):
            at = [row for row in curve if row[0] == kept]
            if at:
                _k, cov, coverable, wu, wc, wd = at[0]
                logger.info("%s: kept %d of %d picks, %d of %d coverable bases, worst genome %d at %.6f",
                            name, kept, len(gains), cov, coverable, wu, wc / wd if wd else 1.0)
            else:
                logger.info("%s: kept %d of %d picks", name, kept, len(gains))
        if args.max_probes is not None:
            logger.info("--max-probes %d: %d set cover picks kept, %d probes in the output",
                        args.max_probes, sum(scf.last_budget_kept), len(pb.final_probes))
        if args.write_coverage_curve:
            write_coverage_curve(args.write_coverage_curve, names, scf)
    if args.write_probe_fasta:
        seq_io.write_probe_fasta(pb.final_probes, args.write_probe_fasta)
    if args.write_probe_report:
        # the records of the output FASTA as probe_report would read them back, judged with this run's options
        from catch_amd import probe_report
        judge = probe_report.Judge(args)
        try:
            probe_report.write_report(judge, probe_report.records_of_probes(pb.final_probes), args.write_probe_report)
        finally:
            judge.close()
    if (args.print_analysis or args.write_analysis_to_tsv or
            args.write_sliding_window_coverage or
            args.write_probe_map_counts_to_tsv or
            args.write_uncovered_regions or args.write_uncovered_fasta):
        # bin/design.py:417-442; the reverse strands are analysed when reverse-
        # complement probes were added (rc_too follows --add-reverse-complements)
        from catch_amd import coverage_analysis
        analyzed = pb.final_probes
        if existing_probes:      # what the user will order against: the probes they own, then the new ones
            from catch_amd import probe
            analyzed = [probe.Probe.from_str(s) for s in existing_probes] + list(analyzed)
        analyzer = coverage_analysis.Analyzer(
            analyzed, args.mismatches, lcf_thres, genomes_grouped,
            target_genomes_names=[os.path.basename(fn) for fn in args.dataset],
            island_of_exact_match=args.island_of_exact_match,
            cover_extension=args.cover_extension,
            kmer_probe_map_k=k_analyzer,
            rc_too=args.add_reverse_complements,
            target_regions=regions,
            # (with both orientations in the output the usual two-strand analysis is the report)
            either_strand=args.either_strand and not args.add_reverse_complements)
        analyzer.run()
        if args.write_analysis_to_tsv:
            analyzer.write_data_matrix_as_tsv(args.write_analysis_to_tsv)
        if args.write_sliding_window_coverage:
            analyzer.write_sliding_window_coverage(
                args.write_sliding_window_coverage)
        if args.write_probe_map_counts_to_tsv:
            analyzer.write_probe_map_counts(args.write_probe_map_counts_to_tsv)
        if args.print_analysis:
            analyzer.print_analysis()
        coverage_analysis.write_uncovered(analyzer, args)
    else:
        # bin/design.py:443-445: only without an analysis (with --extend-probes: the number of NEW probes)
        print(len(pb.final_probes))
    return pb


if __name__ == "__main__":
    main(parse_args(sys.argv[1:]))
