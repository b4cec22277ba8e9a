#!/usr/bin/env python3
"""What the probes of a FASTA file are like:  python -m catch_amd.probe_report -f probes.fasta [-o report.tsv]

One row per record, in file order: probe (the record's name), length, gc,
homopolymer, dust, stem, dimer (catch_amd/filter/quality.py has the
definitions), tm_c (TmFilter._tm_c, hundredths of a degree Celsius) and
background_hits (BackgroundFilter._hits; with --background, within
--background-mismatches) -- NA for what was
not computed or is undefined.  With a threshold option a last column, verdict,
lists the rules the probe fails, or ok; the thresholds are the design
command's and are compared as it compares them.  Not in the reference.
--cross-dimer puts two columns behind background_hits: cross_dimer, the longest
antiparallel pairing with ANOTHER record of the file, and cross_partner, the
number of the first record that reaches it (1-based, in file order; NA when
the value is 0); --max-cross-dimer X implies it and adds the rule cross-dimer
to every record whose value exceeds X, so both members of a pair fail
(catch_amd/filter/cross_dimer.py has the definition).  For these two columns
all records of the file are ONE list, whatever their lengths.
--cross-dimer-against panel.fasta puts two more columns behind them (or where
they would stand): cross_against, the longest antiparallel pairing with a
record of the panel (an equal record included), and cross_against_partner, the
number of the first panel record that reaches it (1-based, NA at 0); with
--max-cross-dimer X a record whose value exceeds X also fails the rule
cross-against (cross_dimer.py: cross_against).
--cross-dimer-dg puts cross_dg and cross_dg_partner behind those columns (or
where they would stand): the stability of the probe's firmest stretch with
another record of the file, in hundredths of a kcal/mol, and the number of the
first record that reaches it (1-based, NA at 0); --max-cross-dimer-dg G implies
it and adds the rule cross-dg to every record whose value exceeds
floor(100 G).  With --cross-dimer-against, cross_dg_against and
cross_dg_against_partner follow, and their rule is cross-dg-against
(catch_amd/filter/cross_duplex.py has the definition).  The length options and
the dG options are independent of each other.

Records are read with seq_io.iterate_fasta: bytes as they are (lower case is
no base), any lengths.  On the device the records are grouped by length: a
group is one engine.Targets of a sequence per record, one engine.Candidates
with probe_length = stride = the length, and one Candidates.measure call.
Records of fewer than 2 characters, records the candidate list leaves out
(those with two N in a row) and everything under CATCHHIP_HOST_FRONT_END=1
take the NumPy path, which gives the same values.
"""
import argparse
import logging
import os
import sys

import numpy as np

from catch_amd.filter import background_filter, composition_filter, cross_dimer, cross_duplex, quality
from catch_amd.filter import structure_filter, tm_filter
from catch_amd.utils import seq_io

logger = logging.getLogger("catch_amd.probe_report")

COLUMNS = ("probe", "length") + quality.QUANTITIES + ("tm_c", "background_hits")
CROSS_COLUMNS = ("cross_dimer", "cross_partner")
RULES = ("gc", "homopolymer", "low-complexity", "hairpin", "self-dimer", "tm", "background")
CROSS_RULE = "cross-dimer"              # the one rule that looks at the other records of the file
AGAINST_COLUMNS = ("cross_against", "cross_against_partner")
AGAINST_RULE = "cross-against"          # ... and the one that looks at another file
DG_COLUMNS = ("cross_dg", "cross_dg_partner")
DG_RULE = "cross-dg"                    # the same two rules by stability (catch_amd/filter/cross_duplex.py)
DG_AGAINST_COLUMNS = ("cross_dg_against", "cross_dg_against_partner")
DG_AGAINST_RULE = "cross-dg-against"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-f", "--probes-fasta", required=True, help="the probes, one record each")
    p.add_argument("-o", "--write-report", metavar="FILE", help="the report as a TSV (default: standard output)")
    composition_filter.add_arguments(p)     # the design command's options: here they judge, and drop nothing
    structure_filter.add_arguments(p)
    tm_filter.add_arguments(p)
    background_filter.add_arguments(p)
    cross_dimer.add_arguments(p)
    cross_duplex.add_arguments(p)
    p.add_argument("--cross-dimer-against", metavar="FASTA",
                   help="two more columns: cross_against, the longest stretch "
                        "over which the probe and a record of this file (a "
                        "panel it will share a tube with) can anneal, and "
                        "cross_against_partner, the number of the first panel "
                        "record that reaches it (1-based, NA when the value is "
                        "0); with --max-cross-dimer X a probe whose value "
                        "exceeds X fails the rule cross-against; with "
                        "--cross-dimer-dg also cross_dg_against and "
                        "cross_dg_against_partner, the same by stability "
                        "(rule cross-dg-against under --max-cross-dimer-dg)")
    p.add_argument("--write-kept", metavar="FASTA", help="the records that fail no rule, as they were read")
    p.add_argument("--write-failed", metavar="FASTA", help="the records that fail a rule")
    p.add_argument("--verbose", action="store_true")
    for action in p._actions:               # the two histograms are the design command's; the report has every value
        if action.dest in ("write_tm_histogram", "write_background_histogram"):
            action.help = argparse.SUPPRESS
    args = p.parse_args(argv)
    for dest, flag in (("write_tm_histogram", "--write-tm-histogram"),
                       ("write_background_histogram", "--write-background-histogram")):
        if getattr(args, dest) is not None:
            p.error("%s is an option of the design commands: the report lists every probe's value" % flag)
    if args.background is None:
        for flag, value in (("--background-kmer", args.background_kmer), ("--background-max-hits", args.background_max_hits),
                            ("--background-mismatches", args.background_mismatches)):
            if value is not None:
                p.error("%s needs --background" % flag)
    cross_dimer.check_args(args, p.error)
    cross_duplex.check_args(args, p.error)
    try:
        Judge(args, load=False)
    except ValueError as exc:
        p.error(str(exc))
    if (args.write_kept or args.write_failed) and not Judge(args, load=False).thresholds:
        p.error("--write-kept and --write-failed need a threshold option")
    return args


class Judge:
    """The parameters and thresholds of a report, validated by the four filter
    classes themselves (a bad value is their ValueError)."""

    def __init__(self, args, load=True):
        self.composition = composition_filter.CompositionFilter(
            gc_range=args.filter_gc, max_homopolymer=args.max_homopolymer, max_dust=args.filter_low_complexity,
            dust_window=args.low_complexity_window)
        self.structure = structure_filter.StructureFilter(
            max_hairpin_stem=args.max_hairpin_stem,
            hairpin_min_loop=3 if args.hairpin_min_loop is None else args.hairpin_min_loop,
            max_self_dimer=args.max_self_dimer)
        self.tm = tm_filter.TmFilter(
            tm_range=args.filter_tm, sodium_mm="50" if args.tm_sodium is None else args.tm_sodium,
            oligo_nm="50" if args.tm_oligo is None else args.tm_oligo,
            formamide_pct="0" if args.tm_formamide is None else args.tm_formamide)
        self.background = None
        if args.background is not None:
            # (load = False only validates the options: a stand-in background with a k-mer of every length)
            seqs = [s for fn in args.background for s in seq_io.read_fasta(fn).values()] if load else ["ACGT" * 8]
            self.background = background_filter.BackgroundFilter(
                seqs, kmer=background_filter.KMER_DEFAULT if args.background_kmer is None else args.background_kmer,
                max_hits=args.background_max_hits, mismatches=getattr(args, "background_mismatches", None) or 0)
        elif args.background_max_hits is not None:
            raise ValueError("--background-max-hits needs --background")
        # (the design commands without the two cross-dimer options hand over a namespace without them)
        self.max_cross_dimer = getattr(args, "max_cross_dimer", None)
        if self.max_cross_dimer is not None:
            self.max_cross_dimer = cross_dimer._threshold(self.max_cross_dimer, "--max-cross-dimer")
        self.cross_dimer = bool(getattr(args, "cross_dimer", False)) or self.max_cross_dimer is not None
        # ... the same by stability: the threshold in hundredths of a kcal/mol
        self.max_cross_dg = getattr(args, "max_cross_dimer_dg", None)
        if self.max_cross_dg is not None:
            self.max_cross_dg = cross_duplex.threshold(self.max_cross_dg, "--max-cross-dimer-dg")
        self.cross_dg = bool(getattr(args, "cross_dimer_dg", False)) or self.max_cross_dg is not None
        # the panel of --cross-dimer-against: its records' sequences (load = False: only that there is one)
        self.against = getattr(args, "cross_dimer_against", None)
        if self.against is not None and load:
            self.against = [s for _name, s in read_records(self.against)]
        self.thresholds = any(x is not None for x in (
            args.filter_gc, args.max_homopolymer, args.filter_low_complexity, args.max_hairpin_stem,
            args.max_self_dimer, args.filter_tm, args.background_max_hits, self.max_cross_dimer, self.max_cross_dg))

    @property
    def min_loop(self):
        return self.structure.hairpin_min_loop

    @property
    def dust_window(self):
        return self.composition.dust_window

    def failed(self, length, five, tm_c, hits, cross=0, against=0, dg=0, dg_against=0):
        """The names of the rules a probe with these values fails, with the ties of the design command."""
        gc, run, dust, stem, dimer = five
        c, s, out = self.composition, self.structure, []
        lo, hi = c._gc_bounds(length)
        if not lo <= gc <= hi:
            out.append(RULES[0])
        if c.max_homopolymer is not None and run > c.max_homopolymer:
            out.append(RULES[1])
        if c.max_dust is not None and dust > c.max_dust:
            out.append(RULES[2])
        if s.max_hairpin_stem is not None and stem > s.max_hairpin_stem:
            out.append(RULES[3])
        if s.max_self_dimer is not None and dimer > s.max_self_dimer:
            out.append(RULES[4])
        if self.tm._side(tm_c) != 0:
            out.append(RULES[5])
        if self.background is not None and self.background.max_hits is not None and hits > self.background.max_hits:
            out.append(RULES[6])
        if self.max_cross_dimer is not None and cross > self.max_cross_dimer:
            out.append(CROSS_RULE)
        if self.max_cross_dimer is not None and self.against is not None and against > self.max_cross_dimer:
            out.append(AGAINST_RULE)
        if self.max_cross_dg is not None and dg > self.max_cross_dg:
            out.append(DG_RULE)
        if self.max_cross_dg is not None and self.against is not None and dg_against > self.max_cross_dg:
            out.append(DG_AGAINST_RULE)
        return out

    def close(self):
        if self.background is not None:
            self.background.close()


def read_records(fn):
    """[(name, sequence)] of a FASTA file: the sequences as seq_io.iterate_fasta
    yields them, the names of the records it yields ('' for sequence lines in
    front of the first header)."""
    names, cur, has = [], "", False
    with seq_io._open(fn) as f:
        for line in f:
            line = line.rstrip()
            if len(line) == 0:
                continue
            if line.startswith(">"):
                if has:
                    names.append(cur)
                cur, has = line[1:], False
            else:
                has = True
    if has:
        names.append(cur)
    seqs = list(seq_io.iterate_fasta(fn))
    assert len(names) == len(seqs)
    return list(zip(names, seqs))


def records_of_probes(probes):
    """[(name, sequence)] as read_records reads them back from the FASTA
    seq_io.write_probe_fasta writes for these Probe objects."""
    return [(seq_io.probe_header(p), p.seq_str.translate(seq_io._DEG_TO_N)) for p in probes if p.seq_str]


def _by_length(seqs):
    groups = {}
    for i, s in enumerate(seqs):
        groups.setdefault(len(s), []).append(i)
    return groups


def _host_values(judge, seqs, five, tm_c, hits, where):
    """The NumPy path for the records `where`."""
    part = [seqs[i] for i in where]
    five[where] = quality.measure_many(part, judge.min_loop, judge.dust_window)
    for L, idx in _by_length(part).items():
        strs, at = [part[i] for i in idx], [where[i] for i in idx]
        if L >= 2:
            for i, t in zip(at, judge.tm._tm_c_equal_length(strs, L).tolist()):
                tm_c[i] = t
        if judge.background is not None and L >= judge.background.kmer:
            hits[at] = judge.background._hits_equal_length(strs, L)


def measure_records(judge, seqs):
    """(five: int64 (n, 5), tm_c: list with None where undefined, hits: int64
    array or None without a background) of the sequences, in their order."""
    n = len(seqs)
    five = np.zeros((n, 5), dtype=np.int64)
    tm_c = [None] * n
    hits = np.zeros(n, dtype=np.int64)
    host = list(range(n))
    if not os.environ.get("CATCHHIP_HOST_FRONT_END") and n:
        from catch_amd import engine
        ctx = engine.default_context()
        index = judge.background._device_index(ctx) if judge.background is not None else None
        host = []
        for L, where in _by_length(seqs).items():
            if L < 2 or L > 65535:
                host += where
                continue
            strs = [seqs[i] for i in where]
            targets = engine.Targets(ctx, [[s] for s in strs])
            try:
                cands = engine.Candidates(ctx, targets, L, L)
                try:
                    what = ("composition", "structure", "tm") + (("hits",) if index is not None else ())
                    got = cands.measure(what=what, min_loop=judge.min_loop, dust_window=judge.dust_window,
                                        tm=(judge.tm._q(L), judge.tm.offset_c), index=index, values=True,
                                        histograms=False)
                    row_of = {strs[p // L]: k for k, p in enumerate(cands.positions().tolist())}
                finally:
                    cands.close()
            finally:
                targets.close()
            cols = np.stack([got[name].astype(np.int64) for name in quality.QUANTITIES], axis=1)
            for i, s in zip(where, strs):
                k = row_of.get(s)
                if k is None:                 # (the candidate list leaves out windows with two N in a row)
                    host.append(i)
                    continue
                five[i] = cols[k]
                tm_c[i] = int(got["tm_c"][k])
                if index is not None:
                    hits[i] = int(got["hits"][k])
        host.sort()
    if host:
        _host_values(judge, seqs, five, tm_c, hits, host)
    return five, tm_c, hits if judge.background is not None else None


def report_lines(judge, records):
    """(the report's lines, header first; per record the list of failed rules,
    empty without thresholds)."""
    seqs = [s for _, s in records]
    five, tm_c, hits = measure_records(judge, seqs)
    cross = partner = None
    if judge.cross_dimer:
        cross, partner = cross_dimer.measure(seqs)
    against = against_partner = None
    if judge.against is not None:
        against, against_partner = cross_dimer.measure_against(seqs, judge.against)
    dg = dg_partner = dg_against = dg_against_partner = None
    if judge.cross_dg:
        dg, dg_partner = cross_duplex.measure(seqs)
        if judge.against is not None:
            dg_against, dg_against_partner = cross_duplex.measure_against(seqs, judge.against)
    lines = ["\t".join(COLUMNS + (CROSS_COLUMNS if judge.cross_dimer else ()) +
                       (AGAINST_COLUMNS if against is not None else ()) + (DG_COLUMNS if dg is not None else ()) +
                       (DG_AGAINST_COLUMNS if dg_against is not None else ()) + (("verdict",) if judge.thresholds else ()))]
    failed = []
    for i, (name, s) in enumerate(records):
        row = [name, str(len(s))] + [str(int(v)) for v in five[i]]
        row.append("NA" if tm_c[i] is None else str(tm_c[i]))
        row.append("NA" if hits is None else str(int(hits[i])))
        if cross is not None:
            row += [str(int(cross[i])), str(int(partner[i]) + 1) if cross[i] > 0 else "NA"]
        if against is not None:
            row += [str(int(against[i])), str(int(against_partner[i]) + 1) if against[i] > 0 else "NA"]
        if dg is not None:
            row += [str(int(dg[i])), str(int(dg_partner[i]) + 1) if dg[i] > 0 else "NA"]
        if dg_against is not None:
            row += [str(int(dg_against[i])), str(int(dg_against_partner[i]) + 1) if dg_against[i] > 0 else "NA"]
        bad = []
        if judge.thresholds:
            bad = judge.failed(len(s), [int(v) for v in five[i]], tm_c[i], 0 if hits is None else int(hits[i]),
                               0 if cross is None else int(cross[i]), 0 if against is None else int(against[i]),
                               0 if dg is None else int(dg[i]), 0 if dg_against is None else int(dg_against[i]))
            row.append(",".join(bad) if bad else "ok")
        failed.append(bad)
        lines.append("\t".join(row))
    return lines, failed


def write_report(judge, records, path):
    """The report of `records` to `path` (None: standard output); returns the failed rules per record."""
    lines, failed = report_lines(judge, records)
    text = "\n".join(lines) + "\n"
    if path is None:
        sys.stdout.write(text)
    else:
        with open(path, "w") as f:
            f.write(text)
    return failed


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">%s\n%s\n" % (name, s))


def main(args):
    logging.basicConfig(
        level=logging.INFO if args.verbose else logging.WARNING,
        format="%(asctime)s - %(name)s [%(levelname)s] %(message)s")
    records = read_records(args.probes_fasta)
    judge = Judge(args)
    try:
        failed = write_report(judge, records, args.write_report)
    finally:
        judge.close()
    passing = sum(1 for bad in failed if not bad)
    summary = "%d records" % len(records) + (", %d pass" % passing if judge.thresholds else "")
    # (the report itself is on standard output without -o: the summary goes beside it, not into it)
    print(summary, file=sys.stdout if args.write_report else sys.stderr)
    if args.write_kept:
        _write_fasta(args.write_kept, [r for r, bad in zip(records, failed) if not bad])
    if args.write_failed:
        _write_fasta(args.write_failed, [r for r, bad in zip(records, failed) if bad])
    return failed


if __name__ == "__main__":
    main(parse_args(sys.argv[1:]))
