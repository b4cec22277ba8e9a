"""Target regions: the bases a design has to cover (--target-regions / --exclude-regions).

Not in the reference, which designs for every base of its genomes.  BED files name,
per FASTA record, the bases that are WANTED: the union of the --target-regions
intervals (every base without that option) minus the union of the
--exclude-regions intervals.  Candidates, filters and the scan stay what they are;
after the scan every cover row is cut to its runs of wanted bases
(SetCoverFilter(target_regions=...), engine.Rows.restrict), and the uncovered-region
outputs list runs of wanted bases only (coverage_analysis.Analyzer(target_regions=...)).

The value both take is TargetRegions: per group (dataset), per genome, an int64
array [k, 3] of (seq_index, start, end) in normal form -- sorted by (seq_index,
start), 0 <= start < end <= the sequence's length, neither overlapping nor touching
inside a sequence.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)

_EMPTY2 = np.zeros((0, 2), dtype=np.int64)
_EMPTY3 = np.zeros((0, 3), dtype=np.int64)
_MAX_LISTED = 5


# ---------------------------------------------------------------- intervals in NumPy
def union(iv):
    """[k, 2] (start, end) in any order, empty ones allowed -> the normal form of
    their union: sorted, overlapping and touching intervals merged."""
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
    iv = iv[iv[:, 1] > iv[:, 0]]
    if iv.shape[0] == 0:
        return _EMPTY2
    iv = iv[np.lexsort((iv[:, 1], iv[:, 0]))]
    reach = np.maximum.accumulate(iv[:, 1])
    first = np.ones(iv.shape[0], dtype=bool)
    first[1:] = iv[1:, 0] > reach[:-1]
    last = np.ones(iv.shape[0], dtype=bool)
    last[:-1] = first[1:]
    return np.stack([iv[first, 0], reach[last]], axis=1)


def _inside(iv, x):
    """Which of the points x lie in an interval of iv (normal form)."""
    if iv.shape[0] == 0:
        return np.zeros(x.shape, dtype=bool)
    i = np.searchsorted(iv[:, 0], x, side="right") - 1
    return (i >= 0) & (x < iv[np.maximum(i, 0), 1])


def subtract(a, b):
    """a minus b, both in normal form -> normal form."""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return a
    pts = np.unique(np.concatenate([a.ravel(), b.ravel()]))
    lo, hi = pts[:-1], pts[1:]
    keep = _inside(a, lo) & ~_inside(b, lo)
    return union(np.stack([lo[keep], hi[keep]], axis=1))


def clip(iv, length):
    """The part of iv (normal form) inside [0, length)."""
    if iv.shape[0] == 0:
        return iv
    out = np.stack([np.maximum(iv[:, 0], 0), np.minimum(iv[:, 1], int(length))], axis=1)
    return out[out[:, 1] > out[:, 0]]


# ---------------------------------------------------------------- BED
def read_bed(fn):
    """The lines of a BED file -> [(chrom, start, end, fn, line number)], start and
    end as written (int where they parse as one, else the text).  Tab- or
    space-separated `chrom start end`, further columns ignored; blank lines and
    lines starting with '#', 'track' or 'browser' are skipped; a line with fewer
    than three columns is an error."""
    out, bad = [], []
    with open(fn) as f:
        for no, line in enumerate(f, 1):
            s = line.strip()
            if not s or s.startswith("#") or s.startswith("track") or s.startswith("browser"):
                continue
            # (a tab-separated line may name a whole header, spaces included)
            cols = [c.strip() for c in s.split("\t")] if "\t" in s else s.split()
            if len(cols) < 3:
                bad.append("%s:%d: fewer than three columns" % (fn, no))
                continue
            vals = []
            for c in cols[1:3]:
                try:
                    vals.append(int(c))
                except ValueError:
                    vals.append(c)
            out.append((cols[0], vals[0], vals[1], fn, no))
    _raise_listed(bad)
    return out


def _raise_listed(bad):
    if bad:
        more = len(bad) - _MAX_LISTED
        raise ValueError("target regions: " + "; ".join(bad[:_MAX_LISTED])
                         + ("; and %d more" % more if more > 0 else ""))


def _resolve(lines, names_grouped, lengths_grouped):
    """BED lines -> {(group, record): [k, 2] intervals as written, empty ones
    dropped}.  A chrom names a record when it equals the whole header or its first
    whitespace-delimited token; it applies to every record of every group it
    names.  ValueError (up to five offenders, with file and line) for start > end,
    negative or non-integer coordinates, an end beyond a named record's length, a
    chrom that names no record."""
    index = {}
    for gi, names in enumerate(names_grouped):
        for ri, name in enumerate(names):
            keys = {name}
            tok = name.split()
            if tok:
                keys.add(tok[0])
            for key in keys:
                index.setdefault(key, []).append((gi, ri))
    found, bad = {}, []
    for chrom, a, b, fn, no in lines:
        at = "%s:%d" % (fn, no)
        if not isinstance(a, int) or not isinstance(b, int):
            bad.append("%s: coordinates %s %s are not integers" % (at, a, b))
            continue
        if a < 0 or b < 0:
            bad.append("%s: negative coordinate in %d %d" % (at, a, b))
            continue
        if a > b:
            bad.append("%s: start %d is greater than end %d" % (at, a, b))
            continue
        hits = index.get(chrom)
        if not hits:
            bad.append("%s: '%s' names no sequence of any dataset" % (at, chrom))
            continue
        for gi, ri in hits:
            n = lengths_grouped[gi][ri]
            if b > n:
                bad.append("%s: end %d lies beyond the %d bases of '%s'" % (at, b, n, names_grouped[gi][ri]))
                break
        else:
            if a < b:
                for hit in hits:
                    found.setdefault(hit, []).append((a, b))
    _raise_listed(bad)
    return {k: np.asarray(v, dtype=np.int64).reshape(-1, 2) for k, v in found.items()}


# ---------------------------------------------------------------- the value type
class TargetRegions:
    """per_group[g][j] = int64 [k, 3] of (seq_index, start, end) in normal form:
    the wanted bases of genome j of group g."""

    def __init__(self, per_group):
        self.per_group = [[np.asarray(a, dtype=np.int64).reshape(-1, 3) for a in grp] for grp in per_group]

    @classmethod
    def from_bed(cls, target_beds, exclude_beds, names_grouped, genomes_grouped):
        """names_grouped[g][j] = the FASTA header of genome j of group g
        (seq_io.read_named_genomes_from_fasta; every such genome is one
        sequence).  target_beds / exclude_beds: lists of file names, either may be
        empty or None."""
        lengths = [[len(g.seqs[0]) for g in grp] for grp in genomes_grouped]
        want = _resolve([l for fn in (target_beds or ()) for l in read_bed(fn)], names_grouped, lengths)
        drop = _resolve([l for fn in (exclude_beds or ()) for l in read_bed(fn)], names_grouped, lengths)
        per_group = []
        for gi, lens in enumerate(lengths):
            grp = []
            for ri, n in enumerate(lens):
                if target_beds:
                    w = union(want.get((gi, ri), _EMPTY2))
                else:
                    w = union([(0, n)])
                w = clip(subtract(w, union(drop.get((gi, ri), _EMPTY2))), n)
                grp.append(np.concatenate([np.zeros((w.shape[0], 1), dtype=np.int64), w], axis=1))
            per_group.append(grp)
        return cls(per_group)

    def select(self, group_indices):
        """The regions of the genomes kept: group_indices[g] = the genomes of group
        g in their new order (an index may repeat: sampling with replacement)."""
        return TargetRegions([[self.per_group[g][j] for j in idx] for g, idx in enumerate(group_indices)])

    def select_groups(self, groups):
        """The regions of these groups, in the order given."""
        return TargetRegions([self.per_group[g] for g in groups])

    def genome_intervals(self, group, genomes):
        """(universe int32[n], start int64[n], end int64[n]) with one universe per
        genome of `genomes` (a genome's sequences concatenated, as the set cover
        filter's targets lay them out), for engine.BaseMask."""
        un, st, en = [], [], []
        for j, (gnm, iv) in enumerate(zip(genomes, self.per_group[group])):
            if iv.shape[0] == 0:
                continue
            off = np.zeros(len(gnm.seqs) + 1, dtype=np.int64)
            np.cumsum([len(s) for s in gnm.seqs], out=off[1:])
            m = union(np.stack([off[iv[:, 0]] + iv[:, 1], off[iv[:, 0]] + iv[:, 2]], axis=1))    # (sequences abut)
            un.append(np.full(m.shape[0], j, dtype=np.int32))
            st.append(m[:, 0])
            en.append(m[:, 1])
        return _cat(un, np.int32), _cat(st, np.int64), _cat(en, np.int64)

    def sequence_intervals(self, flat, rc=False):
        """The same with one universe per SEQUENCE, over the genomes flat = [(group,
        genome index, Genome)] in order (coverage_analysis.Analyzer's targets);
        rc: on the reverse-complemented sequences, where [a, b) of a sequence of
        length n is [n - b, n - a)."""
        un, st, en = [], [], []
        base = 0
        for gi, j, gnm in flat:
            iv = self.per_group[gi][j]
            for s in range(len(gnm.seqs)):
                part = iv[iv[:, 0] == s]
                if part.shape[0]:
                    a, b = part[:, 1], part[:, 2]
                    if rc:
                        n = len(gnm.seqs[s])
                        a, b = (n - b)[::-1], (n - a)[::-1]
                    un.append(np.full(part.shape[0], base + s, dtype=np.int32))
                    st.append(a)
                    en.append(b)
            base += len(gnm.seqs)
        return _cat(un, np.int32), _cat(st, np.int64), _cat(en, np.int64)

    def summary(self, group, genomes):
        """(intervals, wanted bases, all bases, sequences with a wanted base,
        sequences) of a group."""
        ivs = self.per_group[group]
        seqs = sum(len(g.seqs) for g in genomes)
        with_wanted = sum(int(np.unique(iv[:, 0]).size) for iv in ivs)
        return (sum(iv.shape[0] for iv in ivs), sum(int((iv[:, 2] - iv[:, 1]).sum()) for iv in ivs),
                sum(len(s) for g in genomes for s in g.seqs), with_wanted, seqs)


def _cat(parts, dtype):
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)


# ---------------------------------------------------------------- command lines
def add_arguments(parser):
    parser.add_argument("--target-regions", nargs="+", metavar="BED",
                        help="design only for the bases of these intervals (BED: chrom start end, 0-based, "
                             "half-open; chrom = a FASTA header or its first word): the wanted bases of every "
                             "sequence are the union of the intervals that name it; candidates still come "
                             "from the whole genomes and -e extends into the flanks")
    parser.add_argument("--exclude-regions", nargs="+", metavar="BED",
                        help="leave the bases of these intervals out of what is to be covered (same format; "
                             "taken away after --target-regions): no probe is spent on them, though a "
                             "probe picked for its other bases may cover them")


def given(args):
    return bool(getattr(args, "target_regions", None) or getattr(args, "exclude_regions", None))


def from_args(args, names_grouped, genomes_grouped):
    """The TargetRegions of a parsed command line (None: neither option given)."""
    if not given(args):
        return None
    return TargetRegions.from_bed(args.target_regions, args.exclude_regions, names_grouped, genomes_grouped)
