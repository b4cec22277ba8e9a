"""Cross-dimers: probes of one pool that anneal to each other.  Not in the
reference; the quantities are defined here, in integers.

A record is a string of bytes as they are: only 'A', 'C', 'G' and 'T' are
bases; 'N', lower case and every other byte pair with nothing.  For two
records s and t, pairs(x, y) holds iff s[x] and t[y] are bases and t[y] is the
Watson-Crick complement of s[x] (A-T, C-G).

    run(s, t)   the largest n for which there are a, b with
                pairs(a + k, b - k) for every k in 0 .. n - 1 and every index
                inside its record, 0 if there is none: the self-dimer rule of
                quality.measure with the two copies replaced by two records.
                run(s, t) = run(t, s) = the longest common substring of s and
                the reverse complement of t over bases only.
    cross(i)    for a list of records, the maximum of run(s_i, s_j) over
                j != i, 0 for a list of one.  An equal record at another index
                is a partner like any other; the record itself is not (its own
                pairing is `dimer`).
    partner(i)  the smallest j != i with run(s_i, s_j) = cross(i), -1 if
                cross(i) = 0.

--max-cross-dimer X (X >= 1, by analogy with --max-self-dimer): a pair {i, j},
i != j, conflicts iff run(s_i, s_j) > X.  CrossDimerFilter keeps probe i iff no
KEPT probe j < i conflicts with it -- the lexicographically first maximal
independent set of the conflict graph in input order, so of a conflicting pair
the earlier probe stays.

The measure is here three times: run / cross_dimers (from the quantifiers
above: the oracle of the other two), cross_dimers_numpy (a DP over ALL pairs,
quadratic in the number of records: the host path) and engine.cross_dimer
(catchhip_cross_dimer, every pair on the device, records of at most 256
characters).  measure chooses: the device, unless CATCHHIP_HOST_FRONT_END=1
is set or a record is longer than 256 characters -- the whole list then goes
to the host path, with a warning.
"""
import logging
import os

import numpy as np

from catch_amd.filter.base_filter import BaseFilter
from catch_amd.filter.composition_filter import BASES, _int

logger = logging.getLogger(__name__)

MAX_DEVICE_LENGTH = 256      # characters per record the pair kernel takes (csrc/cross.hip)
_PARTNER = {"A": "T", "C": "G", "G": "C", "T": "A"}
_CHUNK_CELLS = 1 << 22       # cells of one NumPy step of run_rows


# ---------------------------------------------------------------- the definition
def run(s, t):
    """run(s, t) from the quantifiers."""
    best = 0
    for a in range(len(s)):
        for b in range(len(t)):
            n = 0
            while a + n <= len(s) - 1 and b - n >= 0 and _PARTNER.get(s[a + n]) == t[b - n]:
                n += 1
            best = max(best, n)
    return best


def cross_dimers(seqs):
    """(values, partners): two lists, cross(i) and partner(i) of every record."""
    seqs = list(seqs)
    values, partners = [], []
    for i, s in enumerate(seqs):
        best, who = 0, -1
        for j, t in enumerate(seqs):
            if j != i:
                r = run(s, t)
                if r > best:
                    best, who = r, j
        values.append(best)
        partners.append(who)
    return values, partners


# ---------------------------------------------------------------- NumPy: the host path
def _digits(seqs):
    """int8 (n, longest): 0 .. 3 for 'A', 'C', 'G', 'T', -1 for everything else and behind a record's end."""
    n = len(seqs)
    d = np.full((n, max([len(s) for s in seqs] + [1])), -1, dtype=np.int8)
    digit = np.full(256, -1, dtype=np.int8)
    digit[np.frombuffer(BASES.encode(), dtype=np.uint8)] = np.arange(4)
    for i, s in enumerate(seqs):
        d[i, :len(s)] = digit[np.frombuffer(s.encode("latin-1", "replace"), dtype=np.uint8)]
    return d


def run_rows(d, rows):
    """int32 (len(rows), n): run(s_i, s_j) for the records i of the index array
    `rows` and every j (j = i is the record's self-dimer), d = _digits(seqs).
    cells[y] = the pairs that end at cell (x, y), walking x up and y down, row x
    from row x - 1: cells_x[y] = pairs(x, y) ? cells_(x-1)[y + 1] + 1 : 0; run
    is the largest.  x stops at the longest of the records in `rows`."""
    n, L = d.shape
    wants = np.where(d >= 0, 3 - d, -2).astype(np.int8)      # the digit that pairs with each character of s_j
    mine = d[rows]
    cells = np.zeros((len(rows), n, L + 1), dtype=np.int16)  # (a zero behind the last column: y + 1 = L)
    best = np.zeros((len(rows), n), dtype=np.int16)
    for x in range(_longest(mine)):
        m = wants[None, :, :] == mine[:, x][:, None, None]
        cells[:, :, :L] = (cells[:, :, 1:] + 1) * m
        np.maximum(best, cells[:, :, :L].max(axis=2), out=best)
    return best.astype(np.int32)


def _longest(d):
    """Columns of a _digits array up to the last base of any of its records (what lies behind pairs with nothing)."""
    cols = np.flatnonzero((d >= 0).any(axis=0))
    return int(cols[-1]) + 1 if cols.size else 0


def _row_chunks(seqs, in_order=False):
    """(rows, run_rows(d, rows)) over all records, a bounded number of cells at a
    time: index arrays that partition 0 .. n - 1, the shortest records first
    (a chunk walks as far as its longest record), or ascending with in_order."""
    d = _digits(seqs)
    n, L = d.shape
    order = np.arange(n) if in_order else np.argsort([len(s) for s in seqs], kind="stable")
    step = max(1, _CHUNK_CELLS // (n * (L + 1)))
    for lo in range(0, n, step):
        rows = order[lo:lo + step]
        yield rows, run_rows(d, rows)


def run_matrix(seqs):
    """int32 (n, n): run(s_i, s_j), the diagonal 0.  Quadratic in time AND memory: for tests and small lists."""
    seqs = list(seqs)
    n = len(seqs)
    out = np.zeros((n, n), dtype=np.int32)
    if n:
        for rows, got in _row_chunks(seqs):
            out[rows] = got
        np.fill_diagonal(out, 0)
    return out


def cross_dimers_numpy(seqs):
    """cross_dimers as (values int32[n], partners int32[n]): a DP over ALL
    n * n ordered pairs, a chunk of rows at a time -- quadratic in the number
    of records (and in their length); lists of more than a few thousand
    probes belong on the device."""
    seqs = list(seqs)
    n = len(seqs)
    values = np.zeros(n, dtype=np.int32)
    partners = np.full(n, -1, dtype=np.int32)
    if n < 2:
        return values, partners
    for rows, got in _row_chunks(seqs):
        got[np.arange(len(rows)), rows] = -1                      # the record itself is no partner
        values[rows] = got.max(axis=1)
        partners[rows] = np.where(values[rows] > 0, got.argmax(axis=1), -1)     # (argmax: the first of equals)
    return values, partners


def _on_host(seqs):
    if os.environ.get("CATCHHIP_HOST_FRONT_END"):
        return True
    longest = max([len(s) for s in seqs] + [0])
    if longest > MAX_DEVICE_LENGTH:
        logger.warning("cross-dimer: a record of %d characters (the device pairs at most %d): all %d records take "
                       "the host path, which is quadratic", longest, MAX_DEVICE_LENGTH, len(seqs))
        return True
    return False


def measure(seqs):
    """(values int32[n], partners int32[n]) on the device, or on the host path
    (module docstring) -- the same values."""
    seqs = list(seqs)
    if not seqs:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if _on_host(seqs):
        return cross_dimers_numpy(seqs)
    from catch_amd import engine
    return engine.cross_dimer(engine.default_context(), seqs)


def walk(seqs, above):
    """bool[n] on the host: keep[i] iff no kept j < i has run(s_i, s_j) > above."""
    seqs = list(seqs)
    keep = np.zeros(len(seqs), dtype=bool)
    if seqs:
        for rows, got in _row_chunks(seqs, in_order=True):
            for k, i in enumerate(rows.tolist()):
                keep[i] = not ((got[k, :i] > above) & keep[:i]).any()
    return keep


# ---------------------------------------------------------------- one list against another
def cross_against(b, A):
    """(value, partner) from the quantifiers: the maximum of run(b, a) over the
    records a of the list A (0 for an empty A) and the smallest index into A
    that reaches it (-1 when the value is 0).  A member of A equal to b is a
    partner like any other -- the value is then run(b, b); nothing is
    exempted."""
    best, who = 0, -1
    for j, a in enumerate(A):
        r = run(b, a)
        if r > best:
            best, who = r, j
    return best, who


def conflicts_with(b, A, above):
    """Whether record b pairs with some record of A over more than `above` bases."""
    return cross_against(b, A)[0] > above


def cross_against_numpy(bs, as_):
    """cross_against of every record of `bs` as (values int32[nb], partners
    int32[nb]): run_rows' DP over the nb * na ordered pairs, a bounded number
    of cells at a time -- the host path."""
    bs, as_ = list(bs), list(as_)
    nb, na = len(bs), len(as_)
    values = np.zeros(nb, dtype=np.int32)
    partners = np.full(nb, -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return values, partners
    d = _digits(as_)
    L = d.shape[1]
    wants = np.where(d >= 0, 3 - d, -2).astype(np.int8)
    order = np.argsort([len(s) for s in bs], kind="stable")     # (a chunk walks as far as its longest record)
    step = max(1, _CHUNK_CELLS // (na * (L + 1)))
    for lo in range(0, nb, step):
        rows = order[lo:lo + step]
        mine = _digits([bs[i] for i in rows])
        cells = np.zeros((len(rows), na, L + 1), dtype=np.int16)
        best = np.zeros((len(rows), na), dtype=np.int16)
        for x in range(_longest(mine)):
            m = wants[None, :, :] == mine[:, x][:, None, None]
            cells[:, :, :L] = (cells[:, :, 1:] + 1) * m
            np.maximum(best, cells[:, :, :L].max(axis=2), out=best)
        values[rows] = best.max(axis=1)
        partners[rows] = np.where(values[rows] > 0, best.argmax(axis=1), -1)     # (argmax: the first of equals)
    return values, partners


def measure_against(bs, as_):
    """cross_against of every record of `bs` against the list `as_`, (values
    int32[nb], partners int32[nb]): on the device (engine.cross_against), or on
    the host path when CATCHHIP_HOST_FRONT_END=1 is set or a record of either
    list is longer than 256 characters -- the same values."""
    bs, as_ = list(bs), list(as_)
    if not bs or not as_:
        return np.zeros(len(bs), dtype=np.int32), np.full(len(bs), -1, dtype=np.int32)
    if _on_host(bs + as_):
        return cross_against_numpy(bs, as_)
    from catch_amd import engine
    return engine.cross_against(engine.default_context(), bs, as_)


def flags_against(bs, as_, above):
    """bool[nb]: conflicts_with(b, as_, above) for every record of `bs`, on the
    device (engine.cross_against_flags) or on the host path, as measure_against
    chooses."""
    bs, as_ = list(bs), list(as_)
    if not bs or not as_:
        return np.zeros(len(bs), dtype=bool)
    if _on_host(bs + as_):
        return cross_against_numpy(bs, as_)[0] > above
    from catch_amd import engine
    return engine.cross_against_flags(engine.default_context(), bs, as_, above)


# ---------------------------------------------------------------- the filter
def _threshold(x, what="max_cross_dimer"):
    x = _int(x, what)
    if x < 1:
        raise ValueError("%s must be at least 1, not %d" % (what, x))
    return x


class LengthRule:
    """The conflict rule of --max-cross-dimer X: run > X.  What CrossDimerFilter
    and the set cover filter's redesign rounds ask of the rule in force
    (cross_duplex.DgRule is the other one): the measure of a list, the walk and
    the flags on the host path, the conflict graph and the flags on the device."""
    noun = "cross-dimer"

    def __init__(self, x):
        self.above = _threshold(x)

    def measure(self, seqs):
        return measure(seqs)

    def walk(self, seqs):
        return walk(seqs, self.above)

    def flags_host(self, bs, as_):
        return cross_against_numpy(bs, as_)[0] > self.above

    def graph(self, ctx, strs):
        from catch_amd import engine
        return engine.RedundancyGraph.cross_dimer(ctx, strs, self.above)

    def flags_device(self, ctx, bs, as_):
        from catch_amd import engine
        return engine.cross_against_flags(ctx, bs, as_, self.above)


def rule_of(max_cross_dimer=None, max_cross_dimer_dg=None):
    """The one conflict rule of a design: LengthRule(X) or cross_duplex.DgRule(G)."""
    if max_cross_dimer_dg is not None:
        if max_cross_dimer is not None:
            raise ValueError("max_cross_dimer and max_cross_dimer_dg are two conflict rules: a design applies one")
        from catch_amd.filter import cross_duplex
        return cross_duplex.DgRule(max_cross_dimer_dg)
    return LengthRule(max_cross_dimer)


class CrossDimerFilter(BaseFilter):
    """Drops probes that conflict with an earlier kept probe: under
    max_cross_dimer = X those that pair with it over more than X consecutive
    bases, under max_cross_dimer_dg = G (a keyword; instead of X) those whose
    firmest stretch with it is firmer than G kcal/mol
    (catch_amd/filter/cross_duplex.py).  `dropped` and `seen` accumulate over
    the calls; largest_before / largest_after are the largest cross (or dcross)
    of the last call's input and output (0 for fewer than two probes)."""

    def __init__(self, max_cross_dimer=None, max_cross_dimer_dg=None):
        self.rule = rule_of(max_cross_dimer, max_cross_dimer_dg)
        self.max_cross_dimer = self.rule.above if max_cross_dimer_dg is None else None
        self.max_cross_dimer_dg = max_cross_dimer_dg
        self.dropped = 0
        self.seen = 0
        self.largest_before = 0
        self.largest_after = 0

    def _keep(self, strs):
        if _on_host(strs):
            return self.rule.walk(strs)
        from catch_amd import engine
        graph = self.rule.graph(engine.default_context(), strs)
        try:
            return graph.naive()
        finally:
            graph.close()

    def _filter(self, probes):
        probes = list(probes)
        strs = [p.seq_str for p in probes]
        if not strs:
            return probes
        keep = self._keep(strs)
        kept = [p for p, k in zip(probes, keep) if k]
        self.seen += len(probes)
        self.dropped += len(probes) - len(kept)
        self.largest_before = int(self.rule.measure(strs)[0].max())
        self.largest_after = int(self.rule.measure([p.seq_str for p in kept])[0].max())
        return kept

    def filter(self, input, target_genomes=None, input_is_grouped=False, num_processes=None):
        """Grouped input is ONE list to this filter -- the groups in order, a
        probe counted where it comes first, which is the order of the
        designer's merged output -- and every group gives up what that list
        drops."""
        if not input_is_grouped:
            return self._filter(input)
        merged = list(dict.fromkeys(p for group in input for p in group))
        kept = set(self._filter(merged))
        return [[p for p in group if p in kept] for group in input]


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The two options of catch_amd.design and catch_amd.probe_report."""
    p.add_argument("--cross-dimer", action="store_true",
                   help="in the probe report, two more columns: cross_dimer, "
                        "the longest stretch over which the probe and ANOTHER "
                        "probe of the list can anneal (antiparallel, no "
                        "mismatch; N and lower case pair with nothing), and "
                        "cross_partner, the number of the first record that "
                        "reaches it (1-based, NA when the value is 0); all "
                        "records are one list whatever their lengths "
                        "(catch_amd/filter/cross_dimer.py has the definition)")
    p.add_argument("--max-cross-dimer", type=int, metavar="X",
                   help="probes that anneal to each other over more than X "
                        "consecutive base pairs conflict; random 100-mers "
                        "reach 9 to 16 among a few hundred, so useful values "
                        "start around 20.  In the probe report (implies "
                        "--cross-dimer) both probes of a conflicting pair fail "
                        "the rule cross-dimer.  In the design commands the "
                        "probes the set cover picked, of all datasets and "
                        "clusters as one list, are walked in output order and "
                        "a probe is dropped when it conflicts with a kept "
                        "earlier one; bases that only dropped probes covered "
                        "become uncovered (--write-uncovered-regions and "
                        "--print-analysis show the cost; the design commands' "
                        "--cross-dimer-redesign designs around the conflicts "
                        "instead)")


def check_args(args, error):
    """Bad values of add_arguments' options go to error (ArgumentParser.error in the parsers)."""
    if args.max_cross_dimer is not None and args.max_cross_dimer < 1:
        error("--max-cross-dimer must be at least 1, not %d" % args.max_cross_dimer)
