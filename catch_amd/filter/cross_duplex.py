"""Cross-dimer dG: how FIRMLY probes of one pool anneal to each other.  Not in
the reference; the quantities are defined here, in integers.

Records, bases and pairs(x, y) are those of catch_amd/filter/cross_dimer.py:
bytes as they are, only 'A', 'C', 'G', 'T' are bases, and s[x] pairs with t[y]
iff both are bases and Watson-Crick complements.

dg(d), the stack energy of the dinucleotide d = s[x] s[x+1] read 5'->3' on one
strand, is the unified nearest-neighbour parameter of SantaLucia 1998 (dG at 37
degrees C, 1 M NaCl) in hundredths of a kcal/mol:

    AA TT -100    AT -88     TA -58     CA TG -145    GT AC -144
    CT AG -128    GA TC -130 CG -217    GC -224       GG CC -184

and term(c) is +98 for 'G' or 'C' and +103 for 'A' or 'T'.  A stretch of two
records s and t is a triple (a, b, n), n >= 2, with pairs(a + k, b - k) for
every k in 0 .. n - 1, every index inside its record.  Its stability is

    stab(a, b, n) = -(sum over k in 0 .. n - 2 of dg(s[a+k] s[a+k+1])
                      + term(s[a]) + term(s[a+n-1]))

-- minus the dG of that duplex, so larger is firmer; one base pair is no duplex.

    duplex(s, t)  the maximum of stab over all stretches, 0 if that maximum is
                  negative or there is no stretch.
    dcross(i)     for a list of records, the maximum of duplex(s_i, s_j) over
                  j != i, 0 for a list of one.  An equal record at another
                  index is a partner, as for cross_dimer's cross.
    dpartner(i)   the smallest j != i that reaches dcross(i), -1 if it is 0.

Two properties (tests/test_cross_duplex.py checks both by brute force):
  * duplex(s, t) = duplex(t, s): the table is symmetric under reverse
    complement (dg(xy) = dg(comp(y) comp(x)), term(c) = term(comp(c))), and the
    stretch (a, b, n) of (s, t) is the stretch (b - n + 1, a + n - 1, n) of
    (t, s) over the complementary bases read the other way.
  * the maximum is always reached by a MAXIMAL stretch: one more pair adds a
    stack of at most -58 and changes one terminal by at most 5.  So it is
    enough to score maximal runs, which is what the NumPy form and the kernel
    do.
A stretch of n pairs has stab <= 224 (n - 1) - 196, so against a threshold t no
run of at most (t + 196) // 224 + 1 pairs matters (csrc/duplex.hip aims its run
search by that).

--max-cross-dimer-dg G (0 <= G <= 600, in kcal/mol, decimal text or a fraction,
read exactly): G_c = floor(100 G), and a pair {i, j}, i != j, conflicts iff
duplex(s_i, s_j) > G_c -- its firmest stretch has a dG below -G.

The model: contiguous perfect stretches only -- no mismatches, bulges, loops or
dangling ends; 37 degrees C and 1 M NaCl, no salt or temperature option.  It
ranks pairs; it is no promise of an absolute dG.

The measure is here three times, like cross_dimer's: duplex / dcross_list /
cross_duplex_against (from the quantifiers: the oracle of the other two),
dcross_numpy / against_numpy (run_rows' DP carrying the stack sum and the start
terminal of the run in hand: the host path) and engine.cross_duplex and its
siblings (csrc/duplex.hip, records of at most 256 characters).  measure,
measure_against and flags_against choose as cross_dimer's do.
"""
import logging
import math

import numpy as np

from catch_amd.filter import cross_dimer
from catch_amd.filter.candidate_rule import _fraction
from catch_amd.filter.cross_dimer import _CHUNK_CELLS, _PARTNER, _digits, _longest, _on_host

logger = logging.getLogger(__name__)

DG = {"AA": -100, "TT": -100, "AT": -88, "TA": -58, "CA": -145, "TG": -145, "GT": -144, "AC": -144,
      "CT": -128, "AG": -128, "GA": -130, "TC": -130, "CG": -217, "GC": -224, "GG": -184, "CC": -184}
TERM = {"A": 103, "T": 103, "C": 98, "G": 98}
MAX_DG = 600                 # the largest G the options take, kcal/mol (224 * 255 hundredths is the largest value)
# -dg by cross_dimer._digits' digits (first, second) and term by digit
_STACK = np.array([[-DG[a + b] for b in cross_dimer.BASES] for a in cross_dimer.BASES], dtype=np.int32)
_TERM = np.array([TERM[c] for c in cross_dimer.BASES], dtype=np.int32)


# ---------------------------------------------------------------- the definition
def stab(s, a, n):
    """stab(a, b, n) of a stretch that starts at s[a]: the record s alone decides."""
    return -(sum(DG[s[a + k:a + k + 2]] for k in range(n - 1)) + TERM[s[a]] + TERM[s[a + n - 1]])


def duplex(s, t):
    """duplex(s, t) from the quantifiers: every stretch, maximal or not."""
    best = 0
    for a in range(len(s)):
        for b in range(len(t)):
            n = 0
            while a + n <= len(s) - 1 and b - n >= 0 and _PARTNER.get(s[a + n]) == t[b - n]:
                n += 1
                if n >= 2:
                    best = max(best, stab(s, a, n))
    return best


def dcross_list(seqs):
    """(values, partners): two lists, dcross(i) and dpartner(i) of every record."""
    seqs = list(seqs)
    values, partners = [], []
    for i, s in enumerate(seqs):
        best, who = 0, -1
        for j, t in enumerate(seqs):
            if j != i:
                v = duplex(s, t)
                if v > best:
                    best, who = v, j
        values.append(best)
        partners.append(who)
    return values, partners


def cross_duplex_against(b, A):
    """(value, partner) from the quantifiers: the maximum of duplex(b, a) over
    the records a of the list A (0 for an empty A) and the smallest index into A
    that reaches it (-1 when the value is 0); nothing is exempted."""
    best, who = 0, -1
    for j, a in enumerate(A):
        v = duplex(b, a)
        if v > best:
            best, who = v, j
    return best, who


# ---------------------------------------------------------------- NumPy: the host path
def duplex_rows(mine, d):
    """int32 (len(mine), n): duplex(s_i, t_j) for the records of the _digits
    array `mine` against those of the _digits array `d`.  cross_dimer.run_rows'
    walk -- row x from row x - 1, cell (x, y) from cell (x - 1, y + 1) -- with
    two numbers per cell in place of one: the pairs of the run that ends there
    and, in one word, the sum of -dg over its stacks minus the terminal of its
    start.  The run that ends at a cell is the longest stretch that ends there,
    and by the second property no shorter one is firmer."""
    n, L = d.shape
    wants = np.where(d >= 0, 3 - d, -2).astype(np.int8)      # the digit that pairs with each character of t_j
    R = mine.shape[0]
    cells = np.zeros((R, n, L + 1), dtype=np.int16)          # (a zero behind the last column: y + 1 = L)
    held = np.zeros((R, n, L + 1), dtype=np.int32)           # stacks so far - term(start)
    best = np.zeros((R, n), dtype=np.int32)
    for x in range(_longest(mine)):
        here = mine[:, x]
        m = wants[None, :, :] == here[:, None, None]
        term = _TERM[np.maximum(here, 0)][:, None, None]
        if x:
            before = mine[:, x - 1]
            stack = np.where((before >= 0) & (here >= 0), _STACK[np.maximum(before, 0), np.maximum(here, 0)], 0)
        else:
            stack = np.zeros(R, dtype=np.int32)
        on = cells[:, :, 1:] > 0
        held[:, :, :L] = np.where(on, held[:, :, 1:] + stack[:, None, None], -term) * m
        cells[:, :, :L] = (cells[:, :, 1:] + 1) * m
        score = np.where(cells[:, :, :L] >= 2, held[:, :, :L] - term, 0)
        np.maximum(best, score.max(axis=2), out=best)
    return best


def _chunks(ds, d_all, order):
    """(rows, duplex_rows of them) over the index array `order`, a bounded number of cells at a time."""
    n, L = d_all.shape
    step = max(1, _CHUNK_CELLS // (n * (L + 1)))
    for lo in range(0, len(order), step):
        rows = order[lo:lo + step]
        yield rows, duplex_rows(ds[rows], d_all)


def duplex_matrix(seqs):
    """int32 (n, n): duplex(s_i, s_j), the diagonal 0.  Quadratic in time AND memory: for tests and small lists."""
    seqs = list(seqs)
    n = len(seqs)
    out = np.zeros((n, n), dtype=np.int32)
    if n:
        d = _digits(seqs)
        for rows, got in _chunks(d, d, np.argsort([len(s) for s in seqs], kind="stable")):
            out[rows] = got
        np.fill_diagonal(out, 0)
    return out


def dcross_numpy(seqs):
    """dcross_list as (values int32[n], partners int32[n]): the DP over ALL
    n * n ordered pairs, a chunk of rows at a time -- quadratic; lists of more
    than a few thousand probes belong on the device."""
    seqs = list(seqs)
    n = len(seqs)
    values = np.zeros(n, dtype=np.int32)
    partners = np.full(n, -1, dtype=np.int32)
    if n < 2:
        return values, partners
    d = _digits(seqs)
    for rows, got in _chunks(d, d, np.argsort([len(s) for s in seqs], kind="stable")):
        got[np.arange(len(rows)), rows] = -1                      # the record itself is no partner
        values[rows] = np.maximum(got.max(axis=1), 0)
        partners[rows] = np.where(values[rows] > 0, got.argmax(axis=1), -1)     # (argmax: the first of equals)
    return values, partners


def against_numpy(bs, as_):
    """cross_duplex_against of every record of `bs` as (values int32[nb],
    partners int32[nb]): the host path."""
    bs, as_ = list(bs), list(as_)
    nb = len(bs)
    values = np.zeros(nb, dtype=np.int32)
    partners = np.full(nb, -1, dtype=np.int32)
    if nb == 0 or not as_:
        return values, partners
    for rows, got in _chunks(_digits(bs), _digits(as_), np.argsort([len(s) for s in bs], kind="stable")):
        values[rows] = got.max(axis=1)
        partners[rows] = np.where(values[rows] > 0, got.argmax(axis=1), -1)
    return values, partners


def measure(seqs):
    """(values int32[n], partners int32[n]): dcross and dpartner on the device,
    or on the host path (CATCHHIP_HOST_FRONT_END=1, or a record longer than 256
    characters) -- the same values."""
    seqs = list(seqs)
    if not seqs:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if _on_host(seqs):
        return dcross_numpy(seqs)
    from catch_amd import engine
    return engine.cross_duplex(engine.default_context(), seqs)


def walk(seqs, above):
    """bool[n] on the host: keep[i] iff no kept j < i has duplex(s_i, s_j) > above."""
    seqs = list(seqs)
    keep = np.zeros(len(seqs), dtype=bool)
    if seqs:
        d = _digits(seqs)
        for rows, got in _chunks(d, d, np.arange(len(seqs))):
            for k, i in enumerate(rows.tolist()):
                keep[i] = not ((got[k, :i] > above) & keep[:i]).any()
    return keep


def measure_against(bs, as_):
    """cross_duplex_against of every record of `bs` against the list `as_`,
    (values int32[nb], partners int32[nb]), on the device
    (engine.cross_duplex_against) or on the host path, as measure chooses."""
    bs, as_ = list(bs), list(as_)
    if not bs or not as_:
        return np.zeros(len(bs), dtype=np.int32), np.full(len(bs), -1, dtype=np.int32)
    if _on_host(bs + as_):
        return against_numpy(bs, as_)
    from catch_amd import engine
    return engine.cross_duplex_against(engine.default_context(), bs, as_)


def flags_against(bs, as_, above):
    """bool[nb]: whether duplex(b, a) > above for some record a of `as_`, on
    the device (engine.cross_duplex_against_flags) or on the host path."""
    bs, as_ = list(bs), list(as_)
    if not bs or not as_:
        return np.zeros(len(bs), dtype=bool)
    if _on_host(bs + as_):
        return against_numpy(bs, as_)[0] > above
    from catch_amd import engine
    return engine.cross_duplex_against_flags(engine.default_context(), bs, as_, above)


# ---------------------------------------------------------------- the threshold and the rule
def threshold(g, what="max_cross_dimer_dg"):
    """G_c = floor(100 G) of a threshold G in kcal/mol: a string (decimal text
    or a fraction), an integer or a Fraction, never a float; 0 <= G <= 600."""
    if isinstance(g, bool) or g is None:
        raise ValueError("%s must be a number of kcal/mol, not %r" % (what, g))
    g = _fraction(g, what)
    if not 0 <= g <= MAX_DG:
        raise ValueError("%s must lie in 0 .. %d kcal/mol, not %s" % (what, MAX_DG, g))
    return math.floor(100 * g)


class DgRule:
    """The conflict rule of --max-cross-dimer-dg G: duplex > floor(100 G).  The
    same five methods as cross_dimer.LengthRule, for CrossDimerFilter and the
    set cover filter's redesign rounds."""
    noun = "cross-dimer dG"

    def __init__(self, g):
        self.above = threshold(g)

    def measure(self, seqs):
        return measure(seqs)

    def walk(self, seqs):
        return walk(seqs, self.above)

    def flags_host(self, bs, as_):
        return against_numpy(bs, as_)[0] > self.above

    def graph(self, ctx, strs):
        from catch_amd import engine
        return engine.RedundancyGraph.cross_duplex(ctx, strs, self.above)

    def flags_device(self, ctx, bs, as_):
        from catch_amd import engine
        return engine.cross_duplex_against_flags(ctx, bs, as_, self.above)


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The two options of catch_amd.design and catch_amd.probe_report."""
    p.add_argument("--cross-dimer-dg", action="store_true",
                   help="in the probe report, two more columns: cross_dg, the "
                        "stability of the firmest stretch over which the probe "
                        "and ANOTHER probe of the list can anneal (minus its "
                        "nearest-neighbour dG at 37 degrees C and 1 M NaCl, in "
                        "hundredths of a kcal/mol; contiguous perfect "
                        "stretches only), and cross_dg_partner, the number of "
                        "the first record that reaches it (1-based, NA when "
                        "the value is 0) "
                        "(catch_amd/filter/cross_duplex.py has the definition)")
    p.add_argument("--max-cross-dimer-dg", metavar="G",
                   help="probes whose firmest common stretch has a dG below -G "
                        "kcal/mol conflict (0 <= G <= %d, decimal text or a "
                        "fraction; compared as floor(100 G) hundredths).  The "
                        "energy counterpart of --max-cross-dimer X, with its "
                        "walk and its refusals, and not to be combined with "
                        "it in a design: ten bases of GCGCGCGCGC (17.9 "
                        "kcal/mol) hold about twice as firmly as sixteen of "
                        "ATATATATATATATAT (9.0).  In the probe report (implies "
                        "--cross-dimer-dg) both probes of a conflicting pair "
                        "fail the rule cross-dg" % MAX_DG)


def check_args(args, error):
    """Bad values of add_arguments' options go to error (ArgumentParser.error
    in the parsers); args.max_cross_dimer_dg stays the text that was given."""
    if args.max_cross_dimer_dg is not None:
        try:
            threshold(args.max_cross_dimer_dg, "--max-cross-dimer-dg")
        except ValueError as exc:
            error(str(exc))
