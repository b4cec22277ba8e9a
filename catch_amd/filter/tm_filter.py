"""Removes candidate probes by their melting temperature under the nearest-
neighbour model, and measures the distribution of that temperature.  Not in
the reference; the rule is defined here, in integers, and the order of the
input is kept.

A candidate is a string s of L >= 2 characters; with L < 2 the rule drops
nothing and the histogram counts nothing.  Bytes are compared as they are:
only 'A', 'C', 'G' and 'T' are bases.

Parameters: the unified nearest-neighbour parameters of SantaLucia 1998,
enthalpy h in units of 100 cal/mol and entropy e in units of 0.1 cal/(K mol),
per dinucleotide s[j] s[j+1] read 5'->3' on the probe:

    AA, TT   -79  -222        CT, AG   -78  -210
    AT       -72  -204        GA, TC   -82  -222
    TA       -72  -213        CG      -106  -272
    CA, TG   -85  -227        GC       -98  -244
    GT, AC   -84  -224        GG, CC   -80  -199

A dinucleotide in which either byte is not a base contributes (0, 0).
Initiation, for each of the two terminal characters s[0] and s[L-1]: (+1, -28)
if it is 'G' or 'C', else (+23, +41) -- 'A', 'T', 'N' and anything else.  There
is no symmetry term: a probe is not treated as self-complementary.  H is the
sum of all h, E the sum of all e.

Conditions (sodium_mm = Na in mM, oligo_nm = C in nM, the total strand
concentration, formamide_pct = F in percent; strings or Fractions, never
floats):
    Q(L) = round(1000 (1.987 ln(C 1e-9 / 4) + 0.368 (L - 1) ln(Na / 1000)))
computed once per length on the host with math.log -- the only floating-point
step; the integer Q(L) is what the NumPy path and the kernel receive, so they
cannot disagree.  L - 1 counts every character, 'N' too.  Q(L) <= -8200 is
required (100 E is at most +8200, so the denominator below stays negative):
ValueError otherwise.  At the defaults (50, 50, 0) Q(2) = -37261, Q(100) =
-145299.  f = floor(62 F + 1/2): 0.62 degrees per percent formamide, in
hundredths of a degree.

Value, all in 64-bit integers:
    E'   = 100 E + Q(L)                                  (negative)
    T    = floor(10^7 (-H) / (-E')) if H < 0, else 0     (hundredths of a kelvin)
    tm_c = T - 27315 - f                                 (hundredths of a degree Celsius)

Filter (tm_range = (MIN, MAX), degrees Celsius, -300 <= MIN <= MAX <= 300):
lo_c = ceil(100 MIN), hi_c = floor(100 MAX); kept iff lo_c <= tm_c <= hi_c.
tm_range = None measures only and drops nothing.

Histogram: 128 bins of whole degrees, bin b = min(max(floor(tm_c / 100), 0),
127); every candidate the filter sees is counted, duplicates too, before the
rule drops anything.  `histogram` and `dropped` = [below, above, any]
accumulate over all calls.

It is a two-state model calibrated on short oligos: on 100-mers it ranks
probes consistently, but its absolute values are not a promise.

The rule is here three times: _tm_c / _keeps (straight from the definition
above: the oracle of the other two), _filter_strs (NumPy, equal-length
candidates) and _apply_to_candidates (catchhip_candidates_drop_tm, one kernel
over the unique candidates of the device front end).
"""
import math
import threading
from fractions import Fraction

import numpy as np

from catch_amd.filter.candidate_rule import CandidateRuleFilter, _fraction, _value_error

BASES = "ACGT"
NBINS = 128
Q_MAX = -8200

# (h, e) per dinucleotide, 5'->3'
NN = {
    "AA": (-79, -222), "TT": (-79, -222), "AT": (-72, -204), "TA": (-72, -213),
    "CA": (-85, -227), "TG": (-85, -227), "GT": (-84, -224), "AC": (-84, -224),
    "CT": (-78, -210), "AG": (-78, -210), "GA": (-82, -222), "TC": (-82, -222),
    "CG": (-106, -272), "GC": (-98, -244), "GG": (-80, -199), "CC": (-80, -199),
}
INIT_GC, INIT_OTHER = (1, -28), (23, 41)

# NumPy form of the table: bytes to 0..3 (4: not a base), a dinucleotide to 5 * first + second
_CODE = np.full(256, 4, dtype=np.int64)
_CODE[np.frombuffer(BASES.encode(), dtype=np.uint8)] = np.arange(4)
_H25 = np.zeros(25, dtype=np.int64)
_E25 = np.zeros(25, dtype=np.int64)
for _d, (_h, _e) in NN.items():
    _H25[5 * BASES.index(_d[0]) + BASES.index(_d[1])] = _h
    _E25[5 * BASES.index(_d[0]) + BASES.index(_d[1])] = _e


def _conditions(sodium_mm, oligo_nm, formamide_pct):
    na = _fraction(sodium_mm, "the sodium concentration")
    c = _fraction(oligo_nm, "the oligo concentration")
    f = _fraction(formamide_pct, "the formamide percentage")
    if na <= 0:
        raise ValueError("the sodium concentration must be above 0 mM, not %s" % (sodium_mm,))
    if c <= 0:
        raise ValueError("the oligo concentration must be above 0 nM, not %s" % (oligo_nm,))
    if not 0 <= f <= 100:
        raise ValueError("the formamide percentage must lie in [0, 100], not %s" % (formamide_pct,))
    return na, c, f


def _range(tm_range):
    try:
        lo, hi = tm_range
    except (TypeError, ValueError):
        raise ValueError("tm_range must be a pair (MIN, MAX), not %r" % (tm_range,))
    lo_f, hi_f = _fraction(lo, "the Tm minimum"), _fraction(hi, "the Tm maximum")
    if not (-300 <= lo_f and hi_f <= 300):
        raise ValueError("the Tm bounds must lie in [-300, 300] degrees Celsius, not %s and %s" % (lo, hi))
    if lo_f > hi_f:
        raise ValueError("the Tm minimum (%s) exceeds the maximum (%s)" % (lo, hi))
    return lo_f, hi_f


class TmFilter(CandidateRuleFilter):
    def __init__(self, tm_range=None, sodium_mm="50", oligo_nm="50", formamide_pct="0"):
        self.sodium_mm, self.oligo_nm, self.formamide_pct = _conditions(sodium_mm, oligo_nm, formamide_pct)
        self.tm_min = self.tm_max = self.lo_c = self.hi_c = None
        if tm_range is not None:
            self.tm_min, self.tm_max = _range(tm_range)
            self.lo_c = -((-100 * self.tm_min.numerator) // self.tm_min.denominator)       # ceil(100 MIN)
            self.hi_c = (100 * self.tm_max.numerator) // self.tm_max.denominator           # floor(100 MAX)
        self.offset_c = 27315 + math.floor(62 * self.formamide_pct + Fraction(1, 2))    # 27315 + f
        self.dropped = [0, 0, 0]              # [below, above, any], over all calls
        self.histogram = [0] * NBINS          # candidates per whole degree, over all calls
        self._q_of = {}
        self._lock = threading.Lock()         # (groups in flight are filtered on several host threads)

    def _count(self, three, hist):
        with self._lock:
            self.dropped = [a + int(b) for a, b in zip(self.dropped, three)]
            if hist is not None:
                self.histogram = [a + int(b) for a, b in zip(self.histogram, hist)]

    def _q(self, L):
        """Q(L), the salt and concentration term of candidates of L characters."""
        q = self._q_of.get(L)
        if q is None:
            q = round(1000 * (1.987 * math.log(float(self.oligo_nm) * 1e-9 / 4)
                              + 0.368 * (L - 1) * math.log(float(self.sodium_mm) / 1000)))
            if q > Q_MAX:
                raise ValueError("Q(%d) = %d at %s mM sodium and %s nM oligo: the model needs Q <= %d "
                                 "(less sodium or less oligo)" % (L, q, self.sodium_mm, self.oligo_nm, Q_MAX))
            self._q_of[L] = q
        return q

    # ------------------------------------------------------------ the definition
    @staticmethod
    def _h_e(s):
        """(H, E) of s, len(s) >= 2."""
        H = E = 0
        for j in range(len(s) - 1):
            h, e = NN.get(s[j:j + 2], (0, 0))
            H, E = H + h, E + e
        for c in (s[0], s[-1]):
            h, e = INIT_GC if c in "GC" else INIT_OTHER
            H, E = H + h, E + e
        return H, E

    def _tm_c(self, s):
        """tm_c of s in hundredths of a degree Celsius; None if len(s) < 2."""
        L = len(s)
        if L < 2:
            return None
        H, E = self._h_e(s)
        E1 = 100 * E + self._q(L)
        T = (10 ** 7 * -H) // -E1 if H < 0 else 0
        return T - self.offset_c

    def _side(self, tm_c):
        """-1: dropped below, +1: dropped above, 0: kept."""
        if tm_c is None or self.lo_c is None:
            return 0
        return -1 if tm_c < self.lo_c else 1 if tm_c > self.hi_c else 0

    def _keeps(self, s):
        return self._side(self._tm_c(s)) == 0

    # ------------------------------------------------------------ NumPy, one length
    def _tm_c_equal_length(self, strs, L):
        """_tm_c for strings of one length L >= 2 at once: an int64 array."""
        n = len(strs)
        rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(n, L)
        code = _CODE[rows]
        pair = 5 * code[:, :-1] + code[:, 1:]
        H = _H25[pair].sum(axis=1)
        E = _E25[pair].sum(axis=1)
        for end in (rows[:, 0], rows[:, -1]):
            gc = (end == ord("G")) | (end == ord("C"))
            H += np.where(gc, INIT_GC[0], INIT_OTHER[0])
            E += np.where(gc, INIT_GC[1], INIT_OTHER[1])
        E1 = 100 * E + self._q(L)
        T = np.where(H < 0, (10 ** 7 * -H) // -np.where(H < 0, E1, -1), 0)
        return T - self.offset_c

    def _measure(self, tm_c):
        """(keep mask, [below, above, any], histogram) of an int64 array of tm_c."""
        hist = np.bincount(np.clip(tm_c // 100, 0, NBINS - 1), minlength=NBINS)
        if self.lo_c is None:
            return np.ones(len(tm_c), dtype=bool), [0, 0, 0], hist
        below, above = tm_c < self.lo_c, tm_c > self.hi_c
        nb, na = int(below.sum()), int(above.sum())
        return ~(below | above), [nb, na, nb + na], hist

    def _keep_mask_equal_length(self, strs, L):
        """_keeps for strings of one length L at once (candidate probes); counts them and what it drops."""
        if L < 2:
            return np.ones(len(strs), dtype=bool)
        keep, three, hist = self._measure(self._tm_c_equal_length(strs, L))
        self._count(three, hist)
        return keep

    def _keep_list(self, strs):
        """_keeps string by string, Q per length; counts them and what it drops."""
        tm = [self._tm_c(s) for s in strs]
        side = [self._side(t) for t in tm]
        hist = [0] * NBINS
        for t in tm:
            if t is not None:
                hist[min(max(t // 100, 0), NBINS - 1)] += 1
        nb, na = side.count(-1), side.count(1)
        self._count([nb, na, nb + na], hist)
        return [x == 0 for x in side]

    # ------------------------------------------------------------ the device front end
    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        if cands.L < 2:
            return
        self._count(*cands.drop_tm(self._q(cands.L), self.offset_c, self.lo_c, self.hi_c, histogram=True))

    # ------------------------------------------------------------ the histogram file
    def write_histogram(self, path):
        """tm_c <tab> candidates, one row per whole degree from the lowest
        non-empty bin to the highest (empty bins between them included); bin 0
        holds everything below 1 degree, bin 127 everything from 127 up."""
        with self._lock:
            hist = list(self.histogram)
        filled = [b for b, v in enumerate(hist) if v]
        with open(path, "w") as f:
            f.write("tm_c\tcandidates\n")
            if filled:
                for b in range(filled[0], filled[-1] + 1):
                    f.write("%d\t%d\n" % (b, hist[b]))


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The five options of catch_amd.design and catch_amd.design_grid."""
    p.add_argument("--filter-tm", nargs=2, metavar=("MIN", "MAX"),
                   help="drop candidate probes whose melting temperature "
                        "lies outside [MIN, MAX] degrees Celsius (decimal "
                        "text or a fraction, read exactly): the nearest-"
                        "neighbour model with the unified parameters of "
                        "SantaLucia 1998, in integers (catch_amd/filter/"
                        "tm_filter.py has the rule); a two-state model "
                        "calibrated on short oligos, which ranks long probes "
                        "consistently but whose absolute values are not a "
                        "promise, so look at --write-tm-histogram first; "
                        "like --filter-polya this comes before the set "
                        "cover, so bases that only dropped candidates would "
                        "cover become uncoverable and -c refers to what is "
                        "left")
    p.add_argument("--tm-sodium", metavar="MM",
                   help="sodium concentration of --filter-tm and "
                        "--write-tm-histogram in mM (default 50)")
    p.add_argument("--tm-oligo", metavar="NM",
                   help="total strand concentration of --filter-tm and "
                        "--write-tm-histogram in nM (default 50)")
    p.add_argument("--tm-formamide", metavar="PCT",
                   help="formamide of --filter-tm and --write-tm-histogram in "
                        "percent; lowers every Tm by 0.62 degrees per percent "
                        "(default 0)")
    p.add_argument("--write-tm-histogram", metavar="FILE",
                   help="write the melting temperatures of the candidate "
                        "probes to FILE as a TSV (tm_c, candidates), one row "
                        "per whole degree: the candidates that survive the "
                        "filters before this one (--filter-from-fasta, "
                        "--filter-polya, the composition and structure "
                        "filters), duplicates counted, before --filter-tm "
                        "drops any and over all datasets; without --filter-tm "
                        "it only measures and the design is unchanged")


def from_args(args, error=_value_error):
    """A new TmFilter as the options of add_arguments ask for, or None without
    them; bad values go to error (ArgumentParser.error in the parsers, so that
    they are argparse errors)."""
    conditions = [("--tm-sodium", args.tm_sodium), ("--tm-oligo", args.tm_oligo), ("--tm-formamide", args.tm_formamide)]
    if args.filter_tm is None and args.write_tm_histogram is None:
        for name, value in conditions:
            if value is not None:
                error("%s needs --filter-tm or --write-tm-histogram" % name)
        return None
    try:
        f = TmFilter(tm_range=args.filter_tm,
                     sodium_mm="50" if args.tm_sodium is None else args.tm_sodium,
                     oligo_nm="50" if args.tm_oligo is None else args.tm_oligo,
                     formamide_pct="0" if args.tm_formamide is None else args.tm_formamide)
        if getattr(args, "probe_length", None) is not None and args.probe_length >= 2:
            f._q(args.probe_length)
    except ValueError as exc:
        error("--filter-tm / --write-tm-histogram: %s" % exc)
    return f
