"""Removes candidate probes by their composition: GC content outside a range,
a long homopolymer, low-complexity sequence.  Not in the reference; the rules
are defined here, in integers, and the order of the input is kept.

A candidate is a string s of length L.  Bytes are compared as they are: only
'A', 'C', 'G' and 'T' are bases, 'N' and everything else is "other".

GC range (gc_range = (MIN, MAX), fractions in [0, 1] given as strings or
Fractions, never floats: "0.4" of 100 bases is exactly 40).  gc = the number
of 'G' or 'C' in s.  Kept iff ceil(MIN * L) <= gc <= floor(MAX * L); L counts
every character, 'N' included.

Homopolymer (max_homopolymer = H >= 1).  Kept iff the longest run of one
identical base is <= H.  Runs of 'N' or other bytes do not count, and they
break a run.

Low complexity (max_dust = X >= 0, dust_window = W in 3..256): a DUST score
over fixed windows.  Triplet j (0 <= j <= L - 3) is valid iff s[j], s[j+1] and
s[j+2] are bases; its code is 16 a + 4 b + c.  We = min(W, L).  For every
window start i in 0 .. L - We take the valid triplets j with i <= j <= i + We - 3:
T is their number, c_t their number with code t and S the sum over t of
c_t (c_t - 1) / 2.  The candidate is dropped iff some window has T >= 2 and
10 S > X (T - 1).  X is in sdust's units (score x 10; sdust's default is 20).
If L < 3 nothing is dropped by this rule.  For orientation: a 64-base window of
'A' scores 310, (AC)n 152, random sequence about 5.

A candidate is dropped iff any enabled rule drops it.  `dropped` accumulates,
over all calls, the candidates [GC, homopolymer, low complexity, any rule]
dropped -- candidates as they come out of the sliding windows, duplicates
counted, and one that fails two rules counted for both and once in "any".

The rule is here three times: _keeps (straight from the definitions above: the
oracle of the other two), _filter_strs (NumPy, equal-length candidates) and
_apply_to_candidates (catchhip_candidates_drop_composition, one kernel over the
unique candidates of the device front end).
"""
import threading

import numpy as np

from catch_amd.filter.candidate_rule import CandidateRuleFilter, _fraction, _value_error

BASES = "ACGT"


def _unit_fraction(x, what):
    f = _fraction(x, what)
    if not 0 <= f <= 1:
        raise ValueError("%s must lie in [0, 1], not %s" % (what, x))
    return f


def _int(x, what):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (what, x))
    return int(x)


class CompositionFilter(CandidateRuleFilter):
    def __init__(self, gc_range=None, max_homopolymer=None, max_dust=None, dust_window=64):
        self.gc_min = self.gc_max = None
        if gc_range is not None:
            try:
                lo, hi = gc_range
            except (TypeError, ValueError):
                raise ValueError("gc_range must be a pair (MIN, MAX), not %r" % (gc_range,))
            self.gc_min, self.gc_max = _unit_fraction(lo, "the GC minimum"), _unit_fraction(hi, "the GC maximum")
            if self.gc_min > self.gc_max:
                raise ValueError("the GC minimum (%s) exceeds the maximum (%s)" % (lo, hi))
        self.max_homopolymer = None
        if max_homopolymer is not None:
            self.max_homopolymer = _int(max_homopolymer, "max_homopolymer")
            if self.max_homopolymer < 1:
                raise ValueError("max_homopolymer must be at least 1, not %d" % self.max_homopolymer)
        self.max_dust = None
        if max_dust is not None:
            self.max_dust = _int(max_dust, "max_dust")
            if self.max_dust < 0:
                raise ValueError("max_dust must be at least 0, not %d" % self.max_dust)
        self.dust_window = _int(dust_window, "dust_window")
        if not 3 <= self.dust_window <= 256:
            raise ValueError("dust_window must lie in 3..256, not %d" % self.dust_window)
        self.dropped = [0, 0, 0, 0]      # [GC, homopolymer, low complexity, any rule], over all calls
        self._lock = threading.Lock()    # (groups in flight are filtered on several host threads)

    def _count(self, four):
        with self._lock:
            self.dropped = [a + int(b) for a, b in zip(self.dropped, four)]

    def _gc_bounds(self, L):
        """(gc_lo, gc_hi) for candidates of L characters; (0, L) without the rule."""
        if self.gc_min is None:
            return 0, L
        lo = -((-self.gc_min.numerator * L) // self.gc_min.denominator)       # ceil(MIN * L)
        hi = (self.gc_max.numerator * L) // self.gc_max.denominator           # floor(MAX * L)
        return lo, hi

    # ------------------------------------------------------------ the definition
    def _fails(self, s):
        """(GC, homopolymer, low complexity): which rules drop s."""
        L = len(s)
        gc_lo, gc_hi = self._gc_bounds(L)
        gc = sum(1 for c in s if c in "GC")
        fails_gc = not gc_lo <= gc <= gc_hi
        fails_run = False
        if self.max_homopolymer is not None:
            longest = run = 0
            for j, c in enumerate(s):
                if c not in BASES:
                    run = 0
                elif j > 0 and s[j - 1] == c:
                    run += 1
                else:
                    run = 1
                longest = max(longest, run)
            fails_run = longest > self.max_homopolymer
        fails_dust = False
        if self.max_dust is not None and L >= 3:
            We = min(self.dust_window, L)
            for i in range(L - We + 1):
                counts = {}
                for j in range(i, i + We - 2):
                    t = s[j:j + 3]
                    if all(c in BASES for c in t):
                        counts[t] = counts.get(t, 0) + 1
                T = sum(counts.values())
                S = sum(c * (c - 1) // 2 for c in counts.values())
                if T >= 2 and 10 * S > self.max_dust * (T - 1):
                    fails_dust = True
                    break
        return fails_gc, fails_run, fails_dust

    def _keeps(self, s):
        return not any(self._fails(s))

    # ------------------------------------------------------------ NumPy, one length
    def _fail_masks_equal_length(self, strs, L):
        """_fails for strings of one length L at once: three bool arrays."""
        n = len(strs)
        rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(n, L)
        gc_lo, gc_hi = self._gc_bounds(L)
        gc = ((rows == ord("G")) | (rows == ord("C"))).sum(axis=1)
        fails_gc = (gc < gc_lo) | (gc > gc_hi)
        fails_run = np.zeros(n, dtype=bool)
        H = self.max_homopolymer
        if H is not None and H + 1 <= L:         # a run above H holds a window of H + 1 equal bases
            for base in BASES.encode():
                cs = np.zeros((n, L + 1), dtype=np.int32)
                np.cumsum(rows == base, axis=1, out=cs[:, 1:])
                fails_run |= ((cs[:, H + 1:] - cs[:, :L - H]) == H + 1).any(axis=1)
        fails_dust = np.zeros(n, dtype=bool)
        if self.max_dust is not None and L >= 3:
            We = min(self.dust_window, L)
            digit = np.full(256, -1, dtype=np.int32)
            digit[np.frombuffer(BASES.encode(), dtype=np.uint8)] = np.arange(4)
            d = digit[rows]
            code = 16 * d[:, :L - 2] + 4 * d[:, 1:L - 1] + d[:, 2:]
            code[(d[:, :L - 2] < 0) | (d[:, 1:L - 1] < 0) | (d[:, 2:] < 0)] = -1
            ntrip, width = L - 2, We - 2          # triplets of a candidate, of a window
            S = np.zeros((n, ntrip - width + 1), dtype=np.int32)
            T = np.zeros_like(S)
            cs = np.zeros((n, ntrip + 1), dtype=np.int32)
            for t in range(64):
                np.cumsum(code == t, axis=1, out=cs[:, 1:])
                c = cs[:, width:] - cs[:, :ntrip + 1 - width]
                S += c * (c - 1) // 2
                T += c
            fails_dust = ((T >= 2) & (10 * S.astype(np.int64) > self.max_dust * (T.astype(np.int64) - 1))).any(axis=1)
        return fails_gc, fails_run, fails_dust

    def _keep_mask_equal_length(self, strs, L):
        """_keeps for strings of one length L at once (candidate probes); counts what it drops."""
        fails = self._fail_masks_equal_length(strs, L)
        drop = fails[0] | fails[1] | fails[2]
        self._count([int(f.sum()) for f in fails] + [int(drop.sum())])
        return ~drop

    def _keep_list(self, strs):
        """_keeps string by string; counts what it drops."""
        fails = [self._fails(s) for s in strs]
        self._count([sum(f[k] for f in fails) for k in range(3)] + [sum(any(f) for f in fails)])
        return [not any(f) for f in fails]

    # ------------------------------------------------------------ the device front end
    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        L = cands.L
        gc_lo, gc_hi = self._gc_bounds(L) if self.gc_min is not None else (-1, -1)
        self._count(cands.drop_composition(
            gc_lo, gc_hi,
            -1 if self.max_homopolymer is None else min(self.max_homopolymer, 2 ** 31 - 1),
            -1 if self.max_dust is None else min(self.max_dust, 2 ** 31 - 1),
            self.dust_window))


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The four options of catch_amd.design and catch_amd.design_grid."""
    p.add_argument("--filter-gc", nargs=2, metavar=("MIN", "MAX"),
                   help="drop candidate probes whose GC content lies outside "
                        "[MIN, MAX] (fractions of the probe length, read "
                        "exactly: the number of G or C must be at least "
                        "ceil(MIN x length) and at most floor(MAX x length), "
                        "where the length counts N too); like --filter-polya "
                        "this comes before the set cover, so bases that only "
                        "dropped candidates would cover become uncoverable "
                        "and -c refers to what is left")
    p.add_argument("--max-homopolymer", type=int, metavar="H",
                   help="drop candidate probes with a run of more than H "
                        "identical bases (A, C, G or T; N does not count and "
                        "breaks a run); dropped candidates make bases "
                        "uncoverable as with --filter-polya")
    p.add_argument("--filter-low-complexity", type=int, metavar="X",
                   help="drop candidate probes with a low-complexity window: "
                        "a DUST score (sum over triplets of c(c-1)/2 over the "
                        "number of triplets less one, times 10 as in sdust, "
                        "whose default is 20) above X in some window of "
                        "--low-complexity-window bases; dropped candidates "
                        "make bases uncoverable as with --filter-polya")
    p.add_argument("--low-complexity-window", type=int, default=64, metavar="W",
                   help="window of --filter-low-complexity, 3..256 bases "
                        "(a shorter probe is one window)")


def from_args(args, error=_value_error):
    """A new CompositionFilter as the options of add_arguments ask for, or
    None without them; bad values go to error (ArgumentParser.error in the
    parsers, so that they are argparse errors)."""
    if args.filter_gc is not None:
        try:
            lo, hi = (_unit_fraction(x, "--filter-gc: a bound") for x in args.filter_gc)
        except ValueError as exc:
            error(str(exc))
        if lo > hi:
            error("--filter-gc: MIN (%s) exceeds MAX (%s)" % tuple(args.filter_gc))
    if args.max_homopolymer is not None and args.max_homopolymer < 1:
        error("--max-homopolymer must be at least 1, not %d" % args.max_homopolymer)
    if args.filter_low_complexity is not None and args.filter_low_complexity < 0:
        error("--filter-low-complexity must be at least 0, not %d" % args.filter_low_complexity)
    if not 3 <= args.low_complexity_window <= 256:
        error("--low-complexity-window must lie in 3..256, not %d" % args.low_complexity_window)
    if args.filter_gc is None and args.max_homopolymer is None and args.filter_low_complexity is None:
        return None
    return CompositionFilter(gc_range=args.filter_gc, max_homopolymer=args.max_homopolymer,
                             max_dust=args.filter_low_complexity,
                             dust_window=args.low_complexity_window)
