"""Removes candidate probes by their secondary structure: a hairpin stem, a
self-dimer.  Not in the reference; the rules are defined here, in integers, and
the order of the input is kept.

A candidate is a string s of L characters.  Bytes are compared as they are:
only 'A', 'C', 'G' and 'T' are bases.  pairs(x, y), for 0 <= x, y < L, holds
iff s[x] and s[y] are bases and s[y] is the Watson-Crick complement of s[x]
(A-T, C-G); so pairs(x, x) never holds, and 'N', lower case and every other
byte pair with nothing.

Hairpin (max_hairpin_stem = K >= 1, hairpin_min_loop = P >= 0, default 3).
Dropped iff there are i < j with
    pairs(i + t, j - t) for every t in 0 .. K      (a stem of K + 1 base pairs, antiparallel)
    (j - K) - (i + K) - 1 >= P                     (at least P unpaired characters between the arms' inner ends;
                                                    this also keeps the arms from overlapping)
A candidate with L < 2 K + 2 + P is never dropped.

Self-dimer (max_self_dimer = D >= 1): two copies of s anneal antiparallel.
Dropped iff there are a, b with 0 <= a, a + D <= L - 1, b - D >= 0, b <= L - 1
and pairs(a + t, b - t) for every t in 0 .. D.  There is no relation between a
and b: the stretch may cross the middle of an antidiagonal ('ACGT' is one
stretch of 4).  Every hairpin stem is also such a stretch, so with D < K the
hairpin rule adds nothing; that is allowed.

Both rules ask for R consecutive pairs on an antidiagonal x + y = const of the
L x L table pairs(x, y), or, in words: the arm u = s[a .. a + R - 1] consists of
bases and its reverse complement is found in s, at s[b - R + 1 .. b] -- anywhere
for the self-dimer (R = D + 1), at q = j - K >= i + K + 1 + P for the hairpin
(R = K + 1, a = i).  _fails says exactly that.

A candidate is dropped iff any enabled rule drops it.  `dropped` accumulates,
over all calls, the candidates [hairpin, self-dimer, any rule] dropped --
candidates as they come out of the sliding windows, duplicates counted, and one
that fails both rules counted for both and once in "any".

The rule is here three times: _keeps (from the definitions above: the oracle of
the other two), _filter_strs (NumPy, equal-length candidates) and
_apply_to_candidates (catchhip_candidates_drop_structure, one kernel over the
unique candidates of the device front end).
"""
import threading

import numpy as np

from catch_amd.filter.candidate_rule import CandidateRuleFilter, _value_error
from catch_amd.filter.composition_filter import BASES, _int

_COMPLEMENT = str.maketrans("ACGT", "TGCA")


class StructureFilter(CandidateRuleFilter):
    CHUNK = 1 << 12               # (a chunk's L x L table is walked a diagonal at a time)

    def __init__(self, max_hairpin_stem=None, hairpin_min_loop=3, max_self_dimer=None):
        self.max_hairpin_stem = None
        if max_hairpin_stem is not None:
            self.max_hairpin_stem = _int(max_hairpin_stem, "max_hairpin_stem")
            if self.max_hairpin_stem < 1:
                raise ValueError("max_hairpin_stem must be at least 1, not %d" % self.max_hairpin_stem)
        self.hairpin_min_loop = _int(hairpin_min_loop, "hairpin_min_loop")
        if self.hairpin_min_loop < 0:
            raise ValueError("hairpin_min_loop must be at least 0, not %d" % self.hairpin_min_loop)
        self.max_self_dimer = None
        if max_self_dimer is not None:
            self.max_self_dimer = _int(max_self_dimer, "max_self_dimer")
            if self.max_self_dimer < 1:
                raise ValueError("max_self_dimer must be at least 1, not %d" % self.max_self_dimer)
        self.dropped = [0, 0, 0]         # [hairpin, self-dimer, any rule], over all calls
        self._lock = threading.Lock()    # (groups in flight are filtered on several host threads)

    def _count(self, three):
        with self._lock:
            self.dropped = [a + int(b) for a, b in zip(self.dropped, three)]

    # ------------------------------------------------------------ the definition
    def _fails(self, s):
        """(hairpin, self-dimer): which rules drop s."""
        L = len(s)
        K, P, D = self.max_hairpin_stem, self.hairpin_min_loop, self.max_self_dimer
        other = [0] * (L + 1)            # other[x] = characters of s[:x] that are no bases
        for x, c in enumerate(s):
            other[x + 1] = other[x] + (c not in BASES)

        def arm(a, R):
            """the reverse complement of s[a .. a + R - 1]: what pairs with it, read along s; None unless all are bases"""
            if other[a + R] != other[a]:
                return None
            return s[a:a + R].translate(_COMPLEMENT)[::-1]

        fails_hairpin = False
        if K is not None:
            for i in range(L - 2 * K - 1 - P):           # the right arm starts at q = j - K >= i + K + 1 + P, q + K <= L - 1
                u = arm(i, K + 1)
                if u is not None and s.find(u, i + K + 1 + P) >= 0:
                    fails_hairpin = True
                    break
        fails_dimer = False
        if D is not None:
            for a in range(L - D):
                u = arm(a, D + 1)
                if u is not None and u in s:
                    fails_dimer = True
                    break
        return fails_hairpin, fails_dimer

    def _keeps(self, s):
        return not any(self._fails(s))

    # ------------------------------------------------------------ NumPy, one length
    @staticmethod
    def _has_run(m, R):
        """m: bool (n, width); which rows hold R consecutive True.  AND-shifts that double the run in hand."""
        have = 1
        while have < R and m.shape[1] > 0:
            step = min(have, R - have)
            m = m[:, :-step] & m[:, step:]
            have += step
        return m.any(axis=1) if m.shape[1] > 0 else np.zeros(m.shape[0], dtype=bool)

    def _fail_masks_equal_length(self, strs, L):
        """_fails for strings of one length L at once: two bool arrays.  Antidiagonal by antidiagonal: the
        candidates' columns lo .. hi against the complemented columns c - lo .. c - hi."""
        n = len(strs)
        K, P, D = self.max_hairpin_stem, self.hairpin_min_loop, self.max_self_dimer
        fails_hairpin, fails_dimer = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        need = min(R for R in (None if K is None else K + 1, None if D is None else D + 1, L + 1) if R is not None)
        if need > L:
            return fails_hairpin, fails_dimer
        rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(n, L)
        partner = np.zeros(256, dtype=np.uint8)              # 0: pairs with nothing (is_base masks a byte 0 of s)
        for x, y in zip(b"ACGT", b"TGCA"):
            partner[x] = y
        wants = partner[rows][:, ::-1]                       # wants[:, L - 1 - y] = the byte that pairs with s[y]
        is_base = partner[rows] != 0
        for c in range(need - 1, 2 * (L - 1) - (need - 1) + 1):
            lo, hi = max(0, c - (L - 1)), min(L - 1, c)
            # x = lo .. hi against y = c - x: column L - 1 - y = L - 1 - c + x of wants
            m = (rows[:, lo:hi + 1] == wants[:, L - 1 - c + lo:L - c + hi]) & is_base[:, lo:hi + 1]
            if D is not None and hi - lo >= D:
                fails_dimer |= self._has_run(m, D + 1)
            if K is not None:
                inner = (c - 1 - P) // 2                     # the inner end i + K of the left arm: 2 (i + K) <= c - 1 - P
                if inner - lo >= K:
                    fails_hairpin |= self._has_run(m[:, :inner - lo + 1], K + 1)
        return fails_hairpin, fails_dimer

    def _keep_mask_equal_length(self, strs, L):
        """_keeps for strings of one length L at once (candidate probes); counts what it drops."""
        fails = self._fail_masks_equal_length(strs, L)
        drop = fails[0] | fails[1]
        self._count([int(f.sum()) for f in fails] + [int(drop.sum())])
        return ~drop

    def _keep_list(self, strs):
        """_keeps string by string; counts what it drops."""
        fails = [self._fails(s) for s in strs]
        self._count([sum(f[k] for f in fails) for k in range(2)] + [sum(any(f) for f in fails)])
        return [not any(f) for f in fails]

    # ------------------------------------------------------------ the device front end
    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        big = 2 ** 31 - 1
        self._count(cands.drop_structure(
            -1 if self.max_hairpin_stem is None else min(self.max_hairpin_stem, big),
            min(self.hairpin_min_loop, big),
            -1 if self.max_self_dimer is None else min(self.max_self_dimer, big)))


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The three options of catch_amd.design and catch_amd.design_grid."""
    p.add_argument("--max-hairpin-stem", type=int, metavar="K",
                   help="drop candidate probes that can fold into a hairpin "
                        "with a stem of more than K base pairs (A-T, C-G, "
                        "antiparallel, no mismatch or bulge) around a loop "
                        "of at least --hairpin-min-loop characters; N pairs "
                        "with nothing; a random 100-mer holds a 6-pair stem "
                        "more often than not, so useful values are near 8 "
                        "to 12; like --filter-polya this comes before the "
                        "set cover, so bases that only dropped candidates "
                        "would cover become uncoverable and -c refers to "
                        "what is left")
    p.add_argument("--hairpin-min-loop", type=int, default=None, metavar="P",
                   help="least number of unpaired characters between the two "
                        "arms of a --max-hairpin-stem stem, and of the stems "
                        "--write-candidate-profile measures (default 3)")
    p.add_argument("--max-self-dimer", type=int, metavar="D",
                   help="drop candidate probes of which two copies can "
                        "anneal over more than D consecutive base pairs "
                        "(antiparallel, no mismatch; every hairpin stem is "
                        "such a stretch too, so D below K makes "
                        "--max-hairpin-stem idle); dropped candidates make "
                        "bases uncoverable as with --filter-polya")


def from_args(args, error=_value_error):
    """A new StructureFilter as the options of add_arguments ask for, or None
    without them; bad values go to error (ArgumentParser.error in the parsers,
    so that they are argparse errors)."""
    if args.max_hairpin_stem is not None and args.max_hairpin_stem < 1:
        error("--max-hairpin-stem must be at least 1, not %d" % args.max_hairpin_stem)
    if args.hairpin_min_loop is not None:
        if args.max_hairpin_stem is None and getattr(args, "write_candidate_profile", None) is None:
            error("--hairpin-min-loop needs --max-hairpin-stem")
        if args.hairpin_min_loop < 0:
            error("--hairpin-min-loop must be at least 0, not %d" % args.hairpin_min_loop)
    if args.max_self_dimer is not None and args.max_self_dimer < 1:
        error("--max-self-dimer must be at least 1, not %d" % args.max_self_dimer)
    if args.max_hairpin_stem is None and args.max_self_dimer is None:
        return None
    return StructureFilter(max_hairpin_stem=args.max_hairpin_stem,
                           hairpin_min_loop=3 if args.hairpin_min_loop is None else args.hairpin_min_loop,
                           max_self_dimer=args.max_self_dimer)
