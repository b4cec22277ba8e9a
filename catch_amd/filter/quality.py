"""Measures candidate probes instead of judging them: the value behind every
composition and structure rule.  Not in the reference; the quantities are
defined here, in integers, and nothing is ever dropped.

A candidate is a string s of L characters.  Bytes are compared as they are:
only 'A', 'C', 'G' and 'T' are bases.  pairs(x, y) is as in
structure_filter.py, P = min_loop (--hairpin-min-loop) and W = dust_window
(--low-complexity-window) as in the two filters.

    gc           the number of 'G' or 'C';
                 --filter-gc keeps s iff ceil(MIN L) <= gc <= floor(MAX L)
    homopolymer  the longest run of one identical base, 0 without a base;
                 --max-homopolymer H drops s iff homopolymer > H
    dust         the smallest integer X at which the low-complexity rule keeps
                 s: the maximum of ceil(10 S / (T - 1)) over the windows with
                 T >= 2 (composition_filter.py has S and T), 0 if there is
                 none or L < 3; --filter-low-complexity X drops s iff dust > X.
                 It rounds UP: (AC)32 has 10 S / (T - 1) = 9300 / 61 = 152.46,
                 is dropped at X = 152 and kept at 153.  dust <= 5 T <= 1270.
    stem         the largest n for which there are i < j with
                 pairs(i + t, j - t) for t in 0 .. n - 1 and
                 (j - n + 1) - (i + n - 1) - 1 >= P, 0 if none;
                 --max-hairpin-stem K drops s iff stem > K
    dimer        the largest n for which there are a, b with
                 pairs(a + t, b - t) for t in 0 .. n - 1, every index inside
                 0 .. L - 1, 0 if none; --max-self-dimer D drops s iff dimer > D

The measure is here three times: measure (from the quantifiers above: the
oracle of the other two), measure_equal_length / measure_many (NumPy) and
engine.Candidates.measure (catchhip_candidates_measure, over the unique
candidates of the device front end).

QualityProfile is the filter that only looks: five histograms of 1,280 bins,
bin min(value, 1279), over every candidate it sees, duplicates counted.  dust
always fits; gc, homopolymer, stem and dimer of probes longer than 1,279
characters share the last bin.
"""
import threading

import numpy as np

from catch_amd.filter.base_filter import BaseFilter
from catch_amd.filter.composition_filter import BASES, _int

QUANTITIES = ("gc", "homopolymer", "dust", "stem", "dimer")
NBINS = 1280
_PARTNER = {"A": "T", "C": "G", "G": "C", "T": "A"}
_CHUNK_CELLS = 1 << 22       # characters of one NumPy step of measure_many


def _check(min_loop, dust_window):
    P, W = _int(min_loop, "min_loop"), _int(dust_window, "dust_window")
    if P < 0:
        raise ValueError("min_loop must be at least 0, not %d" % P)
    if not 3 <= W <= 256:
        raise ValueError("dust_window must lie in 3..256, not %d" % W)
    return P, W


# ---------------------------------------------------------------- the definition
def measure(s, min_loop=3, dust_window=64):
    """(gc, homopolymer, dust, stem, dimer) of the string s."""
    P, W = _check(min_loop, dust_window)
    L = len(s)
    gc = sum(1 for c in s if c in "GC")
    homopolymer = run = 0
    for j, c in enumerate(s):
        run = 0 if c not in BASES else run + 1 if j > 0 and s[j - 1] == c else 1
        homopolymer = max(homopolymer, run)
    dust = 0
    if L >= 3:
        We = min(W, L)
        for i in range(L - We + 1):
            counts = {}
            for j in range(i, i + We - 2):
                t = s[j:j + 3]
                if all(c in BASES for c in t):
                    counts[t] = counts.get(t, 0) + 1
            T = sum(counts.values())
            S = sum(c * (c - 1) // 2 for c in counts.values())
            if T >= 2:
                dust = max(dust, -((-10 * S) // (T - 1)))
    stem = dimer = 0
    for a in range(L):
        for b in range(L):
            n = 0
            while a + n <= L - 1 and b - n >= 0 and _PARTNER.get(s[a + n]) == s[b - n]:
                n += 1
            dimer = max(dimer, n)
            # the first n' of these pairs are a stem iff (b - n' + 1) - (a + n' - 1) - 1 >= P
            if a < b:
                stem = max(stem, min(n, (b - a + 1 - P) // 2))
    return gc, homopolymer, dust, stem, dimer


# ---------------------------------------------------------------- NumPy, one length
def measure_equal_length(strs, L, min_loop=3, dust_window=64, composition=True, structure=True):
    """measure for strings of one length L >= 1 at once: an int64 array of
    shape (len(strs), 5), the columns in the order of QUANTITIES; the columns
    of a family that is switched off stay 0."""
    P, W = _check(min_loop, dust_window)
    n = len(strs)
    out = np.zeros((n, 5), dtype=np.int64)
    rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(n, L)
    digit = np.full(256, -1, dtype=np.int32)
    digit[np.frombuffer(BASES.encode(), dtype=np.uint8)] = np.arange(4)
    d = digit[rows]
    base = d >= 0
    if composition:
        out[:, 0] = ((rows == ord("G")) | (rows == ord("C"))).sum(axis=1)
        # homopolymer: a run goes on where a base follows itself; its length = distance to the last column where none did
        idx = np.arange(L, dtype=np.int32)
        goes_on = np.zeros((n, L), dtype=bool)
        goes_on[:, 1:] = (rows[:, 1:] == rows[:, :-1]) & base[:, 1:]
        start = np.maximum.accumulate(np.where(goes_on, 0, idx[None, :]), axis=1)
        out[:, 1] = np.where(base, idx[None, :] - start + 1, 0).max(axis=1)
    if composition and L >= 4:                    # (a window of 3 characters holds one triplet: T < 2)
        We = min(W, L)
        code = 16 * d[:, :L - 2] + 4 * d[:, 1:L - 1] + d[:, 2:]
        code[~(base[:, :L - 2] & base[:, 1:L - 1] & base[:, 2:])] = -1
        ntrip, width = L - 2, We - 2              # triplets of a candidate, of a window
        S = np.zeros((n, ntrip - width + 1), dtype=np.int64)
        T = np.zeros_like(S)
        cs = np.zeros((n, ntrip + 1), dtype=np.int32)
        for t in range(64):
            np.cumsum(code == t, axis=1, out=cs[:, 1:])
            c = cs[:, width:] - cs[:, :ntrip + 1 - width]
            S += c * (c - 1) // 2
            T += c
        score = np.where(T >= 2, -((-10 * S) // np.maximum(T - 1, 1)), 0)
        out[:, 2] = score.max(axis=1)
    # stem and dimer: run[y] = the pairs that end at cell (x, y), walking x up and y down, row x from row x - 1:
    # run_x[y] = pairs(x, y) ? run_(x-1)[y + 1] + 1 : 0.  dimer is the largest of them; a run that ends at (x, y) with
    # y - x - 1 >= P is a stem with all its cells (they have smaller x and larger y), so stem is the largest of those.
    if not structure:
        return out
    partner = np.full(4, -2, dtype=np.int32)
    partner[[0, 1, 2, 3]] = [3, 2, 1, 0]          # digits of 'A', 'C', 'G', 'T'
    wants = np.where(base, partner[np.maximum(d, 0)], -2)
    run = np.zeros((n, L + 1), dtype=np.int32)     # (a zero behind the last column: y + 1 = L)
    for x in range(L):
        m = wants == d[:, x:x + 1]
        run[:, :L] = (run[:, 1:] + 1) * m
        np.maximum(out[:, 4], run[:, :L].max(axis=1), out=out[:, 4])
        if x + 1 + P < L:
            np.maximum(out[:, 3], run[:, x + 1 + P:L].max(axis=1), out=out[:, 3])
    return out


def measure_many(strs, min_loop=3, dust_window=64):
    """measure for strings of any lengths: an int64 array (len(strs), 5), in
    the order of the input; length by length, in chunks (bounded temporaries)."""
    strs = list(strs)
    out = np.zeros((len(strs), 5), dtype=np.int64)
    by_length = {}
    for i, s in enumerate(strs):
        by_length.setdefault(len(s), []).append(i)
    for L, where in by_length.items():
        if L == 0:
            continue
        # (a chunk's L x L table is walked a row at a time: L + 1 ints per string at once, and 64 window sums)
        step = max(1, _CHUNK_CELLS // (L + 1))
        for a in range(0, len(where), step):
            part = where[a:a + step]
            out[part] = measure_equal_length([strs[i] for i in part], L, min_loop, dust_window)
    return out


def histograms_of(values, weights=None):
    """The five histograms (a (5, NBINS) int64 array) of an (n, 5) array of values."""
    values = np.asarray(values).reshape(-1, 5)
    h = np.zeros((5, NBINS), dtype=np.int64)
    for q in range(5):
        b = np.bincount(np.minimum(values[:, q], NBINS - 1), weights=weights, minlength=NBINS)
        h[q] = np.rint(b).astype(np.int64) if weights is not None else b
    return h


class QualityProfile(BaseFilter):
    def __init__(self, min_loop=3, dust_window=64):
        self.min_loop, self.dust_window = _check(min_loop, dust_window)
        self.histograms = np.zeros((5, NBINS), dtype=np.int64)     # per quantity, over all calls
        self._lock = threading.Lock()    # (groups in flight are measured on several host threads)

    def _count(self, hists):
        with self._lock:
            self.histograms += np.asarray(hists, dtype=np.int64).reshape(5, NBINS)

    def _filter_strs(self, strs):
        strs = list(strs)
        if strs:
            self._count(histograms_of(measure_many(strs, self.min_loop, self.dust_window)))
        return strs

    def _filter(self, input):
        if len(input) > 0:
            self._filter_strs([p.seq_str for p in input])
        return input

    # ------------------------------------------------------------ the device front end
    def _apply_to_candidates(self, cands):
        """The measure on an engine.Candidates object (grouped or not), before
        any near-duplicate filter; the list stays as it is."""
        got = cands.measure(what=("composition", "structure"), min_loop=self.min_loop,
                            dust_window=self.dust_window, values=False, histograms=True)
        self._count([got["histograms"][q] for q in QUANTITIES])

    # ------------------------------------------------------------ what was seen
    def medians(self):
        """{quantity: lower median of the candidates seen, None if none}."""
        with self._lock:
            hists = self.histograms.copy()
        out = {}
        for name, h in zip(QUANTITIES, hists):
            total = int(h.sum())
            out[name] = int(np.searchsorted(np.cumsum(h), (total + 1) // 2)) if total else None
        return out

    def write_profile(self, path):
        """quantity <tab> value <tab> candidates <tab> candidates_above, the
        quantities in the order of QUANTITIES, one row per value from the
        lowest non-empty bin to the highest (empty ones between them
        included); candidates_above = the candidates with a larger value, which
        is what a threshold at `value` would drop.  Value 1279 holds
        everything from 1279 up."""
        with self._lock:
            hists = self.histograms.copy()
        with open(path, "w") as f:
            f.write("quantity\tvalue\tcandidates\tcandidates_above\n")
            for name, h in zip(QUANTITIES, hists):
                filled = np.flatnonzero(h)
                if filled.size == 0:
                    continue
                above = int(h.sum())
                for b in range(int(filled[0]), int(filled[-1]) + 1):
                    above -= int(h[b])
                    f.write("%s\t%d\t%d\t%d\n" % (name, b, int(h[b]), above))


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The option of catch_amd.design and catch_amd.design_grid."""
    p.add_argument("--write-candidate-profile", metavar="FILE",
                   help="write what the candidate probes are like to FILE as "
                        "a TSV (quantity, value, candidates, "
                        "candidates_above) over gc, homopolymer, dust, stem "
                        "and dimer -- the values behind --filter-gc, "
                        "--max-homopolymer, --filter-low-complexity, "
                        "--max-hairpin-stem and --max-self-dimer (catch_amd/"
                        "filter/quality.py has the definitions): the "
                        "candidates that survive --filter-from-fasta and "
                        "--filter-polya, duplicates counted, before any other "
                        "filter drops one and over all datasets; "
                        "candidates_above is what a threshold at that value "
                        "would drop; --hairpin-min-loop and "
                        "--low-complexity-window set the loop and the window "
                        "measured with; it only measures, the design is "
                        "unchanged")


def from_args(args):
    """A new QualityProfile if --write-candidate-profile is given, else None
    (the loop and the window were checked by the two filters' from_args)."""
    if getattr(args, "write_candidate_profile", None) is None:
        return None
    return QualityProfile(min_loop=3 if args.hairpin_min_loop is None else args.hairpin_min_loop,
                          dust_window=args.low_complexity_window)


def finish(profile, args, logger):
    """After the design: the file, and the medians for --verbose."""
    profile.write_profile(args.write_candidate_profile)
    med = profile.medians()
    if med["gc"] is not None:
        logger.info("candidate profile: %d candidates; medians: %s", int(profile.histograms[0].sum()),
                    ", ".join("%s %d" % (name, med[name]) for name in QUANTITIES))
