"""Removes candidate probes that share k-mers with a background -- sequences
that are in the tube but are no target: a host genome, rRNA, a vector backbone,
a spike-in -- and measures how many k-mers the candidates share with it.  Not
in the reference; the rule is defined here, in integers, and the order of the
input is kept.

Background: a list of records (strings).  Only 'A', 'C', 'G' and 'T' are bases
(the command line reads the records with seq_io.read_fasta, which upper-cases
them and turns degenerate codes into 'N', so soft-masked FASTAs work).  A k-mer
-- K consecutive characters, 8 <= K <= 32 -- is VALID iff all K are bases; the
k-mers of the background lie inside one record each, never across two.

Hits: a k-mer w HITS iff w or its reverse complement is a valid k-mer of some
background record.  For a candidate s of L characters, bytes compared as they
are (lower case is no base),
    hits(s) = the number of positions j in 0 .. L - K whose k-mer s[j:j+K] is
              valid and hits.
With L < K there is no position: 0 hits, nothing dropped, nothing counted.

Filter (max_hits = H >= 0): a candidate is dropped iff hits(s) > H.  H = None
measures only and drops nothing.  A shared exact stretch of K + h bases yields
h + 1 hits: that is the handle H gives.

Histogram: 256 bins, bin min(hits, 255); every candidate the filter sees is
counted, duplicates too, before the rule drops anything.  `histogram` and
`dropped` accumulate over all calls.

Choosing K: a random position hits a background of G bases with probability
about 2 G / 4^K -- for a host of 3.1 Gbp about 0.6 % per position at K = 20
and about 2e-5 at K = 24, the default.

Code of a k-mer (the NumPy path and the kernel; the definition needs none): 2
bits per character, (c >> 1) & 3 of the byte -- A 0, C 1, T 2, G 3 -- the first
character in the most significant of the 2K bits of a 64-bit word; the
complement of a code is code ^ 2; canonical(w) = the smaller of code(w) and
code(revcomp(w)) as unsigned integers.  w hits iff canonical(w) is among the
canonical codes of the background's valid k-mers.

Mismatches (mismatches = M in 0 .. 2, default 0; K >= 8 (M + 1)): a valid k-mer
w of a candidate hits iff some valid background k-mer v has Hamming(w, v) <= M
or Hamming(w, revcomp(v)) <= M.  Validity is what it was -- 'N' is no wildcard,
a k-mer that holds one neither hits nor is hit -- and so are hits(s), the drop
rule, the histogram and the counting; hits(s) never falls when M rises.  M = 0
is the rule above, computed by the code that computed it before M existed.
Choosing K and M: a random position now hits with probability about
2 G N(K, M) / 4^K, N(K, M) = sum over i <= M of C(K, i) 3^i (N(24, 1) = 73,
N(32, 1) = 97, N(32, 2) = 4,561): against 3.1 Gbp 1.6e-3 at K = 24, M = 1 --
no longer specific -- but 3.3e-8 at K = 32, M = 1 and 1.5e-6 at K = 32, M = 2,
which find a 90 % identical stretch 16 % and 37 % of the time per position
where the exact 24-mer finds it 8 %.

Finding them (NumPy and the kernel): block b = 0 .. M of a k-mer is its
characters [s_b, s_(b+1)), s_b = floor(b K / (M + 1)), each 8 characters at
least; two k-mers at most M mismatches apart agree exactly in one block.  VIEW
b is the list of canonical codes, each rotated left by 2 s_b bits inside its
2K bits, so that block b leads, sorted again (a rotation is a bijection: the
list stays distinct).  Since d(w, revcomp(v)) = d(revcomp(w), v) the canonical
list is enough: code(w) and code(revcomp(w)) are each rotated like view b, the
entries of the view that agree with the query in block b are one sorted range,
and the position hits at the first entry within distance M,
popcount(((x ^ c) | ((x ^ c) >> 1)) & 0x5555555555555555) of two codes rotated
alike.

The rule is here three times: _hits / _keeps (straight from the definition
above, a Python set of strings and, with M > 0, Hamming distances to each of
them: the oracle of the other two), _filter_strs (NumPy: canonical codes in
uint64, np.unique and np.searchsorted; with M > 0 the views, np.searchsorted
for a block's range and a loop over the position inside the ranges) and
_apply_to_candidates (catchhip_candidates_drop_background, one kernel over the
unique candidates of the device front end, against an engine.KmerIndex built
once per device, which carries M).
"""
import logging
import operator
import re
import threading

import numpy as np

from catch_amd.filter.candidate_rule import CandidateRuleFilter, _value_error

logger = logging.getLogger(__name__)

BASES = "ACGT"
NBINS = 256
KMER_MIN, KMER_MAX, KMER_DEFAULT = 8, 32, 24
MISMATCHES_MAX, BLOCK_MIN = 2, 8          # K >= BLOCK_MIN * (M + 1)
_COMPLEMENT = str.maketrans("ACGT", "TGCA")

# bytes to the 2-bit code (c >> 1) & 3 of a base; 4: not a base
_CODE = np.full(256, 4, dtype=np.uint8)
for _c in BASES:
    _CODE[ord(_c)] = (ord(_c) >> 1) & 3
_PIECE = 1 << 20          # background positions per NumPy step


def _both_codes(code, k):
    """(code of the k-mer, code of its reverse complement, valid mask) for the
    k-mers of every row of `code` (a 2-d uint8 array of _CODE values, at least
    k columns): three arrays of shape (rows, columns - k + 1), uint64, uint64
    and bool."""
    n, L = code.shape
    W = L - k + 1
    nonbase = np.zeros((n, L + 1), dtype=np.int32)
    np.cumsum(code == 4, axis=1, out=nonbase[:, 1:])
    valid = (nonbase[:, k:] - nonbase[:, :W]) == 0
    c = (code & 3).astype(np.uint64)
    fwd = np.zeros((n, W), dtype=np.uint64)
    rc = np.zeros((n, W), dtype=np.uint64)
    two = np.uint64(2)
    for t in range(k):
        # (uint64 shifts drop what leaves the word: at k = 32 the first character ends in the top two bits)
        fwd = (fwd << two) | c[:, t:t + W]
        rc |= (c[:, t:t + W] ^ two) << np.uint64(2 * t)
    return fwd, rc, valid


def _canonical(code, k):
    """(canonical codes, valid mask) of the same k-mers."""
    fwd, rc, valid = _both_codes(code, k)
    return np.minimum(fwd, rc), valid


def block_starts(k, mismatches):
    """s_0 .. s_(M+1): block b holds the characters [s_b, s_(b+1))."""
    return [b * k // (mismatches + 1) for b in range(mismatches + 2)]


def _rotate(x, bits, k):
    """uint64 codes rotated left by `bits` (0 <= bits < 2k) inside their 2k bits."""
    if bits == 0:
        return x
    mask = np.uint64((1 << (2 * k)) - 1)
    return ((x << np.uint64(bits)) | (x >> np.uint64(2 * k - bits))) & mask


def _distance(x, c):
    """Characters in which uint64 codes differ (rotated alike or not at all)."""
    d = x ^ c
    d = (d | (d >> np.uint64(1))) & np.uint64(0x5555555555555555)
    d = (d & np.uint64(0x3333333333333333)) + ((d >> np.uint64(2)) & np.uint64(0x3333333333333333))
    d = (d + (d >> np.uint64(4))) & np.uint64(0x0f0f0f0f0f0f0f0f)
    return (d * np.uint64(0x0101010101010101)) >> np.uint64(56)


class BackgroundFilter(CandidateRuleFilter):
    def __init__(self, background_seqs, kmer=KMER_DEFAULT, max_hits=None, mismatches=0):
        if isinstance(kmer, bool) or not isinstance(kmer, int) or not KMER_MIN <= kmer <= KMER_MAX:
            raise ValueError("the k-mer length must be an integer in %d .. %d, not %r" % (KMER_MIN, KMER_MAX, kmer))
        if max_hits is not None and (isinstance(max_hits, bool) or not isinstance(max_hits, int) or max_hits < 0):
            raise ValueError("the number of hits allowed must be an integer >= 0, not %r" % (max_hits,))
        if isinstance(mismatches, bool) or not isinstance(mismatches, int) or not 0 <= mismatches <= MISMATCHES_MAX:
            raise ValueError("the mismatches allowed in a background k-mer must be an integer in 0 .. %d, not %r"
                             % (MISMATCHES_MAX, mismatches))
        if kmer < BLOCK_MIN * (mismatches + 1):
            raise ValueError("%d mismatches need a k-mer length of at least %d, not %d"
                             % (mismatches, BLOCK_MIN * (mismatches + 1), kmer))
        self.background_seqs = [str(s) for s in background_seqs]
        self.kmer, self.max_hits, self.mismatches = kmer, max_hits, mismatches
        self.background_bases = sum(s.count(c) for s in self.background_seqs for c in BASES)
        run = re.compile("[ACGT]{%d}" % kmer)
        if not any(run.search(s) for s in self.background_seqs):
            logger.warning("The background has no valid %d-mer (%d bases in %d records): the background filter "
                           "drops nothing", kmer, self.background_bases, len(self.background_seqs))
        self.dropped = 0                      # candidates dropped, over all calls
        self.histogram = [0] * NBINS          # candidates per min(hits, 255), over all calls
        self._lock = threading.Lock()         # (groups in flight are filtered on several host threads)
        self._build_lock = threading.Lock()   # the lazily built forms of the background: one builder at a time
        self._words = None                    # the definition's set of strings
        self._codes = None                    # NumPy: sorted distinct canonical codes
        self._views = None                    # NumPy, mismatches > 0: [(rotation in bits, rest bits, sorted rotated codes)]
        self._device_indexes = {}             # device number -> engine.KmerIndex

    def _count(self, dropped, hist):
        with self._lock:
            self.dropped += int(dropped)
            if hist is not None:
                self.histogram = [a + int(b) for a, b in zip(self.histogram, hist)]

    # ------------------------------------------------------------ the definition
    def _background_words(self):
        with self._build_lock:
            if self._words is None:
                k, words = self.kmer, set()
                for s in self.background_seqs:
                    for j in range(len(s) - k + 1):
                        w = s[j:j + k]
                        if all(c in BASES for c in w):
                            words.add(w)
                            words.add(w.translate(_COMPLEMENT)[::-1])
                self._words = words
            return self._words

    def _hits(self, s, mismatches=None):
        """hits(s); 0 if len(s) < K.  mismatches: another M than the filter's
        (the definition needs no blocks, so any M >= 0 goes with any K)."""
        k, words, m = self.kmer, self._background_words(), self.mismatches if mismatches is None else mismatches
        if m == 0:
            return sum(1 for j in range(len(s) - k + 1)
                       if all(c in BASES for c in s[j:j + k]) and s[j:j + k] in words)
        return sum(1 for j in range(len(s) - k + 1)
                   if all(c in BASES for c in s[j:j + k])
                   and any(sum(map(operator.ne, s[j:j + k], v)) <= m for v in words))

    def _keeps(self, s):
        return self.max_hits is None or self._hits(s) <= self.max_hits

    # ------------------------------------------------------------ NumPy
    def _background_codes(self):
        """The sorted distinct canonical codes of the background's valid k-mers (uint64)."""
        with self._build_lock:
            if self._codes is None:
                k, parts = self.kmer, []
                for s in self.background_seqs:
                    if len(s) < k:
                        continue
                    code = _CODE[np.frombuffer(s.encode("latin-1", "replace"), dtype=np.uint8)]
                    for a in range(0, len(s) - k + 1, _PIECE):         # (bounded temporaries)
                        canon, valid = _canonical(code[None, a:a + _PIECE + k - 1], k)
                        parts.append(np.unique(canon[valid]))
                self._codes = (np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint64))
            return self._codes

    def _background_views(self):
        """mismatches > 0: per view b = 0 .. M (rotation in bits, bits behind
        block b, the codes rotated and sorted again)."""
        codes, k = self._background_codes(), self.kmer
        with self._build_lock:
            if self._views is None:
                starts = block_starts(k, self.mismatches)
                self._views = [(2 * starts[b], 2 * (k - (starts[b + 1] - starts[b])), np.sort(_rotate(codes, 2 * starts[b], k)))
                               for b in range(self.mismatches + 1)]
            return self._views

    def _hits_tolerant(self, rows):
        """hits within self.mismatches for the byte rows (n, L), L >= K."""
        k, m = self.kmer, self.mismatches
        fwd, rc, valid = _both_codes(_CODE[rows], k)
        hit = np.zeros(fwd.shape, dtype=bool)
        where = np.nonzero(valid)
        if self._background_codes().size and where[0].size:
            f, r = fwd[where], rc[where]
            found = np.zeros(f.size, dtype=bool)
            for query in (f, r):
                for rot, rest, view in self._background_views():
                    q = _rotate(query, rot, k)
                    base = (q >> np.uint64(rest)) << np.uint64(rest)      # block b, zeros behind it
                    lo = np.searchsorted(view, base, side="left")
                    hi = np.searchsorted(view, base | np.uint64((1 << rest) - 1), side="right")
                    todo = np.nonzero((lo < hi) & ~found)[0]
                    t = 0
                    while todo.size:                                      # entry t of every range that is that long
                        near = _distance(q[todo], view[lo[todo] + t]) <= np.uint64(m)
                        found[todo[near]] = True
                        t += 1
                        todo = todo[~near]
                        todo = todo[lo[todo] + t < hi[todo]]
            hit[where] = found
        return hit.sum(axis=1).astype(np.int64)

    def distinct_kmers(self):
        """Distinct canonical k-mers of the background, from whichever index was built (the NumPy one otherwise)."""
        with self._build_lock:
            if self._codes is None and self._device_indexes:
                return next(iter(self._device_indexes.values())).n_unique
        return int(self._background_codes().size)

    def _hits_equal_length(self, strs, L):
        """hits for strings of one length L >= K at once: an int64 array."""
        codes, k = self._background_codes(), self.kmer
        rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(len(strs), L)
        if self.mismatches:
            return self._hits_tolerant(rows)
        canon, valid = _canonical(_CODE[rows], k)
        if codes.size == 0:
            return np.zeros(len(strs), dtype=np.int64)
        at = np.minimum(np.searchsorted(codes, canon), codes.size - 1)
        return ((codes[at] == canon) & valid).sum(axis=1).astype(np.int64)

    def _measure(self, hits):
        """(keep mask, dropped, histogram) of an int64 array of hits."""
        hist = np.bincount(np.minimum(hits, NBINS - 1), minlength=NBINS)
        if self.max_hits is None:
            return np.ones(len(hits), dtype=bool), 0, hist
        keep = hits <= self.max_hits
        return keep, int((~keep).sum()), hist

    def _keep_mask_equal_length(self, strs, L):
        """_keeps for strings of one length L at once (candidate probes); counts them and what it drops."""
        if L < self.kmer:
            return np.ones(len(strs), dtype=bool)
        keep, dropped, hist = self._measure(self._hits_equal_length(strs, L))
        self._count(dropped, hist)
        return keep

    def _keep_list(self, strs):
        """The same for strings of any lengths: length by length, the order kept."""
        keep = [True] * len(strs)
        by_length = {}
        for i, s in enumerate(strs):
            by_length.setdefault(len(s), []).append(i)
        for L, where in by_length.items():
            for a in range(0, len(where), 1 << 14):
                part = where[a:a + (1 << 14)]
                for i, k in zip(part, self._keep_mask_equal_length([strs[i] for i in part], L).tolist()):
                    keep[i] = k
        return keep

    # ------------------------------------------------------------ the device front end
    def _device_index(self, ctx):
        """The engine.KmerIndex of ctx's device: built on first use, on ctx, and
        shared by every context of that device from then on."""
        from catch_amd import engine
        with self._build_lock:
            index = self._device_indexes.get(ctx.device)
            if index is None:
                index = engine.KmerIndex(ctx, self.background_seqs, self.kmer, mismatches=self.mismatches)
                self._device_indexes[ctx.device] = index
            return index

    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        if cands.L < self.kmer:
            return
        self._count(*cands.drop_background(self._device_index(cands.ctx), self.max_hits, histogram=True))

    def summary(self):
        """The line --verbose logs behind a design."""
        return ("background filter: %d candidates dropped; %d background bases, %d distinct k-mers"
                % (self.dropped, self.background_bases, self.distinct_kmers())
                + (" matched within %d mismatches" % self.mismatches if self.mismatches else ""))

    def close(self):
        """Frees the device indexes (they are built again on the next use)."""
        with self._build_lock:
            indexes, self._device_indexes = self._device_indexes, {}
        for index in indexes.values():
            index.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ the histogram file
    def write_histogram(self, path):
        """hits <tab> candidates, one row per hit count from 0 to the highest
        non-empty bin (empty bins below it included); bin 255 holds everything
        from 255 hits up."""
        with self._lock:
            hist = list(self.histogram)
        filled = [b for b, v in enumerate(hist) if v]
        with open(path, "w") as f:
            f.write("hits\tcandidates\n")
            if filled:
                for b in range(filled[-1] + 1):
                    f.write("%d\t%d\n" % (b, hist[b]))


# ---------------------------------------------------------------- command line
def add_arguments(p):
    """The five options of catch_amd.design and catch_amd.design_grid."""
    p.add_argument("--background", nargs="+", metavar="FASTA",
                   help="sequences the probes must not match (a host genome, "
                        "rRNA, a vector backbone, a spike-in): candidate "
                        "probes are screened against the k-mers of these "
                        "files, both strands (catch_amd/filter/"
                        "background_filter.py has the rule); needs "
                        "--background-max-hits or "
                        "--write-background-histogram")
    p.add_argument("--background-kmer", type=int, metavar="K",
                   help="k-mer length of the background screen, 8 to 32 "
                        "(default 24: a random position hits a background of G "
                        "bases with probability about 2 G / 4^K, 2e-5 for a "
                        "host of 3.1 Gbp)")
    p.add_argument("--background-mismatches", type=int, metavar="M",
                   help="count a k-mer of a candidate as shared when a k-mer "
                        "of the background, either strand, lies within M "
                        "substitutions of it: 0 (the default, exact k-mers), 1 "
                        "or 2, with K >= 8 (M + 1); a random position then "
                        "hits with probability about 2 G N / 4^K, N = 97 for "
                        "K = 32, M = 1 and 4,561 for K = 32, M = 2 (3e-8 and "
                        "1.5e-6 for a host of 3.1 Gbp), so raise "
                        "--background-kmer to 32 with it: at K = 24, M = 1 "
                        "it is 1.6e-3")
    p.add_argument("--background-max-hits", type=int, metavar="H",
                   help="drop candidate probes that share more than H k-mers "
                        "with the background (an exact shared stretch of K + h "
                        "bases is h + 1 hits; 0 drops every candidate that "
                        "shares one k-mer); like --filter-polya this comes "
                        "before the set cover, so bases that only dropped "
                        "candidates would cover become uncoverable and -c "
                        "refers to what is left")
    p.add_argument("--write-background-histogram", metavar="FILE",
                   help="write the number of candidate probes per hit count "
                        "to FILE as a TSV (hits, candidates), rows 0 to the "
                        "highest count met (255 and more in one row): the "
                        "candidates that survive the filters before this one, "
                        "duplicates counted, before --background-max-hits "
                        "drops any and over all datasets; without "
                        "--background-max-hits it only measures and the "
                        "design is unchanged")


def from_args(args, error=_value_error, load=True):
    """A new BackgroundFilter as the options of add_arguments ask for, or None
    without them; bad values go to error (ArgumentParser.error in the parsers,
    so that they are argparse errors).  load = False only checks the options
    and returns None: the parsers do not read the background."""
    others = [("--background-kmer", args.background_kmer), ("--background-max-hits", args.background_max_hits),
              ("--write-background-histogram", args.write_background_histogram),
              ("--background-mismatches", getattr(args, "background_mismatches", None))]
    if args.background is None:
        for name, value in others:
            if value is not None:
                error("%s needs --background" % name)
        return None
    if args.background_max_hits is None and args.write_background_histogram is None:
        error("--background needs --background-max-hits or --write-background-histogram")
    k = KMER_DEFAULT if args.background_kmer is None else args.background_kmer
    if not KMER_MIN <= k <= KMER_MAX:
        error("--background-kmer must lie in %d .. %d, not %d" % (KMER_MIN, KMER_MAX, k))
    m = getattr(args, "background_mismatches", None) or 0
    if not 0 <= m <= MISMATCHES_MAX:
        error("--background-mismatches must lie in 0 .. %d, not %d" % (MISMATCHES_MAX, m))
    if k < BLOCK_MIN * (m + 1):
        error("--background-mismatches %d needs --background-kmer >= %d, not %d" % (m, BLOCK_MIN * (m + 1), k))
    if args.background_max_hits is not None and args.background_max_hits < 0:
        error("--background-max-hits must be >= 0, not %d" % args.background_max_hits)
    probe_length = getattr(args, "probe_length", None)
    if probe_length is not None and probe_length < k:
        error("--background-kmer (%d) exceeds the probe length (%d): no candidate has a k-mer" % (k, probe_length))
    if not load:
        return None
    from catch_amd.utils import seq_io
    seqs = [s for fn in args.background for s in seq_io.read_fasta(fn).values()]
    return BackgroundFilter(seqs, kmer=k, max_hits=args.background_max_hits, mismatches=m)
