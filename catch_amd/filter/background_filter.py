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

The rule is here three times: _hits / _keeps (straight from the definition
above, a Python set of strings: the oracle of the other two), _filter_strs
(NumPy: canonical codes in uint64, np.unique and np.searchsorted) and
_apply_to_candidates (catchhip_candidates_drop_background, one kernel over the
unique candidates of the device front end, against an engine.KmerIndex built
once per device).
"""
import logging
import re
import threading

import numpy as np

from catch_amd.filter.base_filter import BaseFilter

logger = logging.getLogger(__name__)

BASES = "ACGT"
NBINS = 256
KMER_MIN, KMER_MAX, KMER_DEFAULT = 8, 32, 24
_COMPLEMENT = str.maketrans("ACGT", "TGCA")

# bytes to the 2-bit code (c >> 1) & 3 of a base; 4: not a base
_CODE = np.full(256, 4, dtype=np.uint8)
for _c in BASES:
    _CODE[ord(_c)] = (ord(_c) >> 1) & 3
_PIECE = 1 << 20          # background positions per NumPy step


def _canonical(code, k):
    """(canonical codes, valid mask) of the k-mers of every row of `code` (a
    2-d uint8 array of _CODE values, at least k columns): two arrays of
    shape (rows, columns - k + 1), uint64 and bool."""
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
    return np.minimum(fwd, rc), valid


class BackgroundFilter(BaseFilter):
    def __init__(self, background_seqs, kmer=KMER_DEFAULT, max_hits=None):
        if isinstance(kmer, bool) or not isinstance(kmer, int) or not KMER_MIN <= kmer <= KMER_MAX:
            raise ValueError("the k-mer length must be an integer in %d .. %d, not %r" % (KMER_MIN, KMER_MAX, kmer))
        if max_hits is not None and (isinstance(max_hits, bool) or not isinstance(max_hits, int) or max_hits < 0):
            raise ValueError("the number of hits allowed must be an integer >= 0, not %r" % (max_hits,))
        self.background_seqs = [str(s) for s in background_seqs]
        self.kmer, self.max_hits = kmer, max_hits
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

    def _hits(self, s):
        """hits(s); 0 if len(s) < K."""
        k, words = self.kmer, self._background_words()
        return sum(1 for j in range(len(s) - k + 1)
                   if all(c in BASES for c in s[j:j + k]) and s[j:j + k] in words)

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

    def _filter_strs(self, strs):
        strs = list(strs)
        if not strs:
            return strs
        L = len(strs[0])
        if L == 0 or any(len(s) != L for s in strs):
            return [s for s, k in zip(strs, self._keep_list(strs)) if k]
        out = []
        for a in range(0, len(strs), 1 << 14):        # (bounded temporaries)
            part = strs[a:a + (1 << 14)]
            keep = self._keep_mask_equal_length(part, L)
            out += [s for s, k in zip(part, keep.tolist()) if k]
        return out

    def _filter(self, input):
        if len(input) == 0:
            return input
        return [p for p, k in zip(input, self._keep_list([p.seq_str for p in input])) if k]

    # ------------------------------------------------------------ the device front end
    def _device_index(self, ctx):
        """The engine.KmerIndex of ctx's device: built on first use, on ctx, and
        shared by every context of that device from then on."""
        from catch_amd import engine
        with self._build_lock:
            index = self._device_indexes.get(ctx.device)
            if index is None:
                index = engine.KmerIndex(ctx, self.background_seqs, self.kmer)
                self._device_indexes[ctx.device] = index
            return index

    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        if cands.L < self.kmer:
            return
        self._count(*cands.drop_background(self._device_index(cands.ctx), self.max_hits, histogram=True))

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
    """The four options of catch_amd.design and catch_amd.design_grid."""
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


def _value_error(message):
    raise ValueError(message)


def from_args(args, error=_value_error, load=True):
    """A new BackgroundFilter as the options of add_arguments ask for, or None
    without them; bad values go to error (ArgumentParser.error in the parsers,
    so that they are argparse errors).  load = False only checks the options
    and returns None: the parsers do not read the background."""
    others = [("--background-kmer", args.background_kmer), ("--background-max-hits", args.background_max_hits),
              ("--write-background-histogram", args.write_background_histogram)]
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
    if args.background_max_hits is not None and args.background_max_hits < 0:
        error("--background-max-hits must be >= 0, not %d" % args.background_max_hits)
    probe_length = getattr(args, "probe_length", None)
    if probe_length is not None and probe_length < k:
        error("--background-kmer (%d) exceeds the probe length (%d): no candidate has a k-mer" % (k, probe_length))
    if not load:
        return None
    from catch_amd.utils import seq_io
    seqs = [s for fn in args.background for s in seq_io.read_fasta(fn).values()]
    return BackgroundFilter(seqs, kmer=k, max_hits=args.background_max_hits)
