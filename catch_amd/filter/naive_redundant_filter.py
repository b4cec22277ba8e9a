"""Naive redundant filter and its two redundancy predicates (mirrors
catch/filter/naive_redundant_filter.py: NaiveRedundantFilter :26-77,
redundant_shift_and_mismatch_count :80-143,
redundant_longest_common_substring :146-215).

The reference walks the probes in order and, for each probe it has kept, drops
every later probe that a pairwise predicate deems redundant to it -- all pairs
in Python.  Here the predicate is evaluated for every pair on the device
(catchhip_redundancy_graph) and the walk is the lexicographically first maximal
independent set of that graph (catchhip_redundancy_naive): probe i is kept iff
no kept probe before it is redundant to it.  The order of the input is kept and
duplicates are not removed first: under the LCF predicate with lcf_thres above
the probe length identical probes are not redundant, and both stay.

The two factories return a working Python predicate are_redundant(probe_a,
probe_b), as the reference's contract is a callable, and the predicate carries
its kind and parameters (`redundancy_kind`, `redundancy_params`); that is how
the filters know which kernel to run.  A callable from anywhere else cannot run
in a kernel: the filters raise NotImplementedError for it, and there is no CPU
path.

The heuristic.  The reference's redundant_longest_common_substring(...,
prune_with_heuristic_and_anchor=True) first asks probe.shares_some_kmers, which
draws np.random.choice per probe and reads an arbitrary element of a set of
strings, and then measures the common substring around that anchor only: its
answer depends on the random stream and on PYTHONHASHSEED, and it can only miss
redundant pairs (the anchored length is a lower bound of k_lcf).  This package
ALWAYS evaluates the exact predicate, the reference's False branch; the
argument is accepted and ignored.
"""
import logging
import time

import numpy as np

from catch_amd.filter.base_filter import BaseFilter

logger = logging.getLogger(__name__)

_LETTERS = frozenset("ACGTN")


def redundant_shift_and_mismatch_count(shift=0, mismatch_thres=0, quick=True,
                                       quick_mismatch_cutoff=10):
    """Predicate: redundant iff, for some offset s in [-shift, shift], the
    overlapping parts of the two probes differ in at most mismatch_thres
    positions.  On the quick path (quick and mismatch_thres <
    quick_mismatch_cutoff) probes may differ in length and an empty overlap has
    0 mismatches, as in the reference's loop (:112-137); off it the probes must
    be equally long and shift below their length (ValueError otherwise, :139-141
    through Probe.mismatches_at_offset)."""
    if shift < 0:
        raise ValueError("shift must not be negative")
    quick_path = bool(quick and mismatch_thres < quick_mismatch_cutoff)

    def are_redundant(probe_a, probe_b):
        if not quick_path:
            return probe_a.min_mismatches_within_shift(probe_b, shift) <= mismatch_thres
        a = np.frombuffer(probe_a.seq_str.encode("utf-32-le"), dtype=np.uint32)
        b = np.frombuffer(probe_b.seq_str.encode("utf-32-le"), dtype=np.uint32)
        for s in range(-shift, shift + 1):
            i, j = max(s, 0), max(-s, 0)
            size = max(0, min(a.size - i, b.size - j))
            if int(np.count_nonzero(a[i:i + size] != b[j:j + size])) <= mismatch_thres:
                return True
        return False

    are_redundant.redundancy_kind = "shift"
    are_redundant.redundancy_params = (int(shift), int(mismatch_thres), quick_path)
    return are_redundant


def redundant_longest_common_substring(mismatches, lcf_thres,
                                       prune_with_heuristic_and_anchor=True):
    """Predicate: redundant iff the longest common substring with at most
    `mismatches` mismatches is at least lcf_thres long (k_lcf(a, b,
    mismatches)[0] >= lcf_thres).  Characters compare by plain inequality: 'N'
    equals 'N'.  prune_with_heuristic_and_anchor is accepted and IGNORED: the
    exact predicate is always evaluated (see the module docstring)."""
    if mismatches < 0:
        raise ValueError("mismatches must not be negative")

    def are_redundant(probe_a, probe_b):
        return probe_a.longest_common_substring_length(probe_b, mismatches) >= lcf_thres

    are_redundant.redundancy_kind = "lcf"
    are_redundant.redundancy_params = (int(mismatches), int(lcf_thres))
    return are_redundant


def _predicate_of(are_redundant_fn):
    """(kind, params) of a predicate made by the two factories above (None: the
    reference's default, redundant iff identical)."""
    if are_redundant_fn is None:
        are_redundant_fn = redundant_shift_and_mismatch_count(shift=0, mismatch_thres=0)
    kind = getattr(are_redundant_fn, "redundancy_kind", None)
    params = getattr(are_redundant_fn, "redundancy_params", None)
    if kind not in ("shift", "lcf") or params is None:
        raise NotImplementedError(
            "are_redundant_fn must come from redundant_shift_and_mismatch_count or "
            "redundant_longest_common_substring: an arbitrary Python callable cannot run on the GPU path")
    return are_redundant_fn, kind, tuple(params)


COMPLETE = "complete"      # every pair is redundant: no graph is built


def redundancy_graph(strs, kind, params, ctx=None):
    """The device graph of `strs` under the predicate, or COMPLETE when the
    parameters make every pair redundant (lcf_thres <= 0).  ValueError for a
    letter outside ACGTN, a probe longer than the kernel's compiled maximum, or
    -- off the shift predicate's quick path -- what the reference raises for."""
    from catch_amd import engine
    for s in strs:
        if len(s) > engine.REDUNDANT_MAX_LENGTH:
            raise ValueError("a probe has %d bases; the redundancy kernel compares at most %d"
                             % (len(s), engine.REDUNDANT_MAX_LENGTH))
    bad = set("".join(strs)) - _LETTERS
    if bad:
        raise ValueError("probes hold letters outside ACGTN (%s); the redundancy kernel packs those five"
                         % "".join(sorted(bad)))
    if kind == "lcf":
        mismatches, lcf_thres = params
        if lcf_thres <= 0:
            return COMPLETE
        code, p0, p1 = engine.REDUNDANT_LCF, mismatches, lcf_thres
    else:
        shift, mismatch_thres, quick_path = params
        if not quick_path and len(strs) > 1:
            lengths = set(map(len, strs))
            if len(lengths) > 1:
                raise ValueError("Sequences must be of same length")
            if shift >= min(lengths):
                raise ValueError("Invalid offset value " + str(-shift))
        code, p0, p1 = engine.REDUNDANT_SHIFT, shift, mismatch_thres
    if ctx is None:
        ctx = engine.default_context()
    return engine.RedundancyGraph(ctx, strs, code, p0, p1)


class NaiveRedundantFilter(BaseFilter):
    def __init__(self, are_redundant_fn=None):
        self.are_redundant_fn, self._kind, self._params = _predicate_of(are_redundant_fn)
        self.last_timings = {}

    def _keep_mask(self, strs):
        t0 = time.perf_counter()
        graph = redundancy_graph(strs, self._kind, self._params)
        t1 = time.perf_counter()
        if graph is COMPLETE:
            keep = np.zeros(len(strs), dtype=bool)
            keep[:1] = True
            pairs = 0
        else:
            try:
                keep = graph.naive()
                pairs = graph.nedges // 2
            finally:
                graph.close()
        self.last_timings = dict(graph_s=t1 - t0, naive_s=time.perf_counter() - t1, redundant_pairs=pairs)
        return keep

    def _filter_strs(self, strs):
        strs = list(strs)
        if not strs:
            return strs
        return [s for s, k in zip(strs, self._keep_mask(strs).tolist()) if k]

    def _filter(self, input):
        input = list(input)
        if not input:
            return input
        keep = self._keep_mask([p.seq_str for p in input])
        return [p for p, k in zip(input, keep.tolist()) if k]
