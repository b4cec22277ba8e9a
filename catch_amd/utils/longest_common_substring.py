"""Longest common substring with k mismatches on the host (the contract of
catch/utils/longest_common_substring.py:11-56, k_lcf).

The reference walks every diagonal of the |a| x |b| comparison matrix character
by character with a queue of the last k mismatches.  Here a diagonal is one
NumPy comparison: with its mismatch positions p_0 < p_1 < ... and the two ends
of the diagonal standing in as p_-1 = -1 and p_c = O, the longest stretch with
at most k mismatches is the largest p_(j+k+1) - p_j - 1, and it starts at
p_j + 1.  Diagonals are visited in the reference's order and only a strictly
longer stretch replaces the best one, so the reported starts are the
reference's as well.  Characters compare by plain inequality ('N' equals 'N').

This is host code for the Python predicates of
catch_amd.filter.naive_redundant_filter; the filters themselves evaluate their
predicate for all pairs on the device (csrc/redundant.hip).
"""
import numpy as np


def _codes(s):
    if isinstance(s, str):
        return np.frombuffer(s.encode("utf-32-le"), dtype=np.uint32)
    return np.asarray(s)


def k_lcf(a, b, k):
    """(length, start in a, start in b) of the longest common substring of a and
    b with at most k mismatches; (0, 0, 0) when there is none."""
    if k < 0:
        raise ValueError("k must not be negative")
    a, b = _codes(a), _codes(b)
    n, m = len(a), len(b)
    best, r_a, r_b = 0, 0, 0
    for d in range(-m + 1, n):
        i, j = max(d, 0), max(-d, 0)
        size = min(n - i, m - j)
        if size <= best:
            continue      # nothing on this diagonal can be strictly longer
        pos = np.flatnonzero(a[i:i + size] != b[j:j + size])
        if pos.size <= k:
            length, start = size, 0
        else:
            ends = np.concatenate(([-1], pos, [size]))
            gaps = ends[k + 1:] - ends[:-(k + 1)] - 1
            at = int(np.argmax(gaps))
            length, start = int(gaps[at]), int(ends[at]) + 1
        if length > best:
            best, r_a, r_b = length, i + start, j + start
    return best, r_a, r_b
