"""Removes probes with long stretches of A or T (mirrors
catch/filter/polya_filter.py:18-71); the order of the input is kept.

The reference asks, per probe, for the longest common substring with 'A' * L
(and 'T' * L) under `mismatches` mismatches -- an O(L^2) k_lcf call -- and
drops the probe when it is >= `length`; it only asks at all when the probe
holds an exact run of min_exact_length_to_consider 'A' or 'T', which changes
answers and is therefore part of the rule.  A window of >= length characters
with <= mismatches mismatches contains one of exactly `length` characters with
no more, so the rule is: some window of `length` characters differs from 'A'
(or from 'T') in at most `mismatches` places.  Any other character is a
mismatch, 'N' included.

On the device front end the filter is one kernel over the unique candidates
(catchhip_candidates_drop_polya, _apply_to_candidates); the object and host
string paths use the same rule here.
"""
import numpy as np

from catch_amd.filter.candidate_rule import CandidateRuleFilter


class PolyAFilter(CandidateRuleFilter):
    CHUNK = 1 << 16

    def __init__(self, length, mismatches, min_exact_length_to_consider=6):
        self.length = length
        self.mismatches = mismatches
        self.min_exact_length_to_consider = min_exact_length_to_consider

    def _has_window(self, s, base, length, mismatches):
        """Whether `length` consecutive characters of s differ from `base` in
        at most `mismatches` places."""
        if length > len(s):
            return False
        mm = sum(1 for c in s[:length] if c != base)
        if mm <= mismatches:
            return True
        for j in range(length, len(s)):
            mm += (s[j] != base) - (s[j - length] != base)
            if mm <= mismatches:
                return True
        return False

    def _keeps(self, s):
        gate = self.min_exact_length_to_consider
        if "A" * gate not in s and "T" * gate not in s:
            return True
        return not (self._has_window(s, "A", self.length, self.mismatches)
                    or self._has_window(s, "T", self.length, self.mismatches))

    def _keep_mask_equal_length(self, strs, L):
        """_keeps for strings of one length L at once (candidate probes)."""
        rows = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8).reshape(len(strs), L)

        def window(width, mismatches):
            if width > L:
                return np.zeros(len(strs), dtype=bool)
            if width == 0:
                return np.ones(len(strs), dtype=bool)
            hit = np.zeros(len(strs), dtype=bool)
            for base in b"AT":
                cs = np.zeros((len(strs), L + 1), dtype=np.int32)
                np.cumsum(rows != base, axis=1, out=cs[:, 1:])
                hit |= ((cs[:, width:] - cs[:, :L + 1 - width]) <= mismatches).any(axis=1)
            return hit
        drop = window(self.min_exact_length_to_consider, 0) & window(self.length, self.mismatches)
        return ~drop

    def _apply_to_candidates(self, cands):
        """The filter on an engine.Candidates object (grouped or not), before
        any near-duplicate filter."""
        cands.drop_polya(self.length, self.mismatches, self.min_exact_length_to_consider)
