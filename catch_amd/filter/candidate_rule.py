"""What the filters that judge a candidate probe by itself share on the host
(PolyAFilter, CompositionFilter, StructureFilter, TmFilter, BackgroundFilter):
the walk over strings and probes, and the reading of their options.  Not in
the reference.

A rule defines
  _keeps(s)                          the definition, one string;
  _keep_mask_equal_length(strs, L)   the same in NumPy for strings of one
                                     length L > 0: a bool array; it counts
                                     what it drops, where the rule counts;
  _keep_list(strs)                   optionally, _keeps for strings of any
                                     lengths with the same counting.
"""
from fractions import Fraction

from catch_amd.filter.base_filter import BaseFilter


def _fraction(x, what):
    """x as an exact Fraction: a string, an integer or a Fraction, never a float."""
    if isinstance(x, float):
        raise ValueError("%s must be given as a string or a Fraction, not a float (%r)" % (what, x))
    try:
        return Fraction(x)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("%s is not a number: %r" % (what, x))


def _value_error(message):
    """The default `error` of the rules' from_args (the parsers pass ArgumentParser.error)."""
    raise ValueError(message)


class CandidateRuleFilter(BaseFilter):
    CHUNK = 1 << 14               # strings per NumPy pass (bounded temporaries)

    def _keep_list(self, strs):
        return [self._keeps(s) for s in strs]

    def _filter_strs(self, strs):
        strs = list(strs)
        if not strs:
            return strs
        L = len(strs[0])
        if L == 0 or any(len(s) != L for s in strs):
            return [s for s, k in zip(strs, self._keep_list(strs)) if k]
        out = []
        for a in range(0, len(strs), self.CHUNK):
            part = strs[a:a + self.CHUNK]
            keep = self._keep_mask_equal_length(part, L)
            out += [s for s, k in zip(part, keep.tolist()) if k]
        return out

    def _filter(self, input):
        if len(input) == 0:
            return input
        return [p for p, k in zip(input, self._keep_list([p.seq_str for p in input])) if k]
