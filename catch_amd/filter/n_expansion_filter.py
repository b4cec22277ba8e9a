"""Replaces every probe that holds 'N' bases by the probes with real bases in
their place (mirrors catch/filter/n_expansion_filter.py:42-105); the order of
the input is kept, a probe's expansions standing where it stood.

A probe with n 'N' becomes 4^n probes.  limit_n_expansion_randomly (None: no
limit) caps n: while more 'N' are left than the limit, one of them -- random.
choice of the remaining positions -- is replaced by a random.choice of
A, T, C, G; `random` is consumed call for call as by the reference, so a seeded
run gives the reference's probes.  The remaining 'N' are expanded first 'N'
first, each in the base order A, T, C, G.  It acts on the few selected probes:
host code.
"""
import itertools
import random

from catch_amd import probe
from catch_amd.filter.base_filter import BaseFilter

_REAL_BASES = ["A", "T", "C", "G"]


class NExpansionFilter(BaseFilter):
    def __init__(self, limit_n_expansion_randomly=3):
        self.limit_n_expansion_randomly = limit_n_expansion_randomly

    def _expand(self, seq):
        """The sequences `seq` (which holds an 'N') expands to, in order."""
        limit = self.limit_n_expansion_randomly
        occurrences = [i for i, base in enumerate(seq) if base == "N"]
        if limit is not None and len(occurrences) > limit:
            bases = list(seq)
            while len(occurrences) > limit:
                occ = random.choice(occurrences)
                bases[occ] = random.choice(_REAL_BASES)
                occurrences.remove(occ)
            seq = "".join(bases)
        # first 'N' first = the first 'N' varies slowest: the product's order
        parts = seq.split("N")
        out = []
        for fill in itertools.product(_REAL_BASES, repeat=len(parts) - 1):
            out.append("".join(itertools.chain.from_iterable(
                zip(parts, fill + ("",)))))
        return out

    def _filter_strs(self, strs):
        out = []
        for s in strs:
            if "N" in s:
                out += self._expand(s)
            else:
                out.append(s)
        return out

    def _filter(self, input):
        output = []
        for p in input:
            if "N" not in p.seq_str:
                output.append(p)        # the same object, as in the reference
                continue
            output += [probe.Probe.from_str(s) for s in self._expand(p.seq_str)]
        return output
