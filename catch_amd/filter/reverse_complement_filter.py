"""Adds the reverse complement of every probe (mirrors
catch/filter/reverse_complement_filter.py:18-34): [P1, P2] becomes
[P1, P1r, P2, P2r], and both get the header that says which is which.  It acts
on the few selected probes: host code.
"""
from catch_amd.filter.base_filter import BaseFilter


class ReverseComplementFilter(BaseFilter):
    def _filter(self, input):
        output = []
        for p in input:
            p.header = "probe_%s | from target sequence" % p.identifier()
            output.append(p)
            p_rc = p.reverse_complement()
            p_rc.header = ("probe_%s | reverse complement of probe_%s"
                           % (p_rc.identifier(), p.identifier()))
            output.append(p_rc)
        return output
