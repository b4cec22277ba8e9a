"""Dominating set filter (mirrors catch/filter/dominating_set_filter.py:41-91).

Probes are vertices, a redundant pair is an edge, and the filter approximates
the smallest set of probes such that every probe is chosen or redundant to a
chosen one.  The reference builds the sets S_i = {probe i} + {probes redundant
to i} pair by pair in Python and runs set_cover.approx on them
(catch/utils/set_cover.py:14-144, cost 1, p = 1), which always takes the set
with the largest gain and, of equal gains, the one with the lowest id.

Here the graph is built on the device (catchhip_redundancy_graph, the exact
predicate for every pair), a kernel turns it into the cover rows of the sets
(catchhip_redundancy_rows) and the library's greedy solver picks
(catchhip_setcover_greedy: largest gain, lowest id on ties).

The reference's universe holds Probe objects, which hash by sequence, so equal
probes are one element.  The filter therefore builds the graph on the first
occurrence of every sequence and maps the picks back to that occurrence's input
index; a duplicate has the same set and a larger id and is never picked.  The
result is `[input[id] for id in set_ids_in_cover]` over a Python set of ints: a
real set is filled in pick order and iterated, so the interpreter gives the
order the reference returns.

The predicate must come from catch_amd.filter.naive_redundant_filter's two
factories (NotImplementedError otherwise; the LCF predicate is always exact,
see that module).
"""
import logging
import time

from catch_amd.filter import naive_redundant_filter
from catch_amd.filter.base_filter import BaseFilter

logger = logging.getLogger(__name__)


class DominatingSetFilter(BaseFilter):
    def __init__(self, are_redundant_fn=None):
        self.are_redundant_fn, self._kind, self._params = naive_redundant_filter._predicate_of(are_redundant_fn)
        self.last_timings = {}
        self.last_picks = []

    def _pick_ids(self, strs):
        """Input indices in the order the greedy cover picks them."""
        first = {}
        for i, s in enumerate(strs):
            first.setdefault(s, i)
        uniq = list(first)
        first_index = list(first.values())
        t0 = time.perf_counter()
        graph = naive_redundant_filter.redundancy_graph(uniq, self._kind, self._params)
        t1 = time.perf_counter()
        if graph is naive_redundant_filter.COMPLETE:
            picks, pairs = [0], 0         # set 0 covers everything, and no set has a larger gain or a lower id
        else:
            try:
                rows = graph.rows()
                try:
                    picks = rows.greedy(len(uniq))
                finally:
                    rows.close()
                pairs = graph.nedges // 2
            finally:
                graph.close()
        self.last_timings = dict(graph_s=t1 - t0, solve_s=time.perf_counter() - t1, redundant_pairs=pairs)
        self.last_picks = [first_index[u] for u in picks]
        return self.last_picks

    def _ids_in_cover(self, strs):
        set_ids_in_cover = set()
        for i in self._pick_ids(strs):
            set_ids_in_cover.add(i)
        return set_ids_in_cover

    def _filter_strs(self, strs):
        strs = list(strs)
        if not strs:
            return strs
        return [strs[i] for i in self._ids_in_cover(strs)]

    def _filter(self, input):
        input = list(input)
        if not input:
            return input
        return [input[i] for i in self._ids_in_cover([p.seq_str for p in input])]
