"""The cross-dimer dG entries beside their length counterparts, on tools/cross_dimer_profile.py's lists.  (GPU box)
    python tools/cross_duplex_profile.py [--sizes 1000 10000 100000] [--worst 10000] [--repeats 10] [--slow-ms 400]
                                         [--above 20]
For every size a list of uniformly random 100-mers, and for --worst a list of that many records in which every
record's reverse complement is present.  On each list, in one process and alternating, each new entry and the length
entry it was modelled on -- the yardstick, unchanged code:
    catchhip_cross_duplex        |  catchhip_cross_dimer                  (values and partners)
    catchhip_cross_duplex_graph  |  catchhip_cross_dimer_graph            (the graph at G | at X = --above)
G (hundredths of a kcal/mol) is the threshold whose conflict count on that list is closest to X's: the tool finds it
from above -- the largest dcross first, downwards in growing steps until the count reaches X's, then by bisection, so
that no graph it builds on the way is much larger than X's -- and prints it.
The times are the library's own, HIP events around the call's kernels alone (phase 3 of catchhip_ctx_last_kernel_ms);
one warm-up call each; a call that takes longer than --slow-ms in the warm-up is timed 3 times instead of --repeats.
Prints the median, the least and the greatest, the ratio of the medians (new / length), then min / median / 99th
percentile / max of dcross and the number of records whose dpartner differs from their length partner."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from tools.cross_dimer_profile import PHASE_NDF, _RC, _option, _random_list  # noqa: E402


def _edges(ctx, strs, g):
    graph = engine.RedundancyGraph.cross_duplex(ctx, strs, g)
    n = graph.nedges
    graph.close()
    return n


def _closest_g(ctx, strs, top, target):
    """The threshold whose edge count is closest to `target` (edges fall as G rises; of equals the smaller G)."""
    hi, step = top, 32                      # (edges(top) = 0)
    lo = hi
    while lo > 0:
        lo = max(0, lo - step)
        if _edges(ctx, strs, lo) >= target:
            break
        hi, step = lo, step * 2
    while hi - lo > 1:                      # edges(lo) >= target > edges(hi), or lo = 0
        mid = (lo + hi) // 2
        if _edges(ctx, strs, mid) >= target:
            lo = mid
        else:
            hi = mid
    return min((lo, hi), key=lambda g: (abs(_edges(ctx, strs, g) - target), g))


def _line(tag, v, pairs):
    med = statistics.median(v)
    print("%-44s median %.3f ms, min %.3f, max %.3f over %d calls (%.3g pairs per second)" % (
        tag, med, min(v), max(v), len(v), pairs / (med / 1e3) if med > 0 else float("nan")), flush=True)
    return med


def _alternate(ctx, calls, repeats, slow_ms, pairs):
    """Times the (tag, call) pairs in turn; returns the medians by tag."""
    ms, rounds = {}, {}
    for tag, call in calls:                  # (warm-up; it also says how often the call is timed)
        call()
        ms[tag] = []
        rounds[tag] = 3 if ctx.kernel_ms(PHASE_NDF)[0] > slow_ms else repeats
    for rep in range(max(rounds.values())):
        for tag, call in calls:
            if rep < rounds[tag]:
                call()
                ms[tag].append(ctx.kernel_ms(PHASE_NDF)[0])
    return {tag: _line(tag, ms[tag], pairs) for tag, _ in calls}


def _profile(ctx, name, strs, above, repeats, slow_ms):
    n = len(strs)
    pairs = n * (n - 1) // 2
    print("%s: %d records, %d pairs" % (name, n, pairs), flush=True)
    seen = {}

    def length_values():
        seen["length"] = engine.cross_dimer(ctx, strs)

    def dg_values():
        seen["dg"] = engine.cross_duplex(ctx, strs)

    med = _alternate(ctx, [("  cross_duplex (values and partners)", dg_values),
                           ("  cross_dimer (values and partners)", length_values)], repeats, slow_ms, pairs)
    print("  values: new / length = %.2f" % (med["  cross_duplex (values and partners)"] /
                                            med["  cross_dimer (values and partners)"]), flush=True)
    (v, p), (_lv, lp) = seen["dg"], seen["length"]

    def length_graph():
        g = engine.RedundancyGraph.cross_dimer(ctx, strs, above)
        seen["length edges"] = g.nedges
        g.close()

    length_graph()
    g_c = _closest_g(ctx, strs, int(v.max()), seen["length edges"])

    def dg_graph():
        seen["dg edges"] = _edges(ctx, strs, g_c)

    tags = ("  cross_duplex_graph, above %d" % g_c, "  cross_dimer_graph, above %d" % above)
    med = _alternate(ctx, [(tags[0], dg_graph), (tags[1], length_graph)], repeats, slow_ms, pairs)
    print("  graph: new / length = %.2f; G = %.2f kcal/mol gives %d conflicting pairs, X = %d gives %d" % (
        med[tags[0]] / med[tags[1]], g_c / 100.0, seen["dg edges"] // 2, above, seen["length edges"] // 2), flush=True)
    s = np.sort(v)
    print("  dcross: min %d, median %d, 99th percentile %d, max %d; %d of %d records have another partner than by length"
          % (s[0], s[n // 2], s[min(n - 1, (99 * n) // 100)], s[-1], int((p != lp).sum()), n), flush=True)


def main():
    sizes = _option("--sizes", [1000, 10000, 100000], many=True)
    worst = _option("--worst", 10000)
    repeats = _option("--repeats", 10)
    slow_ms = _option("--slow-ms", 400)
    above = _option("--above", 20)
    ctx = engine.Context(0)
    for n in sizes:
        _profile(ctx, "random 100-mers", _random_list(n, n), above, repeats, slow_ms)
    if worst:
        half = _random_list(worst // 2, 7)
        _profile(ctx, "every reverse complement present", half + [s[::-1].translate(_RC) for s in half], above, repeats,
                 slow_ms)
    ctx.close()


if __name__ == "__main__":
    main()
