"""The two cross-dimer entries on lists of random 100-mers, beside the redundancy graph as a yardstick.  (GPU box)
    python tools/cross_dimer_profile.py [--sizes 1000 10000 100000] [--worst 10000] [--repeats 10] [--slow-ms 400]
                                        [--above 20]
For every size a list of uniformly random 100-mers, and for --worst a list of that many records in which every
record's reverse complement is present (the first half random, the second half their reverse complements): every
best is 100, the worst case for the early exits of the value entry.  On each list, in one process and alternating,
    catchhip_cross_dimer                                    (engine.cross_dimer: pack, pairs, result)
    catchhip_cross_dimer_graph at --above                   (RedundancyGraph.cross_dimer: pack, pairs, degree, scan, fill)
    catchhip_redundancy_graph, REDUNDANT_LCF, 0 mismatches, lcf_thres 21
                                                            (the same all-pairs shape: pack, pairs, degree, scan, fill)
The times are the library's own, HIP events around the call's kernels alone (phase 3 of catchhip_ctx_last_kernel_ms);
the upload and the read-back are outside them.  One warm-up call each; a call that takes longer than --slow-ms in
the warm-up is timed 3 times instead of --repeats.  Prints the median, the least and the greatest, and the pairs per
second at the median (n (n - 1) / 2 pairs), then min / median / 99th percentile / max of the values and the edges of
the two graphs."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402

PHASE_NDF = 3
_RC = str.maketrans("ACGT", "TGCA")


def _option(name, default, many=False):
    if name not in sys.argv:
        return default
    at = sys.argv.index(name) + 1
    if not many:
        return int(sys.argv[at])
    out = []
    while at < len(sys.argv) and sys.argv[at].isdigit():
        out.append(int(sys.argv[at]))
        at += 1
    return out


def _random_list(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows = letters[rng.integers(0, 4, size=(n, 100), dtype=np.uint8)]
    return [r.tobytes().decode("ascii") for r in rows]


def _line(tag, v, pairs):
    med = statistics.median(v)
    print("%-44s median %.3f ms, min %.3f, max %.3f over %d calls (%.3g pairs per second)" % (
        tag, med, min(v), max(v), len(v), pairs / (med / 1e3) if med > 0 else float("nan")), flush=True)


def _profile(ctx, name, strs, above, repeats, slow_ms):
    n = len(strs)
    pairs = n * (n - 1) // 2
    print("%s: %d records, %d pairs" % (name, n, pairs), flush=True)
    seen = {}

    def values():
        seen["values"] = engine.cross_dimer(ctx, strs)[0]

    def graph():
        g = engine.RedundancyGraph.cross_dimer(ctx, strs, above)
        seen["edges"] = g.nedges
        g.close()

    def yardstick():
        g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, 0, 21)
        seen["yardstick edges"] = g.nedges
        g.close()

    calls = [("  cross_dimer (values and partners)", values),
             ("  cross_dimer_graph, above %d" % above, graph),
             ("  redundancy_graph, LCF 0 mismatches, 21", yardstick)]
    ms, rounds = {}, {}
    for tag, call in calls:                  # (warm-up; it also says how often the call is timed)
        try:
            call()
        except ValueError as exc:
            print("%s: refused: %s" % (tag, exc), flush=True)
            continue
        ms[tag] = []
        rounds[tag] = 3 if ctx.kernel_ms(PHASE_NDF)[0] > slow_ms else repeats
    for rep in range(max(rounds.values(), default=0)):
        for tag, call in calls:
            if tag in ms and rep < rounds[tag]:
                call()
                ms[tag].append(ctx.kernel_ms(PHASE_NDF)[0])
    for tag, _ in calls:
        if tag in ms:
            _line(tag, ms[tag], pairs)
    v = np.sort(seen["values"])
    print("  cross: min %d, median %d, 99th percentile %d, max %d; %d conflicting pairs above %d; %s pairs in the "
          "yardstick's graph" % (v[0], v[n // 2], v[min(n - 1, (99 * n) // 100)], v[-1], seen.get("edges", 0) // 2, above,
                                 seen["yardstick edges"] // 2 if "yardstick edges" in seen else "NA"), flush=True)


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
