"""The two list-against-list entries on random 100-mers, beside the one-list entries as the yardstick.  (GPU box)
    python tools/cross_against_profile.py [--shapes 1000x100000 10000x1000000] [--one-list 10000 100000]
                                          [--repeats 10] [--above 20]
A shape is na x nb: nb uniformly random 100-mers (B, the candidates) against na others (A, the kept probes).  Shape i
is timed in the same rounds as the one-list entries on a list of --one-list[i] records, alternating, in one process:
    catchhip_cross_against_flags at --above     (engine.cross_against_flags: pack A, pack B, pairs)
    catchhip_cross_against                      (engine.cross_against: pack A, pack B, pairs, result)
    catchhip_cross_dimer_graph at --above       (RedundancyGraph.cross_dimer: pack, pairs, degree, scan, fill)
    catchhip_cross_dimer                        (engine.cross_dimer: pack, pairs, result)
The times are the library's own, HIP events around the call's kernels alone (phase 3 of catchhip_ctx_last_kernel_ms);
the upload and the read-back are outside them.  One warm-up call each, then --repeats timed calls.  Prints the median,
the least and the greatest, and the pairs per second at the median (na nb pairs, n (n - 1) / 2 for the one-list
entries), then the flagged records and the largest value."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402

PHASE_NDF = 3


def _option(name, default, many=False):
    if name not in sys.argv:
        return default
    at = sys.argv.index(name) + 1
    if not many:
        return int(sys.argv[at])
    out = []
    while at < len(sys.argv) and not sys.argv[at].startswith("--"):
        out.append(sys.argv[at])
        at += 1
    return out


def _random_list(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows = letters[rng.integers(0, 4, size=(n, 100), dtype=np.uint8)]
    return [r.tobytes().decode("ascii") for r in rows]


def _line(tag, v, pairs):
    med = statistics.median(v)
    print("%-52s median %.3f ms, min %.3f, max %.3f over %d calls (%.3g pairs per second)" % (
        tag, med, min(v), max(v), len(v), pairs / (med / 1e3) if med > 0 else float("nan")), flush=True)


def _profile(ctx, na, nb, n, above, repeats):
    as_, bs, one = _random_list(na, na), _random_list(nb, nb + 1), _random_list(n, n)
    print("%d records against %d (%d pairs); one list of %d (%d pairs)" % (nb, na, na * nb, n, n * (n - 1) // 2), flush=True)
    seen = {}

    def flags():
        seen["flagged"] = int(engine.cross_against_flags(ctx, bs, as_, above).sum())

    def values():
        seen["largest"] = int(engine.cross_against(ctx, bs, as_)[0].max())

    def graph():
        g = engine.RedundancyGraph.cross_dimer(ctx, one, above)
        seen["edges"] = g.nedges
        g.close()

    def one_list():
        seen["one largest"] = int(engine.cross_dimer(ctx, one)[0].max())

    calls = [("  cross_against_flags, above %d" % above, flags, na * nb),
             ("  cross_against (values and partners)", values, na * nb),
             ("  cross_dimer_graph, above %d (one list)" % above, graph, n * (n - 1) // 2),
             ("  cross_dimer (values and partners, one list)", one_list, n * (n - 1) // 2)]
    ms = {}
    for tag, call, _pairs in calls:          # (warm-up)
        try:
            call()
        except ValueError as exc:
            print("%s: refused: %s" % (tag, exc), flush=True)
            continue
        ms[tag] = []
    for _rep in range(repeats):
        for tag, call, _pairs in calls:
            if tag in ms:
                call()
                ms[tag].append(ctx.kernel_ms(PHASE_NDF)[0])
    for tag, _call, pairs in calls:
        if tag in ms:
            _line(tag, ms[tag], pairs)
    print("  %d of %d records flagged above %d, largest value %s; one list: %s conflicting pairs, largest value %s" % (
        seen.get("flagged", -1), nb, above, seen.get("largest", "NA"),
        seen["edges"] // 2 if "edges" in seen else "NA", seen.get("one largest", "NA")), flush=True)


def main():
    shapes = [tuple(int(x) for x in s.split("x")) for s in _option("--shapes", ["1000x100000", "10000x1000000"], many=True)]
    ones = [int(x) for x in _option("--one-list", ["10000", "100000"], many=True)]
    repeats = _option("--repeats", 10)
    above = _option("--above", 20)
    if len(ones) != len(shapes):
        sys.exit("--one-list takes one size per shape")
    ctx = engine.Context(0)
    for (na, nb), n in zip(shapes, ones):
        _profile(ctx, na, nb, n, above, repeats)
    ctx.close()


if __name__ == "__main__":
    main()
