"""The measure kernels beside the flag kernels they look behind, on one resident candidate list.  (GPU box)
    python tools/measure_profile.py S4 1.0 [--repeats 20] [--loop 3] [--window 64] [--background-bases 8000000]
Builds the synthetic dataset, puts all its genomes into ONE targets object and makes the unique candidates (L = 100,
stride 50) on the device.  Then times, alternating, after a warm-up of each:
    measure composition   catchhip_candidates_measure  (measure_rows_kernel<STAGE, true, false, false>, histograms)
    measure structure     catchhip_candidates_measure  (measure_structure_kernel<LDS>, histograms)
    measure Tm            catchhip_candidates_measure  (measure_rows_kernel<STAGE, false, true, false>, values)
    measure hits          catchhip_candidates_measure  (measure_rows_kernel<STAGE, false, false, true>, values)
    measure all           catchhip_candidates_measure  (both kernels, every family, values and histograms)
    flag structure        catchhip_candidates_drop_structure at K = 9, P = 3, D = 11
    flag composition      catchhip_candidates_drop_composition, all three rules
    flag Tm               catchhip_candidates_drop_tm, filter and histogram
The measure calls leave the list as it is; the flag calls get thresholds that drop nothing except the structure one,
which makes its list afresh every repeat (outside the time).  The time is the library's own, HIP events around the
kernels alone (phase 9 of catchhip_ctx_last_kernel_ms); the read-back of values and histograms is outside it.  Prints
the median, the least and the greatest of the repeats, the medians of the five quantities, and the work of the structure
measure from the shapes."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.filter.tm_filter import TmFilter  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

PHASE_PREFILTER = 9


def _option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "S4"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 and not sys.argv[2].startswith("-") else 1.0
    repeats = _option("--repeats", 20)
    P, W, bases = _option("--loop", 3), _option("--window", 64), _option("--background-bases", 8000000)
    L, stride = 100, 50
    genomes = [g for grp in synthetic.dataset(name, scale=scale) for g in grp]
    ctx = engine.Context(0)
    targets = engine.Targets(ctx, genomes)
    cands = engine.Candidates(ctx, targets, L, stride)
    n, total = cands.n, cands.ncandidates
    tf = TmFilter()
    tm = (tf._q(L), tf.offset_c)
    rng = np.random.Generator(np.random.PCG64(1))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    index = engine.KmerIndex(ctx, [letters[rng.integers(0, 4, size=bases, dtype=np.uint8)].tobytes().decode("ascii")], 24)
    print("%s x %g: %d bases, %d candidates, %d unique; P = %d, W = %d; background of %d bases, %d distinct 24-mers" % (
        name, scale, sum(len(s) for g in genomes for s in g), total, n, P, W, bases, index.n_unique), flush=True)

    def flag_structure():
        fresh = engine.Candidates(ctx, targets, L, stride)
        try:
            fresh.drop_structure(9, 3, 11)
            return ctx.kernel_ms(PHASE_PREFILTER)
        finally:
            fresh.close()

    def on_list(call):
        def run():
            call()
            return ctx.kernel_ms(PHASE_PREFILTER)
        return run
    kw = dict(min_loop=P, dust_window=W)
    calls = [
        ("measure composition", on_list(lambda: cands.measure(what="composition", values=False, histograms=True, **kw))),
        ("measure structure", on_list(lambda: cands.measure(what="structure", values=False, histograms=True, **kw))),
        ("measure Tm", on_list(lambda: cands.measure(what="tm", tm=tm, values=True, histograms=False))),
        ("measure hits", on_list(lambda: cands.measure(what="hits", index=index, values=True, histograms=False))),
        ("measure all", on_list(lambda: cands.measure(what=("composition", "structure", "tm", "hits"), tm=tm, index=index,
                                                      values=True, histograms=True, **kw))),
        ("flag structure", flag_structure),
        ("flag composition", on_list(lambda: cands.drop_composition(0, L - 1, L - 1, 400000, 64))),
        ("flag Tm", on_list(lambda: cands.drop_tm(tm[0], tm[1], -30000, 30000, histogram=True))),
    ]
    ms = {tag: [] for tag, _ in calls}
    launches = {}
    for rep in range(-2, repeats):           # (two rounds of warm-up)
        for tag, run in calls:
            t, launches[tag] = run()
            if rep >= 0:
                ms[tag].append(t)
    assert cands.n == n
    for tag, _ in calls:
        v = ms[tag]
        print("%-20s median %.3f ms, min %.3f, max %.3f over %d calls (%.2f ns per candidate), %d launch(es)" % (
            tag, statistics.median(v), min(v), max(v), len(v), 1e6 * statistics.median(v) / max(n, 1), launches[tag]),
            flush=True)
    got = cands.measure(values=False, histograms=True, **kw)["histograms"]
    for q, h in got.items():
        cum = np.cumsum(h)
        print("%-12s median %d, 99th percentile %d, largest %d" % (
            q, int(np.searchsorted(cum, (cum[-1] + 1) // 2)), int(np.searchsorted(cum, cum[-1] * 0.99)),
            int(np.flatnonzero(h)[-1])))
    half = sum(((c >> 1) >> 5) - (max(0, c - L + 1) >> 5) + 1 for c in range(1, 2 * L - 2))
    whole = sum((min(L - 1, c) >> 5) - (max(0, c - L + 1) >> 5) + 1 for c in range(2 * L - 1))
    print("structure measure, from the shapes: %d words of 32 cells walked per candidate (%d if the table were walked "
          "whole); planes: %d words of LDS" % (half, whole, 6 * ((L + 31) // 32) + 7))
    index.close()
    cands.close()
    targets.close()


if __name__ == "__main__":
    main()
