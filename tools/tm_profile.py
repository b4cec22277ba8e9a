"""The Tm pre-filter's kernel beside the composition and poly(A) kernels, on one resident candidate list.  (GPU box)
    python tools/tm_profile.py S4 1.0 [--repeats 20]
Builds the synthetic dataset, puts all its genomes into ONE targets object and makes the unique candidates (L = 100,
stride 50) on the device.  Then times six calls on that list, alternating, after a warm-up of each:
    Tm filter + histogram   catchhip_candidates_drop_tm           (tm_flag_kernel<STAGE, true, true>)
    Tm filter only          catchhip_candidates_drop_tm           (tm_flag_kernel<STAGE, true, false>)
    Tm histogram only       catchhip_candidates_drop_tm           (tm_flag_kernel<STAGE, false, true>)
    GC only                 catchhip_candidates_drop_composition  (composition_flag_kernel<STAGE, false>)
    all rules               catchhip_candidates_drop_composition  (composition_flag_kernel<STAGE, true>)
    poly(A)                 catchhip_candidates_drop_polya        (polya_flag_kernel)
with thresholds that drop nothing, so that every repeat sees the same list: the walks have no early exit, their work
does not depend on the thresholds (a Tm range of -300 .. 300 degrees takes the filter's path and adds to no "below" or
"above" counter; the histogram's atomics are all there).  The time is the library's own, HIP events around the flag
kernel alone (phase 9 of catchhip_ctx_last_kernel_ms); the compaction and the read-back are outside it.  Prints the
median, the least and the greatest of the repeats, the histogram's spread (how many bins the atomics go to), and
last one call with a real range (the list's 30th and 70th percentile) on fresh lists, for what the two drop counters
add."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.filter.tm_filter import TmFilter  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

PHASE_PREFILTER = 9


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S2"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 20
    L, stride = 100, 50
    genomes = [g for grp in synthetic.dataset(name, scale=scale) for g in grp]
    ctx = engine.Context(0)
    targets = engine.Targets(ctx, genomes)
    cands = engine.Candidates(ctx, targets, L, stride)
    n = cands.n
    print("%s x %g: %d bases, %d candidates, %d unique" % (
        name, scale, sum(len(s) for g in genomes for s in g), cands.ncandidates, n), flush=True)
    f = TmFilter()
    q, off = f._q(L), f.offset_c
    calls = [
        ("Tm filter + histogram", lambda: cands.drop_tm(q, off, -30000, 30000, histogram=True)),
        ("Tm filter only", lambda: cands.drop_tm(q, off, -30000, 30000, histogram=False)),
        ("Tm histogram only", lambda: cands.drop_tm(q, off, histogram=True)),
        ("GC only", lambda: cands.drop_composition(0, L - 1, -1, -1, 64)),
        ("all rules", lambda: cands.drop_composition(0, L - 1, L - 1, 400000, 64)),
        ("poly(A)", lambda: cands.drop_polya(20, 4, L)),      # --filter-polya 20 4 behind a gate no candidate passes
    ]
    ms = {tag: [] for tag, _ in calls}
    hist = None
    for rep in range(-3, repeats):           # (three rounds of warm-up)
        for tag, call in calls:
            got = call()
            assert cands.n == n, "the timing thresholds must drop nothing"
            t, launches = ctx.kernel_ms(PHASE_PREFILTER)
            assert launches == 1
            if tag == "Tm histogram only":
                hist = got[1]
            if rep >= 0:
                ms[tag].append(t)
    for tag, _ in calls:
        v = ms[tag]
        print("%-22s median %.3f ms, min %.3f, max %.3f over %d calls (%.2f ns per candidate)" % (
            tag, statistics.median(v), min(v), max(v), len(v), 1e6 * statistics.median(v) / max(n, 1)), flush=True)
    med = {tag: statistics.median(v) for tag, v in ms.items()}
    print("Tm filter + histogram / GC only = %.2f, / all rules = %.2f; histogram-off leg saves %.3f ms" % (
        med["Tm filter + histogram"] / med["GC only"], med["Tm filter + histogram"] / med["all rules"],
        med["Tm filter + histogram"] - med["Tm filter only"]))
    filled = [b for b, v in enumerate(hist) if v]
    total = sum(hist)
    top = sorted(hist, reverse=True)
    print("histogram: %d candidates in bins %d .. %d (%d non-empty); the fullest 15 bins hold %.1f %%" % (
        total, filled[0], filled[-1], len(filled), 100.0 * sum(top[:15]) / max(total, 1)))
    acc, lo_c, hi_c = 0, None, None
    for b, v in enumerate(hist):             # whole-degree bounds near the 30th and 70th percentile
        acc += v
        if lo_c is None and acc >= 0.3 * total:
            lo_c = 100 * b
        if hi_c is None and acc >= 0.7 * total:
            hi_c = 100 * b
    cands.close()
    real = []
    for rep in range(6):                     # (a fresh list each time: this call shortens it; the first is warm-up)
        cands = engine.Candidates(ctx, targets, L, stride)
        dropped, _ = cands.drop_tm(q, off, lo_c, hi_c, histogram=True)
        real.append(ctx.kernel_ms(PHASE_PREFILTER)[0])
        kept = cands.n
        cands.close()
    print("real range %.0f .. %.0f degrees: %d of %d unique candidates kept; dropped with multiplicity [below, above, "
          "any] = %s; kernel median %.3f ms, min %.3f, max %.3f over %d calls" % (
              lo_c / 100, hi_c / 100, kept, n, dropped, statistics.median(real[1:]), min(real[1:]), max(real[1:]),
              len(real) - 1))
    targets.close()


if __name__ == "__main__":
    main()
