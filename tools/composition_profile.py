"""The composition pre-filter's kernel beside the poly(A) kernel, on one resident candidate list.  (GPU box)
    python tools/composition_profile.py S4 1.0 [--repeats 20]
Builds the synthetic dataset, puts all its genomes into ONE targets object and makes the unique candidates (L = 100,
stride 50) on the device.  Then times three calls on that list, alternating, after a warm-up of each:
    poly(A)     catchhip_candidates_drop_polya        (polya_flag_kernel)
    GC only     catchhip_candidates_drop_composition  (composition_flag_kernel<STAGE, false>: no counters)
    all rules   catchhip_candidates_drop_composition  (composition_flag_kernel<STAGE, true>)
with thresholds that drop nothing, so that every repeat sees the same list: the walks have no early exit, their work
does not depend on the thresholds.  The time is the library's own, HIP events around the flag kernel alone (phase 9 of
catchhip_ctx_last_kernel_ms); the compaction and the read-back are outside it.  Prints the median, the least and the
greatest of the repeats and the bytes the kernels move, from the shapes.  Last, one call with real thresholds
(--filter-gc 0.35 0.6 --max-homopolymer 5 --filter-low-complexity 20) for what it drops."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.filter.composition_filter import CompositionFilter  # noqa: E402
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
    calls = [
        ("poly(A)", lambda: cands.drop_polya(20, 4, L)),      # --filter-polya 20 4 behind a gate no candidate passes
        ("GC only", lambda: cands.drop_composition(0, L - 1, -1, -1, 64)),
        ("all rules", lambda: cands.drop_composition(0, L - 1, L - 1, 400000, 64)),
    ]
    ms = {tag: [] for tag, _ in calls}
    for rep in range(-3, repeats):           # (three rounds of warm-up)
        for tag, call in calls:
            call()
            assert cands.n == n, "the timing thresholds must drop nothing"
            t, launches = ctx.kernel_ms(PHASE_PREFILTER)
            assert launches == 1
            if rep >= 0:
                ms[tag].append(t)
    nchunk = (L + 30) // 16
    print("bytes per flag kernel, from the shapes: upos n * 4, rows at most n * 16 * %d, flag n * 4 = %d; the composition "
          "kernel also reads mult n * 4" % (nchunk, n * (8 + 16 * nchunk)))
    for tag, _ in calls:
        v = ms[tag]
        print("%-9s  median %.3f ms, min %.3f, max %.3f over %d calls (%.2f ns per candidate)" % (
            tag, statistics.median(v), min(v), max(v), len(v), 1e6 * statistics.median(v) / max(n, 1)), flush=True)
    base = statistics.median(ms["poly(A)"])
    print("GC only / poly(A) = %.2f, all rules / poly(A) = %.2f" % (
        statistics.median(ms["GC only"]) / base, statistics.median(ms["all rules"]) / base))
    cands.close()
    real = []
    for rep in range(6):                     # (a fresh list each time: this call shortens it; the first is warm-up)
        cands = engine.Candidates(ctx, targets, L, stride)
        f = CompositionFilter(gc_range=("0.35", "0.6"), max_homopolymer=5, max_dust=20)
        f._apply_to_candidates(cands)
        real.append(ctx.kernel_ms(PHASE_PREFILTER)[0])
        kept = cands.n
        cands.close()
    print("real thresholds: %d of %d unique candidates kept; dropped with multiplicity [GC, homopolymer, low "
          "complexity, any] = %s; kernel median %.3f ms, min %.3f, max %.3f over %d calls (the waves' atomics on top "
          "of the walk)" % (kept, n, f.dropped, statistics.median(real[1:]), min(real[1:]), max(real[1:]), len(real) - 1))
    targets.close()


if __name__ == "__main__":
    main()
