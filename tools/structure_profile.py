"""The structure pre-filter's kernel alone, on the unique candidates of a synthetic dataset as ONE list.  (GPU box)
    python tools/structure_profile.py S4 1.0 [--repeats 20] [--stem 9] [--loop 3] [--dimer 11]
Builds the synthetic dataset, puts all its genomes into ONE targets object and times three calls of
catchhip_candidates_drop_structure (structure_flag_kernel) on the unique candidates (L = 100, stride 50):
    hairpin only      --max-hairpin-stem 9 (--hairpin-min-loop 3)     structure_flag_kernel<true, false, .>
    self-dimer only   --max-self-dimer 11                             structure_flag_kernel<false, true, .>
    both                                                              structure_flag_kernel<true, true, .>
The calls drop candidates, so every repeat makes the list afresh (the list's construction is outside the time); the three
alternate after a warm-up of each.  The time is the library's own, HIP events around the flag kernel alone (phase 9 of
catchhip_ctx_last_kernel_ms); the compaction and the read-back are outside it.  Prints the median, the least and the
greatest of the repeats, what each call dropped, and the kernel's work from the shapes."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

PHASE_PREFILTER = 9


def _option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S2"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    repeats = _option("--repeats", 20)
    K, P, D = _option("--stem", 9), _option("--loop", 3), _option("--dimer", 11)
    L, stride = 100, 50
    genomes = [g for grp in synthetic.dataset(name, scale=scale) for g in grp]
    ctx = engine.Context(0)
    targets = engine.Targets(ctx, genomes)
    calls = [("hairpin only", (K, P, -1)), ("self-dimer only", (-1, P, D)), ("both", (K, P, D))]
    ms = {tag: [] for tag, _ in calls}
    dropped, n, total = {}, None, None
    for rep in range(-2, repeats):           # (two rounds of warm-up)
        for tag, arguments in calls:
            cands = engine.Candidates(ctx, targets, L, stride)
            n, total = cands.n, cands.ncandidates
            dropped[tag] = (cands.drop_structure(*arguments), cands.n)
            t, launches = ctx.kernel_ms(PHASE_PREFILTER)
            assert launches == 1
            cands.close()
            if rep >= 0:
                ms[tag].append(t)
    print("%s x %g: %d bases, %d candidates, %d unique; K = %d, P = %d, D = %d" % (
        name, scale, sum(len(s) for g in genomes for s in g), total, n, K, P, D), flush=True)
    def words(stem, loop, dimer):      # the kernel's loop bounds: each antidiagonal up to just past its middle
        need = min(x + 1 for x in (stem, dimer) if x >= 0)
        total = 0
        for c in range(need - 1, 2 * (L - 1) - (need - 1) + 1):
            lo, hi = max(0, c - L + 1), min(L - 1, c)
            if dimer < 0 and c < 1 + loop:
                continue
            upto = min(hi, (c + dimer) // 2 if dimer >= 0 else (c - 1 - loop) // 2)
            total += max(0, (upto >> 5) - (lo >> 5) + 1)
        return total
    print("work per candidate, from the shapes: words of 32 cells walked (a table of %d cells, %d words if walked whole): "
          "%s; planes: %d words of LDS" % (
              L * L, sum((min(L - 1, c) >> 5) - (max(0, c - L + 1) >> 5) + 1 for c in range(2 * L - 1)),
              ", ".join("%s %d" % (tag, words(*a)) for tag, a in calls), 6 * ((L + 31) // 32) + 7))
    for tag, _ in calls:
        v = ms[tag]
        print("%-15s  median %.3f ms, min %.3f, max %.3f over %d calls (%.2f ns per candidate); dropped with "
              "multiplicity [hairpin, self-dimer, any] = %s, %d of %d unique kept" % (
                  tag, statistics.median(v), min(v), max(v), len(v), 1e6 * statistics.median(v) / max(n, 1),
                  dropped[tag][0], dropped[tag][1], n), flush=True)
    targets.close()


if __name__ == "__main__":
    main()
