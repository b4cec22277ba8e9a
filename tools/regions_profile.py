"""The target-region calls alone, over the coordinate space of a synthetic dataset as ONE instance.  (GPU box)
    python tools/regions_profile.py S4 1.0 [--repeats 20] [--mismatches 2] [--extension 50]
Builds the synthetic dataset, puts all its genomes into ONE targets object (a universe per genome), scans its unique
candidates (L = 100, stride 50) once, and times, for two interval sets --
    one region    one 1,000-base interval in the middle of every genome
    one hole      everything wanted except that interval
-- catchhip_basemask_create (the word-parallel build and the count per universe), catchhip_rows_restrict of the scan's
rows, and, in the same process, catchhip_rows_subtract of the same rows against the equivalent table (the unwanted
bases as the rows of one set, Rows.from_host), which gives the same rows.  The times are the library's own, HIP events
around each call's device work (phase 1 of catchhip_ctx_last_kernel_ms); the calls alternate after a warm-up of each.
Prints the median, the least and the greatest of the repeats and the bitmap bytes written divided by the build time."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.filter import set_cover_filter as scf  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402


def _option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S2"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    repeats = _option("--repeats", 20)
    mismatches, ext = _option("--mismatches", 2), _option("--extension", 50)
    L, stride = 100, 50
    genomes = [g for grp in synthetic.dataset(name, scale=scale) for g in grp]
    glen = np.array([sum(len(s) for s in g) for g in genomes], dtype=np.int64)
    ctx = engine.Context(0)
    targets = engine.Targets(ctx, genomes)
    cands = engine.Candidates(ctx, targets, L, stride)
    probes = scf._probes_of_candidates(cands, scf._anchors_for_candidates(cands.n, L, mismatches, L, 20))
    rows = engine.Rows.scan(ctx, probes, targets, mismatches, L, 0, ext)
    print("%s x %g: %d bases in %d genomes, %d unique candidates, %d cover rows (m = %d, e = %d)" % (
        name, scale, int(glen.sum()), len(genomes), cands.n, rows.n, mismatches, ext), flush=True)
    univ = np.arange(len(genomes), dtype=np.int32)
    mid = np.minimum(glen // 2, np.maximum(glen - 1000, 0))
    end = np.minimum(mid + 1000, glen)
    some = end > mid
    region = (univ[some], mid[some], end[some])
    # everything but the interval: up to two intervals per genome, in (universe, start) order
    hu = np.repeat(univ, 2)
    hs = np.stack([np.zeros_like(mid), end], axis=1).ravel()
    he = np.stack([mid, glen], axis=1).ravel()
    keep = he > hs
    hole = (hu[keep], hs[keep], he[keep])
    zeros = lambda n: np.zeros(n, dtype=np.int32)      # noqa: E731
    sets = [("one region", region, hole), ("one hole", hole, region)]
    ms = {(tag, what): [] for tag, _w, _c in sets for what in ("mask", "restrict", "subtract")}
    nrows, words = {}, (int(glen.sum()) // 64 + 2) + 8
    for rep in range(-2, repeats):           # (two rounds of warm-up)
        for tag, want, unwanted in sets:
            mask = engine.BaseMask(ctx, glen, *want)
            ms[(tag, "mask")].append(mask.last_build_ms)
            cut = rows.restrict(mask)
            ms[(tag, "restrict")].append(ctx.kernel_ms(engine.PHASE_ROWS)[0])
            covered = engine.Rows.from_host(ctx, zeros(unwanted[0].size), *unwanted, glen)
            sub = rows.subtract(covered)
            ms[(tag, "subtract")].append(ctx.kernel_ms(engine.PHASE_ROWS)[0])
            assert sub.n == cut.n
            nrows[tag] = (cut.n, int(mask.wanted.sum()), want[0].size)
            for h in (sub, covered, cut, mask):
                h.close()
    for tag, _w, _c in sets:
        n, wanted, niv = nrows[tag]
        print("%-10s  %d intervals, %d wanted bases, %d rows left of %d" % (tag, niv, wanted, n, rows.n))
        for what in ("mask", "restrict", "subtract"):
            v = ms[(tag, what)][2:]
            line = "    %-9s median %.3f ms, min %.3f, max %.3f over %d calls" % (
                what, statistics.median(v), min(v), max(v), len(v))
            if what == "mask":
                line += "; %d bitmap bytes written, %.1f GB/s" % (8 * words, 8 * words / statistics.median(v) / 1e6)
            print(line, flush=True)
    for h in (rows, probes, cands, targets):
        h.close()


if __name__ == "__main__":
    main()
