"""catchhip_rows_union alone, over the cover rows of a synthetic dataset as ONE instance.  (GPU box)
    python tools/union_profile.py S4 1.0 [--repeats 20] [--mismatches 2] [--extension 50]
Builds the synthetic dataset, puts all its genomes into ONE targets object (a universe per genome), scans its unique
candidates (L = 100, stride 50) once, and times two unions of the scan's rows --
    with themselves    every row of either table is absorbed by its twin: as many rows out as in one table
    with a shifted copy   every row moved up by half a probe (50 bases, clipped to its universe; made on the host from
                          the fetched table, Rows.from_host): a row and its shifted twin overlap, and where the next
                          row starts inside the shifted one a chain forms
-- and, in the same process, catchhip_rows_subtract of the same two tables (rows minus the other table) as the
yardstick: both calls read two tables and write one.  The times are the library's own, HIP events around each call's
device work (phase 1 of catchhip_ctx_last_kernel_ms); the calls alternate after a warm-up of each.  Prints the median,
the least and the greatest of the repeats and the bytes of rows read and written divided by the union's time.  The
shifted copy holds the table on the host (24 bytes per row) and sends it back: at S4 1.0 that is 12 GB."""
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
    si, un, st, en = rows.fetch()
    half = L // 2
    st2, en2 = st + half, np.minimum(en + half, glen[un])
    keep = st2 < en2
    shifted = engine.Rows.from_host(ctx, si[keep], un[keep], st2[keep], en2[keep], glen)
    del si, un, st, en, st2, en2, keep
    pairs = [("with themselves", rows), ("with a shifted copy", shifted)]
    ms = {(tag, what): [] for tag, _o in pairs for what in ("union", "subtract")}
    out = {}
    for rep in range(-2, repeats):           # (two rounds of warm-up)
        for tag, other in pairs:
            both = rows.union(other)
            ms[(tag, "union")].append(ctx.kernel_ms(engine.PHASE_ROWS)[0])
            sub = rows.subtract(other)
            ms[(tag, "subtract")].append(ctx.kernel_ms(engine.PHASE_ROWS)[0])
            out[tag] = (both.n, sub.n, both.longest(), other.n)
            for h in (sub, both):
                h.close()
    for tag, _o in pairs:
        n, nsub, longest, nother = out[tag]
        print("%-20s %d + %d rows in, %d in the union (longest %d), %d left by subtract" % (
            tag, rows.n, nother, n, longest, nsub))
        for what in ("union", "subtract"):
            v = ms[(tag, what)][2:]
            line = "    %-9s median %.3f ms, min %.3f, max %.3f over %d calls" % (
                what, statistics.median(v), min(v), max(v), len(v))
            if what == "union":
                moved = 16 * (rows.n + nother + n)
                line += "; %d bytes of rows read and written, %.1f GB/s" % (moved, moved / statistics.median(v) / 1e6)
            print(line, flush=True)
    for h in (shifted, rows, probes, cands, targets):
        h.close()


if __name__ == "__main__":
    main()
