"""The background screen's index build and flag kernel against backgrounds of three sizes, on one resident candidate
list.  (GPU box)
    python tools/background_profile.py S4 1.0 [--repeats 10] [--kmer 24] [--bases 200000 8000000 64000000]
                                              [--mismatches 1] [--slow-ms 400]
Builds the synthetic dataset, puts all its genomes into ONE targets object and makes the unique candidates (L = 100,
stride 50) on the device.  For every background size -- uniformly random bases, one record; by default one whose index
fits an XCD's 4 MiB L2, one that fits the 256 MiB Infinity Cache and one well beyond it -- it
    builds the index a few times      catchhip_kmer_index_create            (emit, scan, pair sort, distinct, directory)
    and times three calls on the list catchhip_candidates_drop_background   (background_flag_kernel<STAGE, FILTER, HIST>)
        filter + histogram, filter only, histogram only
alternating, after a warm-up of each, with max_hits = L, which drops nothing, so that every repeat sees the same list:
the walk has no early exit and every valid position is looked up whatever the threshold.  The Tm kernel (filter only)
and the composition kernel (GC only) run in the same rounds for scale.  The times are the library's own, HIP events
around the flag kernel alone, and for the build from behind the upload to the finished directory (phase 9 of
catchhip_ctx_last_kernel_ms); the compaction and the read-back are outside them.  Prints the median, the least and the
greatest of the repeats, the index's size, and the histogram (a random background shares next to nothing with the
candidates: the look-ups are all there, the hits are not).

--mismatches M (1 or 2; --kmer and --mismatches may each list several values, paired in order): next to the exact index
a tolerant one of the same background (catchhip_kmer_index_create_tolerant) is built and timed, and the filter +
histogram call against it (background_flag_tolerant_kernel<M, ...>) runs in the same rounds as the exact calls, so the
M = 0 times of a run are its own baseline.  Printed as well: the tolerant index's bytes, and per view the directory
bits, the mean entries per bucket (n_unique / 2^P) and the longest bucket, from the fetched view.  A tolerant call that
takes longer than --slow-ms in the warm-up is timed 3 times instead of --repeats (long buckets: K = 32, M = 2 against
64 M bases walks about a hundred entries per position)."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine  # noqa: E402
from catch_amd.filter.tm_filter import TmFilter  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

PHASE_PREFILTER = 9


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


def _line(tag, v, n, per="candidate"):
    print("%-34s median %.3f ms, min %.3f, max %.3f over %d calls (%.2f ns per %s)" % (
        tag, statistics.median(v), min(v), max(v), len(v), 1e6 * statistics.median(v) / max(n, 1), per), flush=True)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S2"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    repeats = _option("--repeats", 10)
    kmers = _option("--kmer", [24], many=True)
    budgets = _option("--mismatches", [0], many=True)
    slow_ms = _option("--slow-ms", 400)
    assert len(kmers) == len(budgets) or len(kmers) == 1 or len(budgets) == 1
    count = max(len(kmers), len(budgets))
    configs = list(zip(kmers * (count // len(kmers)), budgets * (count // len(budgets))))
    sizes = _option("--bases", [200_000, 8_000_000, 64_000_000], many=True)
    L, stride = 100, 50
    genomes = [g for grp in synthetic.dataset(name, scale=scale) for g in grp]
    ctx = engine.Context(0)
    targets = engine.Targets(ctx, genomes)
    cands = engine.Candidates(ctx, targets, L, stride)
    n = cands.n
    print("%s x %g: %d bases, %d candidates, %d unique" % (
        name, scale, sum(len(s) for g in genomes for s in g), cands.ncandidates, n), flush=True)
    tm = TmFilter()
    q, off = tm._q(L), tm.offset_c
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for (K, M), bases in [(c, b) for c in configs for b in sizes]:
        print("K = %d, M = %d: %d positions per candidate" % (K, M, L - K + 1), flush=True)
        rng = np.random.default_rng(bases)
        background = [letters[rng.integers(0, 4, size=bases, dtype=np.uint8)].tobytes().decode("ascii")]
        build = []
        index = None
        for rep in range(4):                 # (the first build is warm-up)
            if index is not None:
                index.close()
            index = engine.KmerIndex(ctx, background, K)
            t, launches = ctx.kernel_ms(PHASE_PREFILTER)
            if rep:
                build.append(t)
        P = min(max(int(index.n_unique - 1).bit_length(), 8), min(2 * K, 30))
        resident = 8 * index.n_unique + 4 * ((1 << P) + 1)
        print("background of %d bases: %d valid positions, %d distinct k-mers, directory of 2^%d; resident %.1f MiB "
              "(%.1f bytes per distinct k-mer), build scratch about %.1f MiB; %d launches per build" % (
                  bases, index.n_valid, index.n_unique, P, resident / 2 ** 20, resident / max(index.n_unique, 1),
                  24 * index.n_valid / 2 ** 20, launches), flush=True)
        _line("  index build", build, index.n_valid, "valid position")
        tolerant = None
        if M:
            build = []
            for rep in range(4):
                if tolerant is not None:
                    tolerant.close()
                tolerant = engine.KmerIndex(ctx, background, K, mismatches=M)
                t, launches = ctx.kernel_ms(PHASE_PREFILTER)
                if rep:
                    build.append(t)
            _line("  tolerant index build (M = %d)" % M, build, index.n_valid, "valid position")
            starts = [b * K // (M + 1) for b in range(M + 2)]
            size = 0
            for b in range(M + 1):
                pcap = 2 * (starts[b + 1] - starts[b])
                Pb = min(max(int(index.n_unique - 1).bit_length(), 8), min(pcap, 30))
                view = tolerant.fetch_view(b)
                longest = int(np.bincount((view >> np.uint64(2 * K - Pb)).astype(np.int64), minlength=1).max())
                del view
                size += 8 * index.n_unique + 4 * ((1 << Pb) + 1)
                print("    view %d: block of %d characters, directory of 2^%d, mean bucket %.2f, longest bucket %d" % (
                    b, starts[b + 1] - starts[b], Pb, index.n_unique / 2 ** Pb, longest), flush=True)
            print("    tolerant index resident %.1f MiB, %d launches per build" % (size / 2 ** 20, launches), flush=True)
        calls = [
            ("  background filter + histogram", lambda: cands.drop_background(index, L, histogram=True)),
            ("  background filter only", lambda: cands.drop_background(index, L, histogram=False)),
            ("  background histogram only", lambda: cands.drop_background(index, None, histogram=True)),
            ("  Tm filter only", lambda: cands.drop_tm(q, off, -30000, 30000, histogram=False)),
            ("  GC only", lambda: cands.drop_composition(0, L - 1, -1, -1, 64)),
        ]
        if M:
            calls.insert(1, ("  tolerant filter + histogram", lambda: cands.drop_background(tolerant, L, histogram=True)))
        ms = {tag: [] for tag, _ in calls}
        hist = None
        slow = False
        for rep in range(-2, repeats):       # (two rounds of warm-up)
            for tag, call in calls:
                if slow and rep >= 3 and tag.startswith("  tolerant"):
                    continue
                got = call()
                assert cands.n == n, "the timing thresholds must drop nothing"
                t, launches = ctx.kernel_ms(PHASE_PREFILTER)
                assert launches == 1
                if tag.endswith("histogram only"):
                    hist = got[1]
                if tag.startswith("  tolerant"):
                    if rep < 0 and t > slow_ms:
                        slow = True
                    thist = got[1]
                if rep >= 0:
                    ms[tag].append(t)
        for tag, _ in calls:
            _line(tag, ms[tag], n)
        filled = [b for b, v in enumerate(hist) if v]
        print("  histogram: %d candidates, %d with hits, most hits %d" % (sum(hist), sum(hist[1:]), filled[-1]), flush=True)
        if M:
            filled = [b for b, v in enumerate(thist) if v]
            print("  within %d mismatches: %d with hits, most hits %d" % (M, sum(thist[1:]), filled[-1]), flush=True)
            tolerant.close()
        index.close()
    cands.close()
    targets.close()


if __name__ == "__main__":
    main()
