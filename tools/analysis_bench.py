#!/usr/bin/env python3
"""Wall time of a coverage analysis with the sliding-window file, both strands:
Analyzer.run() + write_sliding_window_coverage(), with the window depth on the
device (the default) against CATCHHIP_ANALYSIS_HOST_WINDOWS=1 (every range
fetched, the depth and the windows computed on the host -- what the package did
before catchhip_rows_window_depth), alternating the two in one process.

  ebola  the 100 genomes of tests/golden/ebola_zaire_100.fasta.gz and the probes
         a design at -pl 100 -m 2 -e 50 selects for them
  S4     synthetic.dataset("S4", scale) (config 4's shape: 20 datasets) and the
         probes the same design selects; --scale sets the size (the host path
         builds a Python tuple per range: keep it where that finishes)

Prints one JSON line per input: per mode the seconds of every repeat (run,
write, total), their median and min-max spread, the ratio of the medians,
whether the two modes wrote identical files, and the traffic the window
kernels need (bytes, from the shapes) for a bytes-per-second figure over the
kernel time of a rocprofv3 --kernel-trace --stats run (--modes device
--repeat 1 for that).  --tree DIR imports the package from another checkout
(an older commit, which has only its one path: --modes device).

--leg uncovered times the region list instead: Analyzer.uncovered_regions() (one
scan per strand and catchhip_rows_uncovered; only the regions come back) against
the host path it replaces -- target_covers fetched (a scan per strand, every
unmerged range to the host) and complemented per genome in NumPy -- on an
analyzer that has run, alternating the two.  Per mode the wall seconds; for the
device also the milliseconds of catchhip_rows_uncovered itself (HIP events, both
strands), and the bytes its kernels move, from the shapes.

    python tools/analysis_bench.py [--inputs ebola S4] [--scale 0.05] [--repeat 3] [--leg windows|uncovered]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
os.environ.setdefault("CATCHHIP_TEST_HOOKS", "1")     # the host-windows switch is a test hook


def design(genome_mod, groups):
    from catch_amd.filter import duplicate_filter, probe_designer, set_cover_filter
    pb = probe_designer.ProbeDesigner(
        groups, [duplicate_filter.DuplicateFilter(),
                 set_cover_filter.SetCoverFilter(mismatches=2, lcf_thres=100, cover_extension=50)],
        probe_length=100, probe_stride=50)
    pb.design()
    return pb.final_probes


def load(name, scale):
    from catch_amd import genome
    from catch_amd.utils import seq_io, synthetic
    if name == "ebola":
        groups = [seq_io.read_genomes_from_fasta(os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz"))]
    else:
        groups = [[genome.Genome.from_one_seq("".join(g)) for g in grp]
                  for grp in synthetic.dataset(name, scale=scale)]
    return groups, design(genome, groups)


def one(groups, probes, host, out_fn):
    from catch_amd import coverage_analysis, engine
    if host:
        os.environ["CATCHHIP_ANALYSIS_HOST_WINDOWS"] = "1"
    else:
        os.environ.pop("CATCHHIP_ANALYSIS_HOST_WINDOWS", None)
    ctx = engine.default_context()
    a = coverage_analysis.Analyzer(probes, 2, 100, groups, cover_extension=50)
    ctx.sync()
    t0 = time.perf_counter()
    a.run()
    t1 = time.perf_counter()
    a.write_sliding_window_coverage(out_fn)      # ends in a device synchronise (the read-back of the windows)
    t2 = time.perf_counter()
    with open(out_fn, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    return dict(run_s=t1 - t0, write_s=t2 - t1, total_s=t2 - t0), digest


def host_uncovered(a):
    """The regions from target_covers, per genome in NumPy: depth by difference array over the genome's coordinates,
    runs of depth 0 cut at the chromosome boundaries, A/C/G/T counted from the bytes; regions with none are dropped
    (uncovered_regions()' defaults).  Same shape as Analyzer.uncovered_regions()."""
    import numpy as np
    rc_table = str.maketrans("ACGT", "TGCA")
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    a._covers = None
    covers = a.target_covers
    out = {}
    for i, j, gnm, rc in a._iter_target_genomes():
        seqs = [s[::-1].translate(rc_table) if rc else s for s in gnm.seqs]
        off = np.concatenate(([0], np.cumsum([len(s) for s in seqs])))
        n = int(off[-1])
        diff = np.zeros(n + 1, dtype=np.int64)
        arr = np.asarray(covers[i][j][rc], dtype=np.int64).reshape(-1, 2)
        np.add.at(diff, arr[:, 0], 1)
        np.add.at(diff, arr[:, 1], -1)
        unc = np.cumsum(diff[:n]) < 1
        first = np.zeros(n + 1, dtype=bool)
        first[off] = True
        starts = np.flatnonzero(unc & (~np.concatenate(([False], unc[:-1])) | first[:n]))
        ends = np.flatnonzero(unc & (~np.concatenate((unc[1:], [False])) | first[1:])) + 1
        csum = np.concatenate(([0], np.cumsum(np.isin(np.frombuffer("".join(seqs).encode(), dtype=np.uint8), acgt))))
        ua = csum[ends] - csum[starts]
        keep = ua >= 1
        starts, ends, ua = starts[keep], ends[keep], ua[keep]
        seq = np.searchsorted(off, starts, side="right") - 1
        out.setdefault(i, {}).setdefault(j, {})[rc] = list(zip(seq.tolist(), (starts - off[seq]).tolist(),
                                                               (ends - off[seq]).tolist(), ua.tolist()))
    return out


def uncovered_leg(name, scale, repeat, groups, probes):
    from catch_amd import coverage_analysis, engine
    ctx = engine.default_context()
    a = coverage_analysis.Analyzer(probes, 2, 100, groups, cover_extension=50)
    a.run()
    runs = dict(device=[], host=[])
    device_ms, got = [], {}
    for i in range(repeat + 1):                     # the first round warms both paths up
        for m in ("device", "host"):
            ctx.sync()
            t0 = time.perf_counter()
            if m == "device":
                a._uncovered = {}
                got[m] = a.uncovered_regions()
            else:
                got[m] = host_uncovered(a)
            dt = time.perf_counter() - t0
            if i > 0 or repeat == 0:
                runs[m].append(dt)
                if m == "device":
                    device_ms.append(a.last_uncovered_ms)
    bases = sum(g.size() for grp in groups for g in grp)
    regions = sum(len(r) for i in got["device"].values() for j in i.values() for r in j.values())
    # all regions, before the ambiguity filter, set the per-region traffic: count them without it (not timed)
    before = sum(len(r) for i in a.uncovered_regions(1, 1, 0).values() for j in i.values() for r in j.values())

    def spread(v, nd):
        return dict(all=[round(x, nd) for x in v], median=round(statistics.median(v), nd), min=round(min(v), nd),
                    max=round(max(v), nd))
    out = dict(leg="uncovered", input=name, scale=scale if name != "ebola" else None,
               genomes=sum(len(grp) for grp in groups), bases=bases, probes=len(probes), strands=2,
               regions_both_strands=regions, regions_before_filters=before,
               device_wall_s=spread(runs["device"], 4), host_wall_s=spread(runs["host"], 4),
               rows_uncovered_ms_both_strands=spread(device_ms, 3),
               host_over_device=round(statistics.median(runs["host"]) / statistics.median(runs["device"]), 2),
               identical=got["device"] == got["host"],
               # both strands.  Per base: the depth array zeroed (4) and scanned in place (12), read by the threshold
               # (4), the sequence byte (1), the three bitmaps written, zeroed and read again by the count and the
               # emit (8 x 1/8), the two count arrays written, scanned and read (0.625).  Per region: rs / re
               # written (8), read and count + flag written (16), the flags scanned (12), the compaction's reads (20);
               # 16 per reported region.  The atomics per row and the ACGT words of the regions are not in it.
               uncovered_kernel_bytes=int(22.625 * 2 * bases + 56 * before + 16 * regions))
    print(json.dumps(out), flush=True)


def summary(runs):
    tot = [r["total_s"] for r in runs]
    return dict(total_s=[round(t, 4) for t in tot], run_s=[round(r["run_s"], 4) for r in runs],
                write_s=[round(r["write_s"], 4) for r in runs], median_s=round(statistics.median(tot), 4),
                min_s=round(min(tot), 4), max_s=round(max(tot), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--inputs", nargs="+", default=["ebola", "S4"])
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["device", "host"], choices=["device", "host"])
    ap.add_argument("--tree", help="import catch_amd from this checkout instead")
    ap.add_argument("--leg", default="windows", choices=["windows", "uncovered"])
    a = ap.parse_args()
    sys.path.insert(0, a.tree or REPO)
    import numpy as np
    for name in a.inputs:
        np.random.seed(0)
        groups, probes = load(name, a.scale)
        if a.leg == "uncovered":
            uncovered_leg(name, a.scale, a.repeat, groups, probes)
            continue
        bases = sum(g.size() for grp in groups for g in grp)
        genomes = sum(len(grp) for grp in groups)
        windows = sum(-(-g.size() // 25) for grp in groups for g in grp)
        runs = {m: [] for m in a.modes}
        digests = {}
        with tempfile.TemporaryDirectory() as tmp:
            for i in range(a.repeat + 1):               # the first round warms both paths up
                for m in a.modes:
                    r, digests[m] = one(groups, probes, m == "host", os.path.join(tmp, m + ".tsv"))
                    if i > 0 or a.repeat == 0:
                        runs[m].append(r)
        out = dict(input=name, tree=a.tree or "this", scale=a.scale if name != "ebola" else None, genomes=genomes,
                   bases=bases, probes=len(probes), strands=2, windows_per_strand=windows,
                   # per strand: the difference array is zeroed, scanned in place (read + write, twice: tile sums and
                   # apply), turned into tile prefixes (read + write): 4 bytes x (1 + 3 + 2) per base; 12 bytes
                   # written per window; the atomics' 8 bytes per range are not in this figure
                   window_kernel_bytes_per_strand=24 * bases + 12 * windows,
                   **{m: summary(runs[m]) for m in a.modes})
        if len(a.modes) == 2:
            out["host_over_device"] = round(out["host"]["median_s"] / out["device"]["median_s"], 3)
            out["identical_files"] = digests["device"] == digests["host"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
