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

    python tools/analysis_bench.py [--inputs ebola S4] [--scale 0.05] [--repeat 3]
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
    a = ap.parse_args()
    sys.path.insert(0, a.tree or REPO)
    import numpy as np
    for name in a.inputs:
        np.random.seed(0)
        groups, probes = load(name, a.scale)
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
