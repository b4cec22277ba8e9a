#!/usr/bin/env python3
"""Timing of the clustering pre-step (catch_amd/csrc/cluster.hip) on a synthetic
input: signatures, one distance row, the condensed matrix, and the whole
cluster_with_minhash_signatures for both methods -- the hierarchical one with
the average linkage on the device and on the host (CATCHHIP_CLUSTER_HOST_LINKAGE),
and the linkage stage alone for both.

    python tools/cluster_bench.py [--workload S4] [--scale 0.25] [--fragment 50000]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from catch_amd import engine                      # noqa: E402
from catch_amd.genome import Genome               # noqa: E402
from catch_amd.utils import cluster, lsh, synthetic   # noqa: E402

PHASE_NDF = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S4")
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--fragment", type=int, default=50000)
    ap.add_argument("--cpu-sample", type=int, default=200000,
                    help="bases hashed by a hashlib loop for comparison (0 = skip)")
    ap.add_argument("--hierarchical-max", type=int, default=12000)
    ap.add_argument("--max-sequences", type=int, default=0,
                    help="cluster only the first so many fragments (0 = all): a chosen n for the linkage timings")
    ap.add_argument("--repeat", type=int, default=3, help="runs of every clustering; the best is reported")
    a = ap.parse_args()
    groups = synthetic.dataset(a.workload, scale=a.scale)
    seqs = []
    for grp in groups:
        for g in grp:
            for s in g:
                seqs += Genome.from_one_seq(s).break_into_fragments(
                    a.fragment, include_full_end=True).seqs
    total = sum(len(s) for s in seqs)
    ctx = engine.default_context()
    out = dict(workload=a.workload, scale=a.scale, sequences=len(seqs), bases=total)
    fam = lsh.MinHashFamily(12, N=100)
    random.seed(1)
    fam.signatures(seqs[:4]).close()               # warm up (module load, pool)
    t0 = time.perf_counter()
    sigs = fam.signatures(seqs)
    out["signatures_wall_s"] = time.perf_counter() - t0
    ms, n = ctx.kernel_ms(PHASE_NDF)
    out["signatures_kernel_ms"] = ms
    # algorithmic bytes: 1 B/base read + 4 B/k-mer hash written, then the select
    # reads every hash 4 times (3 histogram levels + gather)
    out["signatures_GBps"] = total * (1 + 4 + 16) / (ms * 1e-3) / 1e9
    out["kmers_per_s"] = total / (ms * 1e-3)
    rows = []
    for j in range(0, len(seqs), max(1, len(seqs) // 20)):
        t0 = time.perf_counter()
        sigs.common_row(j)
        rows.append(time.perf_counter() - t0)
    out["row_wall_ms"] = 1e3 * float(np.median(rows))
    out["row_kernel_ms"] = ctx.kernel_ms(PHASE_NDF)[0]
    if len(seqs) <= a.hierarchical_max:
        lut = (1.0 - np.arange(101, dtype=np.float64) / 100.0).astype(np.float32)
        t0 = time.perf_counter()
        dm = sigs.condensed(lut)
        out["condensed_wall_s"] = time.perf_counter() - t0
        out["condensed_kernel_ms"] = ctx.kernel_ms(PHASE_NDF)[0]
        out["pairs"] = int(dm.size)
        out["pairs_per_s"] = dm.size / (out["condensed_kernel_ms"] * 1e-3)
    sigs.close()
    named = dict(enumerate(seqs))
    if a.max_sequences and len(seqs) > a.max_sequences:
        named = dict(enumerate(seqs[:a.max_sequences]))
    out["clustered_sequences"] = len(named)
    # (method, key prefix, environment): the hierarchical method with the linkage on the device and, under the
    # CATCHHIP_CLUSTER_HOST_LINKAGE test hook, on the host (condensed float32 matrix + SciPy: the path until now)
    runs = [("simple", "simple", {})]
    if len(named) <= a.hierarchical_max:
        runs += [("hierarchical", "hierarchical", {}),
                 ("hierarchical", "hierarchical_host", {"CATCHHIP_CLUSTER_HOST_LINKAGE": "1"})]
    os.environ["CATCHHIP_TEST_HOOKS"] = "1"
    for method, key, env in runs:
        walls, stages = [], []
        for _ in range(max(1, a.repeat)):
            for k, v in env.items():
                os.environ[k] = v
            try:
                random.seed(1)
                t0 = time.perf_counter()
                cl = cluster.cluster_with_minhash_signatures(named, threshold=0.15, cluster_method=method)
                walls.append(time.perf_counter() - t0)
            finally:
                for k in env:
                    os.environ.pop(k, None)
            stages.append(dict(cluster.last_timings, kernel_ms=ctx.kernel_ms(PHASE_NDF)[0]))
        out[key + "_wall_s"] = min(walls)                      # best of --repeat (the first run is the cold one)
        out[key + "_wall_s_all"] = walls
        out[key + "_clusters"] = len(cl)
        out[key + "_largest"] = [len(c) for c in cl[:5]]
        if method == "hierarchical":
            # the linkage stage alone: distances + linkage + flat clusters (everything after the signatures)
            out[key + "_linkage"] = stages[-1]["linkage"]
            out[key + "_linkage_s"] = min(s["linkage_s"] for s in stages)
            if stages[-1]["linkage"] == "device":       # matrix fill + chain, by the device's events
                out[key + "_linkage_kernel_ms"] = min(s["kernel_ms"] for s in stages)
            if "condensed_s" in stages[-1]:
                out[key + "_condensed_s"] = min(s["condensed_s"] for s in stages)
            out[key + "_result"] = [len(c) for c in cl]
    if "hierarchical_result" in out:
        out["hierarchical_paths_agree"] = out.pop("hierarchical_result") == out.pop("hierarchical_host_result")
        out["linkage_host_over_device"] = out["hierarchical_host_linkage_s"] / out["hierarchical_linkage_s"]
    if a.cpu_sample:
        import hashlib
        import heapq
        sample, got = [], 0
        for s in seqs:
            sample.append(s)
            got += len(s)
            if got >= a.cpu_sample:
                break
        t0 = time.perf_counter()
        for s in sample:      # the same arithmetic, one core, stdlib only
            heapq.nsmallest(100, ((12345 * int(hashlib.md5(s[i:i + 12].encode()).hexdigest(), 16) + 678)
                                  % (2 ** 31 - 1) for i in range(len(s) - 11)))
        dt = time.perf_counter() - t0
        out["cpu_signature_kmers_per_s"] = got / dt
        out["cpu_sample_bases"] = got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
