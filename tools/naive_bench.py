#!/usr/bin/env python3
"""Times of design_naively's device path on the config-2 shape: the unique
candidates of synthetic.dataset("S2") at -pl 100 -ps 50 (22,280 at scale 1),
under the longest-common-substring predicate of `-nrf 3 80` / `-dsf 3 80`.

Prints one JSON line: the redundancy graph (wall seconds, the kernels' GPU
milliseconds, pairs per second, redundant pairs), the naive pass, the
dominating-set rows + greedy solve, the probes each filter keeps, and the pair
kernel's instruction model (DESIGN.md §4 "Naive baseline": diagonals looked at
x words per plane x instructions per word) for a fraction of the integer-VALU
peak over a measured time.  Best of --repeat after one warm-up.

    python tools/naive_bench.py [--scale 1.0] [--repeat 2] [--mismatches 3] [--lcf-thres 80]
    rocprofv3 --kernel-trace --stats -- python tools/naive_bench.py --only-graph
        (rg_pairs_kernel's time in the kernel statistics / pairs = seconds per pair)
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from catch_amd import engine  # noqa: E402
from catch_amd.filter import candidate_probes  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

# per diagonal and 64-base word of the pair kernel (csrc/redundant.hip, rg_pair): 3 planes x (2 LDS reads of the
# shifted operand + 1 of the other, a 64-bit funnel shift = 6, xor + or = 4 32-bit ops) + mask 6 + popcount 4
INSTR_PER_WORD = 3 * (3 + 6 + 4) + 6 + 4
INT_VALU_PEAK = 256 * 4 * 32 * 2.4e9        # lanes x clock: 32-bit integer operations per second of one MI355X


def candidates(scale, probe_length, probe_stride):
    out = []
    for grp in synthetic.dataset("S2", scale=scale):
        for g in grp:
            out += candidate_probes.candidate_strings_from_sequences(["".join(s) for s in g], probe_length, probe_stride)
    return list(dict.fromkeys(out))


def best_of(fn, repeat):
    best, val = None, None
    for i in range(repeat + 1):
        t0 = time.perf_counter()
        val = fn()
        dt = time.perf_counter() - t0
        if i > 0 or repeat == 0:
            best = dt if best is None else min(best, dt)
    return best, val


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--mismatches", type=int, default=3)
    ap.add_argument("--lcf-thres", type=int, default=80)
    ap.add_argument("-pl", "--probe-length", type=int, default=100)
    ap.add_argument("-ps", "--probe-stride", type=int, default=50)
    ap.add_argument("--only-graph", action="store_true", help="one graph build, nothing else (for a kernel trace)")
    a = ap.parse_args()
    strs = candidates(a.scale, a.probe_length, a.probe_stride)
    n = len(strs)
    pairs = n * (n - 1) // 2
    ctx = engine.default_context()
    graphs = []

    def build():
        for g in graphs:
            g.close()
        graphs[:] = [engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, a.mismatches, a.lcf_thres)]
        return ctx.kernel_ms(engine.PHASE_NDF)[0]
    graph_s, graph_ms = best_of(build, 0 if a.only_graph else a.repeat)
    g = graphs[0]
    words = 1 if a.probe_length <= 64 else 2 if a.probe_length <= 128 else 4
    diagonals = 2 * max(0, a.probe_length - a.lcf_thres) + 1
    model = diagonals * words * INSTR_PER_WORD
    out = dict(candidates=n, pairs=pairs, mismatches=a.mismatches, lcf_thres=a.lcf_thres,
               redundant_pairs=g.nedges // 2, graph_s=round(graph_s, 4), graph_kernels_ms=round(graph_ms, 3),
               pairs_per_s=round(pairs / (graph_ms / 1e3)) if graph_ms else None,
               model_instr_per_pair=model,
               model_fraction_of_int_valu_peak=(round(pairs * model / (graph_ms / 1e3) / INT_VALU_PEAK, 4)
                                                if graph_ms else None))
    if not a.only_graph:
        naive_s, keep = best_of(g.naive, a.repeat)
        out.update(naive_s=round(naive_s, 4), naive_kernels_ms=round(ctx.kernel_ms(engine.PHASE_NDF)[0], 3),
                   naive_kept=int(keep.sum()))

        def solve():
            rows = g.rows()
            try:
                return rows.n, rows.greedy(n)
            finally:
                rows.close()
        solve_s, (nrows, picks) = best_of(solve, a.repeat)
        out.update(dominating_rows=nrows, dominating_solve_s=round(solve_s, 4),
                   solver_kernels_ms=round(ctx.kernel_ms(engine.PHASE_GREEDY)[0], 3), dominating_kept=len(picks))
    g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
