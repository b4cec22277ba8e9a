#!/usr/bin/env python3
"""Times catchhip_pool_solve (csrc/pool.hip) beside a NumPy statement of the same dynamic programme.

    python tools/pool_bench.py [--cases vall350 vall700 synth588] [--repeats 3] [--numpy-datasets N] [--out F.json]

Cases: vall350 / vall700 = the reference's V-All table (tests/golden/pool/, 296 datasets x 36 grid points) at budgets
of 350,000 and 700,000; synth588 = a seeded table of 588 datasets x 1,000 options at 700,000.  Per case, after one
warm-up call: the host wall time of engine.pool_solve (ends in a stream synchronisation) and the kernel time between
the events around its launches (catchhip_ctx_last_kernel_ms, phase 8), the best and the median of --repeats calls.
The NumPy programme runs on all of V-All and on the first 12 datasets of synth588 (--numpy-datasets N: on the first N,
0 = all; its cost is the same for every dataset of equal size, and the figure for all D is labelled an extrapolation
when it is one) and, when it ran on all of them,
its answer must equal the kernel's.  The reference's own search time comes from tests/golden/pool/reference_runs.json.
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden", "pool")


def numpy_dp(off, cnt, loss, B, datasets):
    """f and the choice table of the first `datasets` datasets -> (f, table)."""
    prev = np.zeros(B + 1, dtype=np.float64)
    table = []
    for i in range(datasets):
        cur = np.full(B + 1, np.inf)
        ch = np.full(B + 1, 0xffff, dtype=np.uint16)
        for k in range(int(off[i]), int(off[i + 1])):
            n = int(cnt[k])
            if n > B:
                continue
            cand = prev[:B + 1 - n] + loss[k]
            seg, cseg = cur[n:], ch[n:]
            better = cand < seg
            seg[better] = cand[better]
            cseg[better] = k - int(off[i])
        table.append(ch)
        prev = cur
    return prev, table


def vall():
    from catch_amd import pool
    with gzip.open(os.path.join(GOLDEN, "num-probes.V-All.201606.tsv.gz"), "rt") as f:
        text = f.read()
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as g:
        g.write(text)
    try:
        names, counts = pool.read_probe_counts(g.name)
    finally:
        os.unlink(g.name)
    _, off, _, cnt, loss = pool.options(counts, pool.default_loss_coeffs(names))
    return off, cnt, loss


def synth(D=588, K=1000, seed=588):
    """Counts fall with the loss on the whole (a looser point needs fewer probes), noisy, many repeats."""
    rng = np.random.default_rng(seed)
    off = np.arange(D + 1, dtype=np.int64) * K
    size = rng.integers(300, 6000, size=D)
    loss = np.sort(rng.integers(0, 400, size=(D, K)) / 4.0, axis=1)
    frac = 1.0 / (1.0 + loss / 12.0) * rng.uniform(0.85, 1.15, size=(D, K))
    cnt = np.maximum((size[:, None] * frac).astype(np.int64) // 4 * 4, 1)
    return off, cnt.reshape(-1), loss.reshape(-1)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--cases", nargs="+", default=["vall350", "vall700", "synth588"])
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--numpy-datasets", type=int, default=None,
                   help="datasets the NumPy programme runs on (0 = all; default: all of V-All, 12 of synth588)")
    p.add_argument("--out")
    args = p.parse_args()
    from catch_amd import engine
    ctx = engine.default_context()
    inputs = {}
    results = []
    for case in args.cases:
        key = "synth" if case.startswith("synth") else "vall"
        if key not in inputs:
            inputs[key] = synth() if key == "synth" else vall()
        off, cnt, loss = inputs[key]
        B = {"vall350": 350000, "vall700": 700000, "synth588": 700000}[case]
        D = len(off) - 1
        engine.pool_solve(ctx, off, cnt, loss, B)                       # warm-up: code objects, the block cache
        wall, kern = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            choice, total, best = engine.pool_solve(ctx, off, cnt, loss, B)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ctx.kernel_ms(engine.PHASE_POOL)[0])
        want = args.numpy_datasets if args.numpy_datasets is not None else (12 if key == "synth" else 0)
        nd = D if want <= 0 else min(D, want)
        t0 = time.perf_counter()
        f, table = numpy_dp(off, cnt, loss, B, nd)
        numpy_s = time.perf_counter() - t0
        r = dict(case=case, datasets=D, options=int(off[-1]), budget=B, cell_updates=int(off[-1]) * (B + 1),
                 total=total, loss=best, wall_ms_best=round(min(wall), 3), wall_ms_median=round(float(np.median(wall)), 3),
                 kernel_ms_best=round(min(kern), 3), kernel_ms_median=round(float(np.median(kern)), 3),
                 launches=int(ctx.kernel_ms(engine.PHASE_POOL)[1]), numpy_datasets=nd, numpy_s=round(numpy_s, 3))
        r["cell_updates_per_s_kernel"] = round(r["cell_updates"] / (min(kern) * 1e-3), 0)
        if nd == D:
            b, same = B, float(f[B]) == best
            for i in range(D - 1, -1, -1):
                k = int(table[i][b])
                same = same and k == int(choice[i])
                b -= int(cnt[int(off[i]) + k])
            r["numpy_equal"] = bool(same and B - b == total)
        else:
            r["numpy_s_all_datasets_extrapolated"] = round(numpy_s * float(off[-1]) / float(off[nd]), 1)
        path = os.path.join(GOLDEN, "reference_runs.json")
        if key == "vall" and os.path.exists(path):
            with open(path) as fh:
                runs = [x for x in json.load(fh)["runs"] if x["table"] == "V-All" and x["budget"] == B]
            r["reference_runs"] = [dict(status=x["status"], seed=x["seed"], reference_wall_s=x["reference_wall_s"],
                                        jobs=x.get("jobs"), time_limit_s=x.get("time_limit_s"), loss=x.get("loss"))
                                   for x in runs]
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(pool_stats=engine.pool_stats(), results=results), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
