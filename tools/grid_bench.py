#!/usr/bin/env python3
"""Wall time of a grid design (catch_amd.grid) against the same grid with
CATCHHIP_GRID_RESCAN=1 (a fresh cover scan at every cover extension), on two
shapes over the V-All grid (m 0-5 x e 0, 10, ..., 50):

  S4: synthetic.dataset("S4")'s 20 groups as 20 datasets
  S2: synthetic.dataset("S2")'s 2 groups as 2 datasets

Prints one JSON line per shape: grid and rescan wall seconds (best of
--repeat after one warm-up), scans / derived tables / solves of each, and
whether the two selected the same probes at every point.

    python tools/grid_bench.py [--shapes S4 S2] [--repeat 2] [--scale 1.0]
"""
import argparse
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("CATCHHIP_TEST_HOOKS", "1")     # the rescan switch is a test hook

import numpy as np  # noqa: E402
from catch_amd import genome, grid  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

MS = [0, 1, 2, 3, 4, 5]
ES = [0, 10, 20, 30, 40, 50]


def datasets_of(shape, scale):
    return [[genome.Genome.from_one_seq("".join(g)) for g in grp]
            for grp in synthetic.dataset(shape, scale=scale)]


def timed(datasets, rescan, repeat):
    if rescan:
        os.environ["CATCHHIP_GRID_RESCAN"] = "1"
    else:
        os.environ.pop("CATCHHIP_GRID_RESCAN", None)
    best, out, st = None, None, {}
    for i in range(repeat + 1):
        st = {}
        np.random.seed(0)      # m >= 5 at -pl 100 draws random anchors: every run from the same states
        random.seed(0)
        t0 = time.perf_counter()
        out = grid.design_grid(datasets, MS, ES, stats=st)
        dt = time.perf_counter() - t0
        if i > 0 and (best is None or dt < best):
            best = dt
    return best, out, st


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=["S4", "S2"])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only-grid", action="store_true", help="one grid run, no rescan (for a kernel trace)")
    ap.add_argument("--ms", type=int, nargs="+", default=MS, help="the mismatch values (default 0-5)")
    a = ap.parse_args()
    MS[:] = a.ms
    for shape in a.shapes:
        ds = datasets_of(shape, a.scale)
        bases = sum(g.size() for d in ds for g in d)
        if a.only_grid:
            t, _, st = timed(ds, False, 0)
            print(json.dumps(dict(shape=shape, datasets=len(ds), bases=bases, grid_s=round(t or 0.0, 4), grid=st)))
            continue
        tg, og, sg = timed(ds, False, a.repeat)
        tr, orr, sr = timed(ds, True, a.repeat)
        print(json.dumps(dict(shape=shape, datasets=len(ds), bases=bases, ms=MS, es=ES, points=len(og),
                              probes=sum(len(v) for v in og.values()),
                              grid_s=round(tg, 4), rescan_s=round(tr, 4), speedup=round(tr / tg, 3),
                              grid=sg, rescan=sr, equal=og == orr)), flush=True)


if __name__ == "__main__":
    main()
