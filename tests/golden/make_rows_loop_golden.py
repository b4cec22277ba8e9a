"""Records what SetCoverFilter._filter_strs selects and reports for every combination of the options that keep a
group's cover rows on the device (fixed_probes, coverage_depth, prune_redundant, pick_gains / max_probes), so that a
change of the host code that drives them can be replayed against the commit before it:

    python tests/golden/make_rows_loop_golden.py --recorded-at <commit id> --out tests/golden/rows_loop_parent.json.gz

(on a machine with the GPU, in a checkout of the commit to record, library built).  tests/test_rows_loop.py imports
`configurations` and `run` from here and compares field by field.  Input: the first five genomes of the Ebola fixture
and their candidates, as tests/test_extend_probes.py builds them, in two groups of different size -- (all candidates,
five genomes) and (every second candidate, three genomes) -- so that the order of the groups and the budget's merge
over them matter.  Data only: no float is kept (of last_timings the keys and the integer counters)."""
import argparse
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

POINTS = ((0, 1.0), (50, 0.9))          # (cover_extension, coverage)
GAINS = ("none", "pick_gains", "max_probes")
COUNTERS = ("rows", "rows_fixed", "rows_reduced", "picks", "pruned", "prune_rounds")
DEVICE_MS = ("scan_ms", "greedy_ms", "depth_ms", "prune_ms", "gains_ms")


def configurations():
    """The 29 runs, in the order they are recorded."""
    options = []
    for depth in (1, 2):
        for prune in (False, True):
            for gains in (GAINS if depth == 1 else GAINS[:1]):       # (gains with a depth above 1 are refused)
                options.append(dict(fixed=False, depth=depth, prune=prune, gains=gains))
    for prune in (False, True):
        for gains in GAINS:
            options.append(dict(fixed=True, depth=1, prune=prune, gains=gains))
    out = [dict(o, cover_extension=e, coverage=c, avoided=False) for o in options for e, c in POINTS]
    out.append(dict(fixed=False, depth=2, prune=True, gains="none", cover_extension=50, coverage=0.9, avoided=True))
    return out


def inputs():
    from test_extend_probes import _candidates, _genomes
    g5 = _genomes(5)
    c5 = _candidates(g5)
    return g5, c5


def write_avoided(directory, g5):
    """One FASTA holding the first genome."""
    path = os.path.join(str(directory), "avoided.fasta")
    with open(path, "w") as f:
        for i, s in enumerate(g5[0].seqs):
            f.write(">avoided_%d\n%s\n" % (i, s))
    return path


def run(cfg, g5, c5, avoided_path):
    """One run -> (the record, last_timings)."""
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    kw = {}
    if cfg["fixed"]:
        kw["fixed_probes"] = c5[:3]
    if cfg["depth"] != 1:
        kw["coverage_depth"] = cfg["depth"]
    if cfg["prune"]:
        kw["prune_redundant"] = True
    if cfg["gains"] == "pick_gains":
        kw["pick_gains"] = True
    elif cfg["gains"] == "max_probes":
        kw["max_probes"] = 40
    if cfg["avoided"]:
        kw["avoided_genomes"] = [avoided_path]
    f = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=cfg["coverage"],
                       cover_extension=cfg["cover_extension"], **kw)
    np.random.seed(20)
    selection = f._filter_strs([c5, c5[::2]], [g5, g5[:3]], assume_unique=True)
    t = f.last_timings
    rec = dict(config=cfg,
               selection=selection,
               last_layer_sizes=f.last_layer_sizes,
               last_pruned=f.last_pruned,
               last_budget_kept=f.last_budget_kept,
               last_pick_gains=[np.asarray(g).tolist() for g in f.last_pick_gains],
               last_coverage_curve=f.last_coverage_curve,
               timings_keys=sorted(t),
               counters={k: int(t[k]) for k in COUNTERS if k in t})
    return json.loads(json.dumps(rec, default=int)), t       # (tuples as lists, NumPy integers as ints: what the file holds)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--recorded-at", required=True, help="the commit id of the checkout this runs in")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    g5, c5 = inputs()
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        avoided = write_avoided(tmp, g5)
        for cfg in configurations():
            rec, t = run(cfg, g5, c5, avoided)
            runs.append(rec)
            print(json.dumps(cfg, sort_keys=True), "picks", [len(s) for s in rec["selection"]],
                  " ".join("%s %.3f" % (k, t[k]) for k in DEVICE_MS if k in t), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with gzip.GzipFile(args.out, "wb", mtime=0) as f:
        f.write(json.dumps(dict(recorded_at=args.recorded_at, runs=runs), sort_keys=True).encode())
    print("%d runs -> %s" % (len(runs), args.out))


if __name__ == "__main__":
    main()
