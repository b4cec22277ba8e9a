#!/usr/bin/env python3
"""Pooling fixture (authoring container only).

Runs the LIVE reference's pool search (its package `catch` importable, e.g.
from a checkout named by CATCH_REFERENCE; needs SciPy) on the reference's own
two probe-count tables, copied as data to tests/golden/pool/:

    num-probes.V-WAfr.201506.tsv       19 datasets x 58-60 grid points
    num-probes.V-All.201606.tsv.gz    296 datasets x 36 grid points

Every run is param_search.standard_search(counts, budget, round_params=(1, 10))
under np.random.seed(s) / random.seed(s) -- what `pool.py COUNTS BUDGET OUT
--round-params 1 10` does -- in a process of its own, one at a time by default
so that reference_wall_s is the search's own time (every run records how many
ran side by side, `jobs`, and the time limit it was given).
tests/golden/pool/reference_runs.json records of EVERY run the budget, the
seed, the parameters chosen per dataset, the count and loss the reference
reports and its wall time; a run that raised or ran out of time is recorded
with what happened instead.  tests/test_pool.py decides which runs qualify
(parameters on the grid, recounted total within the budget) and requires the
exact search to be at least as good as each of them.

    CATCH_REFERENCE=<reference checkout> python tests/golden/make_pool_golden.py

POOL_GOLDEN_VALL_LIMIT_S: time limit of a V-All run (default 3300 s; the search
makes ~600 interpolated evaluations per gradient there).  POOL_GOLDEN_JOBS:
processes side by side (default 1).  POOL_GOLDEN_TABLES: the tables to run
(default "V-All,V-WAfr"); the recorded runs of the others are kept as they are
in reference_runs.json.
"""
import gzip
import json
import multiprocessing
import os
import random
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
POOL = os.path.join(HERE, "pool")
if os.environ.get("CATCH_REFERENCE"):
    sys.path.insert(0, os.environ["CATCH_REFERENCE"])

TABLES = {
    "V-WAfr": "num-probes.V-WAfr.201506.tsv",
    "V-All": "num-probes.V-All.201606.tsv.gz",
}
# (table, budget, seeds, time limit in seconds)
VALL_LIMIT_S = int(os.environ.get("POOL_GOLDEN_VALL_LIMIT_S", "3300"))
PLAN = [
    ("V-All", 350000, (0,), VALL_LIMIT_S),          # first: the long one
    ("V-WAfr", 90000, (0, 1, 2, 3, 4, 5), 1800),     # the reference README's example
    ("V-WAfr", 60000, (0, 1, 2, 3, 4, 5), 1800),
    ("V-WAfr", 45000, (0, 1, 2, 3, 4, 5), 1800),
]
ROUND_PARAMS = (1, 10)


def read_counts(name):
    """The table as the reference's reader returns it (through a plain copy when gzipped)."""
    from catch.utils import pool_probes_io
    path = os.path.join(POOL, TABLES[name])
    if not path.endswith(".gz"):
        return pool_probes_io.read_table_of_probe_counts(path)
    import tempfile
    with gzip.open(path, "rt") as f, tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as g:
        g.write(f.read())
    try:
        return pool_probes_io.read_table_of_probe_counts(g.name)
    finally:
        os.unlink(g.name)


def one_run(table, budget, seed, conn):
    import numpy as np
    from catch.pool import param_search
    _, counts = read_counts(table)
    np.random.seed(seed)
    random.seed(seed)
    t0 = time.perf_counter()
    try:
        params, count, loss = param_search.standard_search(counts, budget, round_params=ROUND_PARAMS)
        r = dict(status="ok", params={d: [float(v) for v in p] for d, p in sorted(params.items())},
                 count=float(count), loss=float(loss))
    except Exception as exc:        # noqa: BLE001 -- recorded, not hidden
        r = dict(status="raised", error="%s: %s" % (type(exc).__name__, str(exc)[:200]))
    r["reference_wall_s"] = round(time.perf_counter() - t0, 2)
    conn.send(r)
    conn.close()


def main():
    import numpy
    import scipy
    jobs = int(os.environ.get("POOL_GOLDEN_JOBS", "1"))
    tables = os.environ.get("POOL_GOLDEN_TABLES", "V-All,V-WAfr").split(",")
    plan = [(t, b, s, lim) for t, b, seeds, lim in PLAN for s in seeds]
    order = {(t, b, s): i for i, (t, b, s, _) in enumerate(plan)}
    pending, running, runs = [x for x in plan if x[0] in tables], [], []
    out_path = os.path.join(POOL, "reference_runs.json")
    if os.path.exists(out_path):          # the runs of tables not selected stay as recorded
        with open(out_path) as f:
            runs = [r for r in json.load(f)["runs"] if r["table"] not in tables]

    def save():
        runs.sort(key=lambda r: order[(r["table"], r["budget"], r["seed"])])
        with open(out_path, "w") as f:
            json.dump(dict(search="param_search.standard_search(counts, budget, round_params=[1, 10]) under "
                                  "np.random.seed(seed), random.seed(seed)",
                           tables=TABLES, round_params=list(ROUND_PARAMS), python=sys.version.split()[0],
                           numpy=numpy.__version__, scipy=scipy.__version__, runs=runs), f, indent=1)
            f.write("\n")

    while pending or running:
        while pending and len(running) < jobs:
            t, b, s, lim = pending.pop(0)
            parent, child = multiprocessing.Pipe(False)
            p = multiprocessing.Process(target=one_run, args=(t, b, s, child))
            p.start()
            running.append((p, parent, t, b, s, lim, time.perf_counter()))
        for entry in list(running):
            p, parent, t, b, s, lim, t0 = entry
            r = None
            if parent.poll(0):
                r = parent.recv()
                p.join()
            elif time.perf_counter() - t0 > lim:
                p.terminate()
                p.join()
                r = dict(status="timeout", error="no result within the %d s given to this run" % lim,
                         reference_wall_s=None)
            elif not p.is_alive():
                p.join()
                r = dict(status="raised", error="the process ended with exit code %s" % p.exitcode,
                         reference_wall_s=None)
            if r is not None:
                running.remove(entry)
                r.update(table=t, budget=b, seed=s, jobs=jobs, time_limit_s=lim)
                runs.append(r)
                sys.stderr.write(json.dumps({k: v for k, v in r.items() if k != "params"}) + "\n")
                save()
        time.sleep(0.5)


if __name__ == "__main__":
    main()
