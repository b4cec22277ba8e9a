#!/usr/bin/env python3
"""Grid-design parity fixture (authoring container only).

Runs the LIVE reference (its package `catch` importable, e.g. from a checkout
named by CATCH_REFERENCE) once per
point of a small mismatches x cover-extension grid -- what the reference
README's option #3 does with design.py -- over the first 30 records of
tests/golden/ebola_zaire_100.fasta.gz (made by make_real_golden.py):
candidate probes (-pl 100, stride 50) -> DuplicateFilter -> SetCoverFilter at
m in {0, 1, 2, 3}, e in {0, 25, 50}.  Records every point's probe count and the
digest of its sorted picks in tests/golden/grid_runs.json, in table order
(m, then e), so that the grid design's table and picks can be checked against
the reference without running it.

    PYTHONHASHSEED=0 CATCH_REFERENCE=<reference checkout> python tests/golden/make_grid_golden.py
"""
import hashlib
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if os.environ.get("CATCH_REFERENCE"):
    sys.path.insert(0, os.environ["CATCH_REFERENCE"])

from catch.filter import candidate_probes  # noqa: E402
from catch.filter import duplicate_filter  # noqa: E402
from catch.filter import set_cover_filter as scf  # noqa: E402
from catch.utils import seq_io  # noqa: E402

FASTA = os.path.join(HERE, "ebola_zaire_100.fasta.gz")
RECORDS, PL, PS = 30, 100, 50
MISMATCHES = (0, 1, 2, 3)
EXTENSIONS = (0, 25, 50)


def main():
    genomes = seq_io.read_genomes_from_fasta(FASTA)[:RECORDS]
    cands = []
    for g in genomes:
        cands += candidate_probes.make_candidate_probes_from_sequences(
            g.seqs, probe_length=PL, probe_stride=PS)
    cands = duplicate_filter.DuplicateFilter().filter(cands)
    points = []
    for m in MISMATCHES:
        for e in EXTENSIONS:
            f = scf.SetCoverFilter(mismatches=m, lcf_thres=PL, coverage=1.0, cover_extension=e)
            t0 = time.perf_counter()
            out = f.filter([cands], [genomes], input_is_grouped=True)
            wall = time.perf_counter() - t0
            sel = sorted(p.seq_str for p in out[0])
            r = dict(mismatches=m, cover_extension=e, num_probes=len(sel),
                     picks_sha256=hashlib.sha256(",".join(sel).encode()).hexdigest(),
                     reference_wall_s=round(wall, 2))
            points.append(r)
            sys.stderr.write(json.dumps(r) + "\n")
            sys.stderr.flush()
            with open(os.path.join(HERE, "grid_runs.json"), "w") as f:
                json.dump(dict(fasta=os.path.basename(FASTA), records=RECORDS, probe_length=PL, probe_stride=PS,
                               lcf_thres=PL, coverage=1.0, P=len(cands),
                               G=sum(g.size() for g in genomes), python=sys.version.split()[0],
                               hashseed=os.environ.get("PYTHONHASHSEED"), points=points), f, indent=1)


if __name__ == "__main__":
    main()
