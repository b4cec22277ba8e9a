#!/usr/bin/env python3
"""Fixture of the design command's optional filters (authoring container only).

Runs the LIVE reference (a checkout named by CATCH_REFERENCE: its package
`catch` and its bin/design.py) and records, as data only, in
tests/golden/design_filters.json.gz:

  (a) polya     PolyAFilter keep/drop per string over ACGTN: lengths 8-130,
                A/T-heavy compositions, every combination of length in
                {4, 12, L, L+1}, mismatches in {0, 1, 2, 4}, gate 0 and 6;
                stretches at the first base, at the last base and across the
                middle; >= 50 cases that the gate alone decides
  (b) fasta     FastaFilter: a file with repeated sequences (the last index
                wins), repeated candidates, 'reverse complement' headers with
                and without skipping, candidates absent from the file
  (c) nexp      NExpansionFilter with random.seed recorded: probes with
                0, 1, 2, 3 and 5 N; limits None, 0, 1, 3
  (d) rc        ReverseComplementFilter: sequences and both headers
  (e) options   nargs, type name, default and const of the seven options, read
                from the parser bin/design.py builds
  (f) runs      bin/design.py end to end (-pl 100 -ps 50 -m 2 -e 50) on the
                first records of ebola_zaire_100.fasta.gz and on the synthetic
                design_filters_n.fasta this script writes (isolated N, at most
                2 per window: --expand-n draws nothing there); per run the
                output FASTA's (header, sequence) records, sorted, and stdout

    PYTHONHASHSEED=0 CATCH_REFERENCE=<reference checkout> python tests/golden/make_design_filters_golden.py
"""
import argparse
import contextlib
import gzip
import importlib.util
import io
import json
import os
import random
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["CATCH_REFERENCE"]
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
from catch import probe  # noqa: E402
from catch.filter import fasta_filter, n_expansion_filter  # noqa: E402
from catch.filter import polya_filter, reverse_complement_filter  # noqa: E402

EBOLA = os.path.join(HERE, "ebola_zaire_100.fasta.gz")
N_FASTA = os.path.join(HERE, "design_filters_n.fasta")
OPTIONS = ("--filter-polya", "--filter-from-fasta", "--skip-set-cover", "--expand-n",
           "--add-reverse-complements", "--limit-target-genomes",
           "--limit-target-genomes-randomly-with-replacement")


def load_design():
    spec = importlib.util.spec_from_file_location("reference_design", os.path.join(REF, "bin", "design.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# -- (a) ------------------------------------------------------------------
def polya_cases(rng):
    def window_hit(s, length, k):
        return any(sum(c != b for c in s[i:i + length]) <= k
                   for b in "AT" for i in range(len(s) - length + 1))

    strings = []
    comps = ([5, 1, 1, 1, 0.2], [1, 5, 1, 1, 0.2], [3, 3, 1, 1, 0.5], [8, 1, 0.5, 0.5, 0.1], [1, 1, 1, 1, 0.1])
    for _ in range(1500):
        L = rng.choice([8, 9, 12, 13, 20, 33, 63, 64, 65, 100, 101, 130])
        strings.append("".join(rng.choices("ATCGN", weights=rng.choice(comps), k=L)))
    for _ in range(360):
        # a planted stretch (some characters spoilt) at the first base, at the last base or across the middle
        L = rng.choice([20, 33, 64, 65, 100, 130])
        s = rng.choices("ACGTN", weights=[2, 2, 2, 2, 0.3], k=L)
        n = rng.randrange(4, min(L, 40))
        at = rng.choice([0, L - n, (L - n) // 2])
        base = rng.choice("AT")
        for j in range(at, at + n):
            s[j] = base if rng.random() > 0.1 else rng.choice("CGN")
        strings.append("".join(s))
    for _ in range(200):
        # runs of five, never six: the window rule is met where only the gate keeps the probe
        L = rng.choice([24, 64, 100, 130])
        base = rng.choice("AT")
        s = ""
        while len(s) < L:
            s += base * rng.randrange(3, 6) + rng.choice("CGN" + ("T" if base == "A" else "A"))
        strings.append(s[:L])
    rng.shuffle(strings)
    combos = [(ln, mm, gate) for ln in ("4", "12", "L", "L+1") for mm in (0, 1, 2, 4) for gate in (0, 6)]
    out, gate_decides = [], 0
    for i, s in enumerate(strings):
        ln, mm, gate = combos[i % len(combos)]
        length = {"4": 4, "12": 12, "L": len(s), "L+1": len(s) + 1}[ln]
        f = polya_filter.PolyAFilter(length, mm, min_exact_length_to_consider=gate)
        kept = len(f._filter([probe.Probe.from_str(s)])) == 1
        if kept and window_hit(s, length, mm):
            gate_decides += 1
        out.append([s, length, mm, gate, kept])
    assert gate_decides >= 50, gate_decides
    return dict(cases=out, gate_decides=gate_decides)


# -- (b) ------------------------------------------------------------------
def fasta_cases(rng, tmp):
    def seq(n=30):
        return "".join(rng.choices("ACGT", k=n))
    s = [seq() for _ in range(9)]
    records = [("p0", s[0]), ("p1", s[1]), ("p2 | reverse complement of p1", s[2]), ("p3", s[3]),
               ("p4", s[1]),                                   # s[1] again: its rank is this record's index
               ("p5 | reverse complement of p3", s[4]), ("p6", s[5]),
               ("p7 | reverse complement of p6", s[0]),        # s[0] last under a skipped header
               ("p8", s[6])]
    text = "".join(">%s\n%s\n" % r for r in records)
    path = os.path.join(tmp, "keep.fasta")
    with open(path, "w") as f:
        f.write(text)
    cands = [s[6], s[3], s[7], s[1], s[0], s[2], s[1], s[8], s[4], s[5], s[0], s[6]]
    out = {}
    for skip in (False, True):
        f = fasta_filter.FastaFilter(path, skip_reverse_complements=skip)
        out["skip" if skip else "all"] = [p.seq_str for p in f._filter([probe.Probe.from_str(c) for c in cands])]
    return dict(fasta=text, candidates=cands, kept=out)


# -- (c) ------------------------------------------------------------------
def nexp_cases(rng):
    def with_n(count, L=24):
        s = rng.choices("ACGT", k=L)
        for j in rng.sample(range(L), count):
            s[j] = "N"
        return "".join(s)
    probes = [with_n(c) for c in (0, 1, 2, 3, 5, 0, 2, 5, 1, 3)]
    cases = []
    for limit in (None, 0, 1, 3):
        for seed in (1, 2):
            random.seed(seed)
            f = n_expansion_filter.NExpansionFilter(limit_n_expansion_randomly=limit)
            out = f._filter([probe.Probe.from_str(p) for p in probes])
            cases.append(dict(limit=limit, seed=seed, out=[p.seq_str for p in out],
                              next_draw=random.random()))      # (the state the draws leave behind)
    return dict(probes=probes, cases=cases)


# -- (d) ------------------------------------------------------------------
def rc_cases(rng):
    probes = ["".join(rng.choices("ACGT", k=20)) for _ in range(4)]
    probes.append("ACGTNACCGTNNTTAGC")
    f = reverse_complement_filter.ReverseComplementFilter()
    out = f._filter([probe.Probe.from_str(p) for p in probes])
    return dict(probes=probes, out=[[p.header, p.seq_str] for p in out])


# -- (e) ------------------------------------------------------------------
def option_surface(design):
    caught = []

    class Caught(Exception):
        pass

    def grab(self, *a, **k):
        caught.append(self)
        raise Caught()
    real = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = grab
    try:
        design.init_and_parse_args(args_type="basic")
    except Caught:
        pass
    finally:
        argparse.ArgumentParser.parse_args = real
    out = []
    for act in caught[0]._actions:
        for opt in OPTIONS:
            if opt in act.option_strings:
                out.append(dict(option=opt, nargs=act.nargs, type=act.type.__name__ if act.type else None,
                                default=act.default, const=act.const, dest=act.dest))
    assert len(out) == len(OPTIONS)
    return out


# -- (f) ------------------------------------------------------------------
def read_records(path):
    recs, cur = [], None
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                cur = [line[1:], ""]
                recs.append(cur)
            elif cur is not None:
                cur[1] += line
    return recs


def run_design(design, tmp, name, dataset, options, seed):
    out_fn = os.path.join(tmp, name + ".fasta")
    argv = ["design.py", dataset, "-pl", "100", "-ps", "50", "-m", "2", "-e", "50", "-o", out_fn] + options
    random.seed(seed)
    np.random.seed(seed)
    old_argv, sys.argv = sys.argv, argv
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            design.main(design.init_and_parse_args(args_type="basic"))
    finally:
        sys.argv = old_argv
    recs = read_records(out_fn)
    sys.stderr.write("%s: %d records\n" % (name, len(recs)))
    return dict(name=name, options=options, seed=seed, records_in_file_order=recs, records=sorted(recs),
                stdout=buf.getvalue()), out_fn


def write_n_fasta(rng):
    """Three related 700-base sequences with an isolated N every 70 bases: a window of 100 holds at most 2."""
    base = rng.choices("ACGT", k=700)
    with open(N_FASTA, "w") as f:
        for gi in range(3):
            s = list(base)
            for j in rng.sample(range(700), 12 * gi):
                s[j] = rng.choice("ACGT")
            for j in range(20 + 7 * gi, 700, 70):
                s[j] = "N"
            f.write(">synthetic_%d\n%s\n" % (gi, "".join(s)))


def main():
    rng = random.Random(20240521)
    design = load_design()
    data = dict(python=sys.version.split()[0], hashseed=os.environ.get("PYTHONHASHSEED"))
    with tempfile.TemporaryDirectory() as tmp:
        data["polya"] = polya_cases(rng)
        data["fasta"] = fasta_cases(rng, tmp)
        data["nexp"] = nexp_cases(rng)
        data["rc"] = rc_cases(rng)
        data["options"] = option_surface(design)
        write_n_fasta(rng)
        runs = []
        polya = ["--filter-polya", "12", "2"]
        plain, plain_fn = run_design(design, tmp, "plain10", EBOLA, ["--limit-target-genomes", "10"], 1)
        runs.append(plain)
        specs = [("run1", EBOLA, ["--limit-target-genomes", "30"] + polya, 1),
                 ("run2", EBOLA, ["--limit-target-genomes", "30"] + polya + ["--filter-with-lsh-hamming", "2"], 1),
                 ("run3", EBOLA, ["--limit-target-genomes", "10"] + polya + ["--add-reverse-complements", "--print-analysis"], 1),
                 ("run4", EBOLA, ["--limit-target-genomes", "10", "--filter-from-fasta", plain_fn, "--skip-set-cover"], 1),
                 ("run5", EBOLA, ["--limit-target-genomes-randomly-with-replacement", "8"], 7),
                 ("run6", N_FASTA, ["--expand-n"], 1)]
        for name, dataset, options, seed in specs:
            r, _ = run_design(design, tmp, name, dataset, options, seed)
            # (the test writes plain10's records to a file of its own and names it here)
            r["options"] = ["<plain10>" if o == plain_fn else o for o in r["options"]]
            r["dataset"] = os.path.basename(dataset)
            runs.append(r)
        plain["dataset"] = os.path.basename(EBOLA)
        data["runs"] = runs
    with gzip.GzipFile(os.path.join(HERE, "design_filters.json.gz"), "wb", mtime=0) as g:
        g.write(json.dumps(data, indent=0).encode())


if __name__ == "__main__":
    main()
