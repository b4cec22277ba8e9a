#!/usr/bin/env python3
"""Coverage-analysis command fixture (authoring container only).

Runs the LIVE reference (its package `catch` and its bin/ directory in a
checkout named by CATCH_REFERENCE) and records only inputs and outputs as
tests/golden/analysis_cli.json.gz:

  cli cases       bin/analyze_probe_coverage.py's main(args) in-process, after
                  np.random.seed(seed) (the random-anchor k-mer map draws from
                  np.random), on FASTA files written from the recorded records
  analyzer cases  coverage_analysis.Analyzer directly, for genomes of several
                  chromosomes (the command reads one genome per FASTA record, so
                  it cannot make them), after the same seeding

Every case records its inputs (FASTA records of every dataset and of the probe
file, in file order, repeated headers included; the options), and of the run:
`sliding_coverage` (per group, genome and strand the sorted (key, value)
pairs), `target_covers` (the cover ranges those windows were computed from),
the text of the three written files and the printed report.

Inputs: seeded species of catch_amd/utils/synthetic.py, with a genome shorter
than the 50-base window and one shorter than half of it appended to one
dataset, and the first records of tests/golden/ebola_zaire_100.fasta.gz.
The probe files hold two records that share a sequence under different headers
and two that share a header.

    CATCH_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/make_analysis_golden.py
"""
import argparse
import contextlib
import gzip
import importlib.util
import io
import json
import logging
import os
import sys
import tempfile
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if not os.environ.get("CATCH_REFERENCE"):
    sys.exit("set CATCH_REFERENCE to a checkout of the reference")
REF = os.environ["CATCH_REFERENCE"]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)

import numpy as np  # noqa: E402

from catch import coverage_analysis, genome, probe  # noqa: E402

from catch_amd.utils import synthetic  # noqa: E402


def reference_command():
    spec = importlib.util.spec_from_file_location(
        "reference_analyze_probe_coverage", os.path.join(REF, "bin", "analyze_probe_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tile(seq, length, stride):
    return [seq[i:i + length] for i in range(0, len(seq) - length + 1, stride)
            if "N" not in seq[i:i + length]]


def probe_records(seqs):
    """Headers p0, p1, ..; then a record that repeats probe 1's sequence under a header of its own, and two
    records under one header (read_fasta keeps the later sequence at the first one's place)."""
    recs = [["p%d" % i, s] for i, s in enumerate(seqs)]
    recs.append(["same_sequence_as_p1", seqs[1]])
    recs.append(["p2", seqs[3][::-1]])
    return recs


def write_fasta(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n" % h)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")


def read_ebola(n):
    recs, cur = [], None
    with gzip.open(os.path.join(HERE, "ebola_zaire_100.fasta.gz"), "rt") as f:
        for line in f:
            line = line.rstrip()
            if line.startswith(">"):
                if len(recs) == n:
                    break
                cur = [line[1:], ""]
                recs.append(cur)
            elif line:
                cur[1] += line.upper()
    return recs


def per_strand_lists(analyzer, genomes_grouped):
    """(sliding_coverage as sorted (key, value) pairs, target_covers as sorted (start, end) pairs), each
    [group][genome][strand]; the cover ranges are what the window rule is applied to."""
    sliding, covers = [], []
    for i, grp in enumerate(genomes_grouped):
        sliding.append([])
        covers.append([])
        for j in range(len(grp)):
            strands = (False, True) if analyzer.rc_too else (False,)
            sliding[i].append([sorted([float(k), float(v)] for k, v in analyzer.sliding_coverage[i][j][rc].items())
                               for rc in strands])
            covers[i].append([sorted([int(a), int(b)] for a, b in analyzer.target_covers[i][j][rc])
                              for rc in strands])
    return sliding, covers


def outputs(run, tmp):
    """run(tsv, sliding, counts) performs the analysis and prints the report."""
    paths = [os.path.join(tmp, n) for n in ("analysis.tsv", "sliding.tsv", "counts.tsv")]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        run(*paths)
    texts = []
    for p in paths:
        with open(p) as f:
            texts.append(f.read())
    return dict(analysis_tsv=texts[0], sliding_tsv=texts[1], map_counts_tsv=texts[2], report=buf.getvalue())


def cli_case(cmd, name, seed, datasets, probes, options):
    """datasets: [(file name, records)]"""
    captured = {}
    orig_run = coverage_analysis.Analyzer.run

    def run_and_keep(self, *a, **kw):
        captured["analyzer"] = self
        return orig_run(self, *a, **kw)

    with tempfile.TemporaryDirectory() as tmp:
        for fn, recs in datasets:
            write_fasta(os.path.join(tmp, fn), recs)
        write_fasta(os.path.join(tmp, "probes.fasta"), probes)

        def run(tsv, sliding, counts):
            args = argparse.Namespace(
                dataset=[os.path.join(tmp, fn) for fn, _ in datasets],
                probes_fasta=os.path.join(tmp, "probes.fasta"),
                mismatches=options["mismatches"], lcf_thres=options["lcf_thres"],
                island_of_exact_match=options.get("island_of_exact_match", 0),
                cover_extension=options.get("cover_extension", 0),
                limit_target_genomes=options.get("limit_target_genomes"),
                print_analysis=True, write_analysis_to_tsv=tsv, write_sliding_window_coverage=sliding,
                write_probe_map_counts_to_tsv=counts, max_num_processes=None,
                kmer_probe_map_k=options.get("kmer_probe_map_k", 10), log_level=logging.WARNING)
            np.random.seed(seed)
            coverage_analysis.Analyzer.run = run_and_keep
            try:
                cmd.main(args)
            finally:
                coverage_analysis.Analyzer.run = orig_run
        t0 = time.perf_counter()
        out = outputs(run, tmp)
    a = captured["analyzer"]
    out["sliding_coverage"], out["target_covers"] = per_strand_lists(a, a.target_genomes)
    out["genome_lengths"] = [[g.size(False) for g in grp] for grp in a.target_genomes]
    out["reference_wall_s"] = round(time.perf_counter() - t0, 2)
    sys.stderr.write("%s: %.1f s\n" % (name, out["reference_wall_s"]))
    return dict(name=name, kind="cli", np_seed=seed, options=options, probes=probes,
                datasets=[dict(file=fn, records=recs) for fn, recs in datasets], **out)


def analyzer_case(name, seed, groups, group_names, probes, options):
    """groups: [[[chromosome, ...] per genome] per group]"""
    gens = [[genome.Genome.from_one_seq(g[0]) if len(g) == 1 else
             genome.Genome.from_chrs(dict(("c%d" % i, x) for i, x in enumerate(g))) for g in grp] for grp in groups]
    ps = [probe.Probe.from_str(s) for s in probes]
    np.random.seed(seed)
    a = coverage_analysis.Analyzer(ps, options["mismatches"], options["lcf_thres"], gens, group_names,
                                   cover_extension=options.get("cover_extension", 0),
                                   kmer_probe_map_k=options.get("kmer_probe_map_k", 10))

    def run(tsv, sliding, counts):
        a.run()
        a.write_data_matrix_as_tsv(tsv)
        a.write_sliding_window_coverage(sliding)
        a.write_probe_map_counts(counts)
        a.print_analysis()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        out = outputs(run, tmp)
    out["sliding_coverage"], out["target_covers"] = per_strand_lists(a, gens)
    out["genome_lengths"] = [[g.size(False) for g in grp] for grp in gens]
    out["reference_wall_s"] = round(time.perf_counter() - t0, 2)
    sys.stderr.write("%s: %.1f s\n" % (name, out["reference_wall_s"]))
    return dict(name=name, kind="analyzer", np_seed=seed, options=options, probes=probes, groups=groups,
                group_names=group_names, **out)


def main():
    cmd = reference_command()
    rng = np.random.Generator(np.random.PCG64(20261017))
    sp1 = synthetic.make_species(rng, [2400], 3, 2, 0.04, 0.01)
    sp2 = synthetic.make_species(rng, [1700], 2, 1, 0.05, 0.02)
    sp3 = synthetic.make_species(rng, [900, 600, 130], 2, 1, 0.04, 0.02)     # three chromosomes per genome
    short = "".join("ACGT"[c] for c in rng.integers(0, 4, size=40))
    ds1 = [["sp1_g%d" % i, g[0]] for i, g in enumerate(sp1)]
    ds2 = [["sp2_g%d" % i, g[0]] for i, g in enumerate(sp2)]
    # shorter than the 50-base window (2n - 50 > 0) and shorter than half of it
    ds2 += [["sp2_short40", short], ["sp2_short20", short[7:27]]]
    two = [("species_one.fasta", ds1), ("species_two.fa", ds2)]
    # (related genomes are tiled at offsets that differ modulo every anchor spacing: two probes that first matched at
    # the same k-mer of a sequence would be listed in the order of a Python set, which follows the string hash seed)
    seqs = tile(sp1[0][0], 100, 150) + tile(sp2[0][0], 100, 150) + tile(sp1[2][0][37:], 100, 300)
    probes = probe_records(seqs)

    cases = [
        cli_case(cmd, "pigeonhole_e0", 1, two, probes, dict(mismatches=2, lcf_thres=100)),
        cli_case(cmd, "pigeonhole_e50", 2, two, probes, dict(mismatches=2, lcf_thres=100, cover_extension=50)),
        cli_case(cmd, "random_anchor_e20", 3, two, probes, dict(mismatches=3, lcf_thres=80, cover_extension=20)),
        cli_case(cmd, "limit_target_genomes", 4, two, probes,
                 dict(mismatches=2, lcf_thres=100, cover_extension=10, limit_target_genomes=2)),
        cli_case(cmd, "island_k20", 5, two, probes,
                 dict(mismatches=4, lcf_thres=100, island_of_exact_match=30, kmer_probe_map_k=20)),
    ]
    # short genomes that ARE covered, unevenly: the last 30 (15) bases of a probe, then bases of their own -- so the
    # window [max(0, 2n - 50), n) of the 40-base genome averages differently from the whole genome
    pr = tile(sp2[0][0], 100, 150)[2]
    own = "".join("ACGT"[c] for c in rng.integers(0, 4, size=10))
    covered_short = [["short40", pr[70:] + own], ["short20", pr[85:] + own[:5]], ["sp2_g1", sp2[1][0]]]
    cases.append(cli_case(cmd, "short_genomes_covered", 11, [("short.fasta", covered_short)], probes,
                          dict(mismatches=0, lcf_thres=15)))
    ebola = read_ebola(3)
    eb_probes = probe_records(tile(ebola[0][1], 100, 400) + tile(ebola[2][1][53:], 100, 900))
    cases.append(cli_case(cmd, "ebola_e50", 6, [("ebola_zaire_3.fasta", ebola)], eb_probes,
                          dict(mismatches=2, lcf_thres=100, cover_extension=50)))
    chr_probes = [s for _h, s in probe_records(tile(sp3[0][0], 100, 120) + tile(sp3[0][1], 100, 120) +
                                               tile(sp1[1][0], 100, 400))]
    cases.append(analyzer_case("multi_chromosome_e30", 7, [[list(g) for g in sp3], [[g[0]] for g in sp1[:2]]],
                               ["segmented", "species_one"], chr_probes,
                               dict(mismatches=2, lcf_thres=100, cover_extension=30)))
    cases.append(analyzer_case("multi_chromosome_random_anchor", 8, [[list(g) for g in sp3]], ["segmented"],
                               chr_probes, dict(mismatches=2, lcf_thres=75, cover_extension=0)))

    import catch
    out = dict(window=[50, 25], python=sys.version.split()[0], numpy=np.__version__,
               reference_version=getattr(catch, "__version__", None), cases=cases)
    path = os.path.join(HERE, "analysis_cli.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    sys.stderr.write("%s: %d cases, %d bytes\n" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
