"""--max-cross-dimer and --cross-dimer through the design command and the probe report, on the GPU: a case small
enough to prove by hand, and real genomes filed in both orientations (the models are cross_dimer.py's host forms)."""
import logging

import numpy as np
import pytest

from test_either_strand import _mixed, _provable, _write_fasta


def _cd():
    from catch_amd.filter import cross_dimer
    return cross_dimer


def _read(path):
    from catch_amd.utils import seq_io
    return list(seq_io.iterate_fasta(str(path)))


# ------------------------------------------------------------------ small and provable
@pytest.mark.gpu
def test_design_drops_the_second_orientation_of_one_genome(ctx, tmp_path, capsys, caplog):
    from catch_amd import design, probe_report
    cd = _cd()
    G, R, _genomes, cands = _provable()
    # the four windows of G do not pair with each other beyond 30; with the windows of revcomp(G) every probe has a
    # partner over its whole length
    values, _partners = cd.cross_dimers(cands[:4])
    assert max(values) <= 30
    values, partners = cd.cross_dimers(cands)
    assert values == [100] * 8 and partners == [7, 6, 5, 4, 3, 2, 1, 0]
    fa = _write_fasta(tmp_path / "two.fasta", [("forward", G), ("reverse", R)])
    base = [fa, "-pl", "100", "-ps", "100", "-m", "0", "-l", "100", "-e", "0", "-c", "1.0"]
    plain, out = str(tmp_path / "plain.fasta"), str(tmp_path / "out.fasta")
    report, again = str(tmp_path / "report.tsv"), str(tmp_path / "again.tsv")
    capsys.readouterr()
    design.main(design.parse_args(base + ["-o", plain]))
    assert capsys.readouterr().out.split() == ["8"]
    first = _read(plain)
    assert sorted(first) == sorted(cands)
    with caplog.at_level(logging.INFO, logger="catch_amd.design"):
        design.main(design.parse_args(base + ["-o", out, "--max-cross-dimer", "30", "--verbose",
                                              "--write-probe-report", report]))
    assert capsys.readouterr().out.split() == ["4"]
    assert _read(out) == first[:4]
    said = [r.getMessage() for r in caplog.records if "cross-dimer filter" in r.getMessage()]
    assert len(said) == 1 and "cross-dimer filter: 4 of 8 probes dropped (largest cross-dimer 100 before, " in said[0]
    assert said[0].endswith("%d after)" % max(cd.cross_dimers(first[:4])[0]))
    probe_report.main(probe_report.parse_args(["-f", out, "-o", again, "--max-cross-dimer", "30"]))
    capsys.readouterr()
    assert open(report).read() == open(again).read()
    rows = [line.split("\t") for line in open(report).read().splitlines()]
    assert rows[0][-3:] == ["cross_dimer", "cross_partner", "verdict"] and len(rows) == 5
    assert all(r[-1] == "ok" for r in rows[1:])
    # --cross-dimer alone only adds the two columns to the report
    design.main(design.parse_args(base + ["-o", out, "--cross-dimer", "--write-probe-report", report]))
    capsys.readouterr()
    assert _read(out) == first
    rows = [line.split("\t") for line in open(report).read().splitlines()]
    assert rows[0][-2:] == ["cross_dimer", "cross_partner"]
    assert [r[-2:] for r in rows[1:]] == [["100", str(first.index(_rc_of(s)) + 1)] for s in first]


def _rc_of(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


# ------------------------------------------------------------------ real data
_cache = {}
BASE = ["-pl", "100", "-ps", "200", "-m", "4", "-l", "100", "-e", "50", "-c", "0.75"]


def _plain(tmp_path_factory, capsys):
    """The plain design of the five genomes (two of them reverse-complemented), and the run matrix of its probes."""
    if "p" not in _cache:
        from catch_amd import design
        genomes, _cands = _mixed()
        d = tmp_path_factory.mktemp("cross_dimer")
        fa = _write_fasta(d / "mixed.fasta", [("g%d" % j, g.seqs[0]) for j, g in enumerate(genomes)])
        out = str(d / "plain.fasta")
        design.main(design.parse_args([fa] + BASE + ["-o", out]))
        capsys.readouterr()
        probes = _read(out)
        _cache["p"] = (fa, out, probes, _cd().run_matrix(probes))
    return _cache["p"]


@pytest.mark.gpu
def test_report_and_engine_equal_the_host_path_on_real_probes(ctx, tmp_path_factory, tmp_path, capsys):
    from catch_amd import engine, probe_report
    cd = _cd()
    _fa, out, probes, m = _plain(tmp_path_factory, capsys)
    print("probes %d, largest cross %d" % (len(probes), int(m.max())))
    want_v, want_p = cd.cross_dimers_numpy(probes)
    assert want_v.tolist() == m.max(axis=1).tolist()
    assert len(probes) >= 50 and int(want_v.max()) > 30                    # both orientations meet in this design
    report = str(tmp_path / "r.tsv")
    probe_report.main(probe_report.parse_args(["-f", out, "-o", report, "--cross-dimer"]))
    capsys.readouterr()
    rows = [line.split("\t") for line in open(report).read().splitlines()]
    assert rows[0][-2:] == ["cross_dimer", "cross_partner"] and len(rows) == len(probes) + 1
    assert [r[-2] for r in rows[1:]] == [str(v) for v in want_v.tolist()]
    assert [r[-1] for r in rows[1:]] == [str(p + 1) if v > 0 else "NA" for v, p in zip(want_v.tolist(), want_p.tolist())]
    values, partners = engine.cross_dimer(ctx, probes)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()


@pytest.mark.gpu
def test_design_keeps_what_the_host_walk_keeps_on_real_probes(ctx, tmp_path_factory, tmp_path, capsys):
    from catch_amd import design
    cd = _cd()
    fa, _out, probes, m = _plain(tmp_path_factory, capsys)
    keep = cd.walk(probes, 30)
    n = len(probes)
    assert keep.tolist() == [not any(keep[j] and m[i, j] > 30 for j in range(i)) for i in range(n)]
    assert 0 < int(keep.sum()) < n
    out = str(tmp_path / "kept.fasta")
    design.main(design.parse_args([fa] + BASE + ["-o", out, "--max-cross-dimer", "30"]))
    assert capsys.readouterr().out.split() == [str(int(keep.sum()))]
    assert _read(out) == [s for s, k in zip(probes, keep) if k]
