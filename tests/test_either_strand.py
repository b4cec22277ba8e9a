"""SetCoverFilter(either_strand=True), `design --either-strand`, `prune_probes --either-strand` and
Analyzer(either_strand=True): a candidate covers what its own string or its reverse complement hybridises to.

set(i) = rows(scan of s_i) | rows(scan of revcomp(s_i)), both against the targets as given; the expected tables here
are the NumPy union (test_rows_union._model_union) of the oracle's cover rows of the strings and of their reverse
complements, and everything behind the table is checked with the restatements of the other options' own test files."""
import os
from collections import Counter

import numpy as np
import pytest

from test_extend_probes import (EBOLA, _candidates, _genomes, _np_subtract, _oracle_rows, _table, _union_len)
from test_rows_union import _model_union

_RC = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s[::-1].translate(_RC)


def _filter(e=0, coverage=1.0, m=2, **kw):
    from catch_amd.filter import set_cover_filter as scf
    return scf.SetCoverFilter(mismatches=m, lcf_thres=100, coverage=coverage, cover_extension=e, **kw)


def _random_genome():
    rng = np.random.default_rng(20261021)
    return "".join(rng.choice(list("ACGT"), size=400))


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n%s\n" % (name, seq))
    return str(path)


# ------------------------------------------------------------------ without a GPU
def test_reverse_complement_leaves_n_and_other_bytes_alone():
    from catch_amd.filter.set_cover_filter import _reverse_complement
    assert _reverse_complement("ACGTN") == "NACGT"
    assert _reverse_complement("AANNCRY-acgt") == "tgca-YRGNNTT"
    assert _reverse_complement("") == ""
    s = "GATTACANNRYKM"
    assert _reverse_complement(_reverse_complement(s)) == s


def test_keyword_is_taken_beyond_init_and_keeps_the_rows():
    import inspect
    from catch_amd.filter import set_cover_filter as scf
    assert list(inspect.signature(scf.SetCoverFilter.__init__).parameters)[-1] == "fixed_probes"
    off, on = _filter(), _filter(either_strand=True)
    assert off.either_strand is False and not off.needs_rows
    assert on.either_strand is True and on.needs_rows
    assert _filter(either_strand=np.bool_(True)).either_strand is True
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="either_strand must be True or False"):
            _filter(either_strand=bad)


def test_front_end_stays_on_the_host_under_either_strand():
    from catch_amd.filter import probe_designer
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for flag, want in ((False, "per group"), (True, None)):
        f = _filter(either_strand=flag)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == want


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    with pytest.raises(NotImplementedError, match="either_strand runs on one rank"):
        _filter(either_strand=True)._filter_strs([["ACGT" * 25]], [[]])


def test_command_line_refusals(tmp_path):
    from catch_amd import analyze_probe_coverage, design, prune_probes
    fa = _write_fasta(tmp_path / "t.fasta", [("a", "ACGT" * 100)])
    base = [fa, "-o", str(tmp_path / "o.fasta"), "--either-strand"]
    with pytest.raises(Exception, match="Cannot use --either-strand with --skip-set-cover"):
        design.main(design.parse_args(base + ["--skip-set-cover"]))
    with pytest.raises(Exception, match="--either-strand with --cluster-and-design-separately .*to 0"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="--either-strand with --cluster-and-design-separately .*to 0"):     # design_large's default
        design.main(design.parse_args(base, args_type="large"))
    with pytest.raises(Exception, match="--either-strand with --cluster-from-fragments .*to 0"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0"], args_type="large"))
    assert not os.path.exists(str(tmp_path / "o.fasta"))
    assert design.parse_args([fa, "-o", "x"]).either_strand is False
    assert prune_probes.parse_args(["-d", fa, "-f", fa, "-o", "x", "--either-strand"]).either_strand is True
    assert prune_probes.parse_args(["-d", fa, "-f", fa, "-o", "x"]).either_strand is False
    argv = ["-d", fa, "-f", fa, "-m", "0", "-l", "100"]
    assert analyze_probe_coverage.parse_args(argv + ["--either-strand"]).either_strand is True
    assert analyze_probe_coverage.parse_args(argv).either_strand is False


def test_analyzer_refuses_both_strand_options_and_folds_the_map_counts():
    from catch_amd import coverage_analysis, probe
    probes = [probe.Probe.from_str(s) for s in ("AAAC", "GGGT", "ACGT")]
    with pytest.raises(ValueError, match="rc_too must be False"):
        coverage_analysis.Analyzer(probes, 0, 4, [[]], either_strand=True, rc_too=True)
    with pytest.raises(ValueError, match="rc_too must be False"):
        coverage_analysis.Analyzer(probes, 0, 4, [[]], either_strand=True)       # (rc_too defaults to True)
    a = coverage_analysis.Analyzer(probes, 0, 4, [[]], either_strand=True, rc_too=False)
    assert [p.seq_str for p in a._analysed] == ["AAAC", "GGGT", "ACGT", "GTTT", "ACCC", "ACGT"]
    assert a.probes is probes
    # a stubbed count per analysed entry: entry n + i counts for probe i, and both count where both map
    a.probe_map_counts = Counter()
    a._fold_map_counts(np.array([1, 0, 0, 2, 3, 5]))
    assert a.probe_map_counts == Counter({probes[0]: 3, probes[1]: 3, probes[2]: 5})
    b = coverage_analysis.Analyzer(probes, 0, 4, [[]], rc_too=False)
    assert b._analysed is probes and b.either_strand is False
    b.probe_map_counts = Counter()
    b._fold_map_counts(np.array([1, 0, 4]))
    assert b.probe_map_counts == Counter({probes[0]: 1, probes[2]: 4})


# ------------------------------------------------------------------ 1. the provable case
def _provable():
    """G, revcomp(G), their genomes and the 8 candidates of -pl 100 -ps 100 (the windows of G, then those of
    revcomp(G)); no window of one is a window of the other."""
    from catch_amd.genome import Genome
    G = _random_genome()
    R = _rc(G)
    cands = [G[j:j + 100] for j in range(0, 400, 100)] + [R[j:j + 100] for j in range(0, 400, 100)]
    windows_g = {G[j:j + 100] for j in range(301)}
    assert not windows_g & {R[j:j + 100] for j in range(301)}
    assert len(set(cands)) == 8
    return G, R, [Genome.from_one_seq(G), Genome.from_one_seq(R)], cands


@pytest.mark.gpu
def test_two_orientations_of_one_genome_need_half_the_probes(ctx):
    _G, _R, genomes, cands = _provable()
    f = _filter(m=0, either_strand=True)
    got = f._filter_strs([cands], [genomes], assume_unique=True)
    assert len(got) == 1 and len(got[0]) == 4
    assert sorted(got[0]) == [0, 1, 2, 3]              # of two candidates with equal sets the first one handed in wins
    t = f.last_timings
    assert (t["rows"], t["rows_rc"], t["rows_union"], t["picks"]) == (8, 8, 16, 4)
    assert t["rc_scan_ms"] > 0 and t["union_ms"] > 0 and t["scan_ms"] > 0
    held = []
    try:
        rows = f._scan_group(ctx, held, cands, genomes, assume_unique=True)[2]
        si, un, st, en = rows.fetch()
        assert rows.n == 16 and np.array_equal(si, np.repeat(np.arange(8), 2)) and un.tolist() == [0, 1] * 8
        assert (en - st == 100).all()
        chk = rows.cover_check(len(cands), got[0])
        assert chk["picks_without_gain"] == chk["universes_short"] == chk["bad_pick_ids"] == 0, chk
        assert chk["covered_bases"] == chk["universe_bases"] == 800
        # the other four gain nothing behind them
        assert rows.cover_check(len(cands), got[0] + [4])["picks_without_gain"] == 1
    finally:
        for h in reversed(held):
            h.close()
    plain = _filter(m=0)
    assert len(plain._filter_strs([cands], [genomes], assume_unique=True)[0]) == 8
    assert not {"rc_scan_ms", "union_ms", "rows_rc", "rows_union"} & set(plain.last_timings)
    assert len(_filter(m=0, either_strand=False)._filter_strs([cands], [genomes], assume_unique=True)[0]) == 8


@pytest.mark.gpu
def test_design_either_strand_command_line_and_analysis(ctx, tmp_path, capsys, caplog):
    import logging
    from catch_amd import design
    from catch_amd.utils import seq_io
    G, R, _genomes2, cands = _provable()
    fa = _write_fasta(tmp_path / "two.fasta", [("forward", G), ("reverse", R)])
    base = [fa, "-pl", "100", "-ps", "100", "-m", "0", "-l", "100", "-e", "0", "-c", "1.0"]
    out, plain = str(tmp_path / "either.fasta"), str(tmp_path / "plain.fasta")
    capsys.readouterr()
    with caplog.at_level(logging.INFO, logger="catch_amd.filter.set_cover_filter"):
        design.main(design.parse_args(base + ["--either-strand", "-o", out]))
    assert capsys.readouterr().out.split() == ["4"]
    assert any("either strand: 8 rows forward, 8 reverse, 16 in the union" in r.getMessage() for r in caplog.records)
    assert sorted(seq_io.iterate_fasta(out)) == sorted(cands[:4])  # forward strings, as they were handed in
    design.main(design.parse_args(base + ["-o", plain]))
    assert capsys.readouterr().out.split() == ["8"]
    # the analysis under --either-strand: every base of both genomes is covered, forward rows only
    tsv = str(tmp_path / "a.tsv")
    design.main(design.parse_args(base + ["--either-strand", "-o", out, "--print-analysis",
                                          "--write-analysis-to-tsv", tsv]))
    printed = capsys.readouterr().out
    assert "NUMBER OF PROBES: 4" in printed and printed.count("400 (100.00%)") == 2 and "(rc)" not in printed
    rows = [line.rstrip("\n").split("\t") for line in open(tsv)][1:]
    assert [r[0] for r in rows] == ["two.fasta, genome 0", "two.fasta, genome 1"]
    assert [int(r[1]) for r in rows] == [400, 400] and [float(r[2]) for r in rows] == [1.0, 1.0]
    assert [float(r[4]) for r in rows] == [1.0, 1.0]                # every base under one orientation of one probe
    # with both orientations in the output the two-strand analysis is the report
    design.main(design.parse_args(base + ["--either-strand", "--add-reverse-complements", "-o", out,
                                          "--print-analysis"]))
    printed = capsys.readouterr().out
    assert "NUMBER OF PROBES: 8" in printed and printed.count("400 (100.00%)") == 4 and printed.count("(rc)") == 2


# ------------------------------------------------------------------ 4. prune_probes
@pytest.mark.gpu
def test_prune_probes_either_strand_drops_the_second_orientation(ctx, tmp_path, capsys):
    from catch_amd import prune_probes
    from catch_amd.utils import seq_io
    G, R, _g, _c = _provable()
    windows = [G[j:j + 100] for j in range(0, 400, 100)]
    probes = windows + [_rc(w) for w in windows]
    fa = _write_fasta(tmp_path / "two.fasta", [("forward", G), ("reverse", R)])
    pf = _write_fasta(tmp_path / "probes.fasta", [("p%d" % j, s) for j, s in enumerate(probes)])
    argv = ["-d", fa, "-f", pf, "-m", "0", "-l", "100", "-e", "0"]
    capsys.readouterr()
    kept, removed = prune_probes.main(prune_probes.parse_args(argv + ["-o", str(tmp_path / "k.fasta"), "--either-strand"]))
    assert kept == [0, 1, 2, 3] and removed == [7, 6, 5, 4]
    assert capsys.readouterr().out.split() == ["4", "4"]
    assert list(seq_io.iterate_fasta(str(tmp_path / "k.fasta"))) == windows
    kept, removed = prune_probes.main(prune_probes.parse_args(argv + ["-o", str(tmp_path / "all.fasta")]))
    assert kept == list(range(8)) and removed == []


# ------------------------------------------------------------------ 2. parity on real data
_cache = {}


def _mixed():
    """The first 5 Ebola genomes, the second and the fourth reverse-complemented, and their candidates."""
    if "g" not in _cache:
        from catch_amd.genome import Genome
        g5 = _genomes(5)
        g = [Genome.from_one_seq(_rc(x.seqs[0])) if j in (1, 3) else x for j, x in enumerate(g5)]
        assert all(len(x.seqs) == 1 for x in g5)
        _cache["g"] = (g, _candidates(g))
    return _cache["g"]


def _union_table(oracle, strs, genomes, e, one_set=False):
    """The NumPy union of the oracle's cover rows of `strs` and of their reverse complements (one_set: every string
    under set id 0, as the filter scans its fixed probes)."""
    fwd, rev = _oracle_rows(oracle, strs, genomes, e), _oracle_rows(oracle, [_rc(s) for s in strs], genomes, e)
    if one_set:
        fwd, rev = ((np.zeros_like(t[0]),) + tuple(t[1:]) for t in (fwd, rev))
    return _table(_model_union(fwd, rev)[0])


def _expected(oracle, e):
    key = ("U", e)
    if key not in _cache:
        g, c = _mixed()
        _cache[key] = _union_table(oracle, c, g, e)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_equals_the_oracle_on_the_numpy_union(ctx, oracle, e, coverage):
    from catch_amd import probe
    g, c = _mixed()
    assert not probe.anchors_use_random(c, 2, 100, 20)         # pigeonhole anchors: nothing is drawn
    U = _expected(oracle, e)
    want = oracle.approx_multiuniverse(*U, len(c), len(g), universe_p=[coverage] * len(g))
    f = _filter(e, coverage, either_strand=True)
    got = f._filter_strs([c], [g], assume_unique=True)[0]
    plain = _filter(e, coverage)._filter_strs([c], [g], assume_unique=True)[0]
    t = f.last_timings
    print("e = %d, coverage %g: %d candidates; %d picks under either strand, %d without; rows %d forward, %d reverse, "
          "%d in the union; scan_ms %.3f rc_scan_ms %.3f union_ms %.3f greedy_ms %.3f"
          % (e, coverage, len(c), len(got), len(plain), t["rows"], t["rows_rc"], t["rows_union"], t["scan_ms"],
             t["rc_scan_ms"], t["union_ms"], t["greedy_ms"]))
    assert got == [int(i) for i in want] and 0 < len(got) < len(plain)
    assert t["rows_union"] == U[0].size and t["picks"] == len(got)
    # the device's union table itself, row for row
    held = []
    try:
        rows = f._scan_group(ctx, held, c, g, assume_unique=True)[2]
        for a, b, name in zip(rows.fetch(), U, ("set", "universe", "start", "end")):
            assert np.array_equal(a, b), name
        chk = rows.cover_check(len(c), got, None if coverage == 1.0 else [coverage] * len(g))
        assert chk["picks_without_gain"] == chk["universes_short"] == chk["bad_pick_ids"] == 0, chk
    finally:
        for h in reversed(held):
            h.close()


# ------------------------------------------------------------------ 3. with the other options of the rows loop
@pytest.mark.gpu
@pytest.mark.parametrize("option", ["fixed_probes", "coverage_depth", "prune_redundant", "max_probes",
                                    "target_regions"])
def test_the_other_rows_options_see_the_union_table(ctx, oracle, option):
    from catch_amd.filter.set_cover_filter import extension_fraction
    g, c = _mixed()
    e, ng, glen = 50, len(g), [x.size() for x in g]
    U = _expected(oracle, e)
    picks = [int(i) for i in oracle.approx_multiuniverse(*U, len(c), ng, universe_p=[1.0] * ng)]
    if option == "fixed_probes":
        fixed = [c[i] for i in picks[:len(picks) // 2]]
        cov = _union_table(oracle, fixed, g, e, one_set=True)
        reduced = _np_subtract(U, cov, glen)
        n2, c0 = _union_len(reduced, ng), _union_len(cov, ng)
        q = [extension_fraction(int(a), int(b), 1.0) for a, b in zip(n2, c0)]
        want = [int(i) for i in oracle.approx_multiuniverse(*reduced, len(c), ng, universe_p=q)]
        f = _filter(e, either_strand=True, fixed_probes=fixed)
        assert f._filter_strs([c], [g], assume_unique=True) == [want] and 0 < len(want) < len(picks)
        assert f.last_timings["rows_fixed"] == cov[0].size and f.last_timings["rows_reduced"] == reduced[0].size
    elif option == "coverage_depth":
        from test_coverage_depth import _oracle_depth_design
        layers, _facts, nrows = _oracle_depth_design(oracle, U, len(c), glen, 2, [1.0] * ng)
        f = _filter(e, either_strand=True, coverage_depth=2)
        assert f._filter_strs([c], [g], assume_unique=True) == [[int(i) for layer in layers for i in layer]]
        assert f.last_layer_sizes == [[len(x) for x in layers]] and layers[0] == picks and len(layers[1]) > 0
        assert f.last_timings["rows_reduced"] == sum(nrows)
    elif option == "prune_redundant":
        from test_prune_redundant import _walk
        kept, removed, before, after = _walk(U, glen, picks, 1)
        f = _filter(e, either_strand=True, prune_redundant=True)
        assert f._filter_strs([c], [g], assume_unique=True) == [kept] and f.last_pruned == [removed]
        assert np.array_equal(np.minimum(before, 1), np.minimum(after, 1))
    elif option == "max_probes":
        from test_max_probes import _model
        f = _filter(e, either_strand=True, max_probes=37, curve_points=10)
        assert f._filter_strs([c], [g], assume_unique=True) == [picks[:37]] and len(picks) > 37
        want_gains, _curve = _model(U, glen, picks)
        assert np.array_equal(f.last_pick_gains[0].astype(np.int64), want_gains)
        assert f.last_budget_kept == [37]
    else:
        from test_target_regions import _np_cut, _real_regions, _wanted_bits
        regions, iv = _real_regions(g)
        cut = _np_cut(U, _wanted_bits(glen, iv), glen)
        want = [int(i) for i in oracle.approx_multiuniverse(*cut, len(c), ng, universe_p=[1.0] * ng)]
        f = _filter(e, either_strand=True, target_regions=regions)
        assert f._filter_strs([c], [g], assume_unique=True) == [want] and 0 < len(want) < len(picks)
        assert f.last_timings["rows_restricted"] == cut[0].size
    assert f.last_timings["rows_union"] == U[0].size
