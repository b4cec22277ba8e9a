"""--cross-dimer-redesign / SetCoverFilter(max_cross_dimer=X, cross_dimer_rounds=R): the repair rounds of
catch_amd/filter/set_cover_filter.py (_cross_rounds has the definition).  A case small enough to prove by hand through
the command, two datasets, and real genomes filed in both orientations against an explicit loop of the definition
built from the public pieces: SetCoverFilter(fixed_probes=...) once per round, engine.cross_against_flags (held to the
definition in test_cross_against.py) and cross_dimer.walk."""
import logging
import random

import numpy as np
import pytest

from test_either_strand import _mixed, _write_fasta

_RC = str.maketrans("ACGT", "TGCA")
STARTS = list(range(0, 301, 25))
BASE = ["-pl", "100", "-ps", "25", "-m", "0", "-l", "100", "-e", "0", "-c", "1.0"]


def _rc(s):
    return s[::-1].translate(_RC)


def _cd():
    from catch_amd.filter import cross_dimer
    return cross_dimer


def _read(path):
    from catch_amd.utils import seq_io
    return list(seq_io.iterate_fasta(str(path)))


def _genome(seed, planted=None):
    """400 draws of random.Random(seed).choice("ACGT"); planted: the 31 characters at 219 .. 249."""
    r = random.Random(seed)
    g = [r.choice("ACGT") for _ in range(400)]
    if planted is not None:
        g[219:250] = list(planted)
    return "".join(g)


def _windows(g):
    return [g[s:s + 100] for s in STARTS]


def _provable():
    """The genome whose bases 219 .. 249 are the reverse complement of its first 31."""
    plain = _genome(1)
    return _genome(1, _rc(plain[0:31]))


def _starts(g, probes):
    return [g.index(p) for p in probes]


def _filter(m=4, e=50, coverage=1.0, **kw):
    from catch_amd.filter import set_cover_filter as scf
    return scf.SetCoverFilter(mismatches=m, lcf_thres=100, coverage=coverage, cover_extension=e, **kw)


def _model(ctx, groups, genomes, X, R, E=(), **model):
    """The definition, spelled out: per group (selected strings in the order kept, rounds, picks dropped)."""
    from catch_amd import engine
    cd = _cd()
    K, out = [], []
    for C, gs in zip(groups, genomes):
        Kg, rounds, dropped = [], 0, 0
        while True:
            against = list(E) + K
            flags = engine.cross_against_flags(ctx, C, against, X) if against else np.zeros(len(C), bool)
            A = [c for c, f in zip(C, flags) if c not in set(Kg) and not f]
            fixed = list(E) + Kg
            picks = []
            if A:
                f = _filter(fixed_probes=fixed, **model) if fixed else _filter(**model)
                picks = [A[i] for i in f._filter_strs([A], [gs], assume_unique=True)[0]]
            keep = cd.walk(picks, X)
            kept = [p for p, k in zip(picks, keep) if k]
            Kg += kept
            K += [p for p in kept if p not in K]
            rounds += 1
            dropped += len(picks) - len(kept)
            if not picks or len(kept) == len(picks) or rounds == R:
                break
        out.append((Kg, rounds, dropped))
    return out


# ------------------------------------------------------------------ without a GPU
def test_keywords_are_taken_beyond_init_and_keep_the_rows():
    import inspect
    from catch_amd.filter import set_cover_filter as scf
    assert list(inspect.signature(scf.SetCoverFilter.__init__).parameters)[-1] == "fixed_probes"
    off, on = _filter(), _filter(max_cross_dimer=30)
    assert off.max_cross_dimer is None and not off.needs_rows
    assert on.max_cross_dimer == 30 and on.cross_dimer_rounds == 8 and on.needs_rows
    assert _filter(max_cross_dimer=30, cross_dimer_rounds=3).cross_dimer_rounds == 3
    assert _filter(max_cross_dimer=30, fixed_probes=["ACGT" * 25], either_strand=True, coverage=0.9).max_cross_dimer == 30
    for bad in (0, -3, 2.5, "7", True):
        with pytest.raises(ValueError):
            _filter(max_cross_dimer=bad)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="cross_dimer_rounds"):
            _filter(max_cross_dimer=30, cross_dimer_rounds=bad)
    for kw in (dict(coverage_depth=2), dict(prune_redundant=True), dict(max_probes=5), dict(pick_gains=True)):
        with pytest.raises(NotImplementedError, match="max_cross_dimer"):
            _filter(max_cross_dimer=30, **kw)


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    with pytest.raises(NotImplementedError, match="cross-dimer redesign .* one rank"):
        _filter(max_cross_dimer=30)._filter_strs([["ACGT" * 25]], [[]])


def test_command_line_refusals(tmp_path, capsys):
    from catch_amd import design, design_grid, design_naively
    fa = _write_fasta(tmp_path / "t.fasta", [("a", "ACGT" * 100)])
    out = str(tmp_path / "o.fasta")
    on = [fa, "-o", out, "--max-cross-dimer", "30", "--cross-dimer-redesign"]
    for argv, said in (
            ([fa, "-o", out, "--cross-dimer-redesign"], "needs --max-cross-dimer"),
            ([fa, "-o", out, "--max-cross-dimer", "30", "--cross-dimer-rounds", "3"], "needs --cross-dimer-redesign"),
            (on + ["--cross-dimer-rounds", "0"], "at least 1"),
            (on + ["--skip-set-cover"], "--skip-set-cover"),
            (on + ["--coverage-depth", "2"], "--coverage-depth above 1"),
            (on + ["--prune-redundant"], "--prune-redundant"),
            (on + ["--max-probes", "10"], "--max-probes"),
            (on + ["--write-coverage-curve", str(tmp_path / "c.tsv")], "--write-coverage-curve")):
        for args_type in ("basic", "large"):
            with pytest.raises(SystemExit) as exc:
                design.parse_args(argv, args_type=args_type)
            assert exc.value.code == 2
            assert said in capsys.readouterr().err, argv
    args = design.parse_args(on)
    assert args.cross_dimer_redesign and args.cross_dimer_rounds == 8 and args.max_cross_dimer == 30
    assert design.parse_args(on + ["--cross-dimer-rounds", "2"]).cross_dimer_rounds == 2
    off = design.parse_args([fa, "-o", out, "--max-cross-dimer", "30"])
    assert off.cross_dimer_redesign is False and off.cross_dimer_rounds is None
    with pytest.raises(Exception, match="--cross-dimer-redesign with --cluster-and-design-separately .*to 0"):
        design.main(design.parse_args(on + ["--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="--cross-dimer-redesign with --cluster-and-design-separately .*to 0"):
        design.main(design.parse_args(on, args_type="large"))           # design_large's default
    with pytest.raises(Exception, match="--cross-dimer-redesign with --cluster-from-fragments .*to 0"):
        design.main(design.parse_args(on + ["--cluster-and-design-separately", "0"], args_type="large"))
    # the other commands do not learn the option
    with pytest.raises(SystemExit):
        design_grid.parse_args([fa, "-o", out, "--grid-mismatches", "1", "--grid-cover-extension", "0",
                                "--cross-dimer-redesign"])
    assert "unrecognized arguments" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        design_naively.parse_args([fa, "-o", out, "--cross-dimer-redesign"])
    capsys.readouterr()


# ------------------------------------------------------------------ small and provable
@pytest.mark.gpu
def test_the_provable_case_through_the_command(ctx, tmp_path, capsys, caplog):
    from catch_amd import design
    cd = _cd()
    g = _provable()
    w = _windows(g)
    m = cd.run_matrix(w)
    above = {(STARTS[i], STARTS[j]) for i in range(13) for j in range(i + 1, 13) if m[i, j] > 30}
    assert above == {(0, 150), (0, 175), (0, 200)}
    assert max(int(m[i, j]) for i in range(13) for j in range(13) if m[i, j] <= 30) <= 25
    assert len({g[i:i + 20] for i in range(381)}) == 381                 # no 20-mer of the genome repeats
    fa = _write_fasta(tmp_path / "g.fasta", [("g", g)])
    base = [fa] + BASE

    def run(name, *more):
        out = str(tmp_path / name)
        design.main(design.parse_args(base + ["-o", out] + list(more)))
        capsys.readouterr()
        return out
    plain = run("plain.fasta")
    assert sorted(_starts(g, _read(plain))) == [0, 100, 200, 300]
    # the post-filter alone: three probes, and a hole
    gaps = str(tmp_path / "gaps.tsv")
    dropped = run("dropped.fasta", "--max-cross-dimer", "30", "--write-uncovered-regions", gaps)
    assert sorted(_starts(g, _read(dropped))) == [0, 100, 300]
    rows = [line.split("\t") for line in open(gaps).read().splitlines()[1:]]
    assert [r[2:5] for r in rows] == [["200", "300", "100"]]
    # the redesign: two rounds, windows 150, 175 and 200 never appear, nothing stays uncovered
    with caplog.at_level(logging.INFO):
        out = run("redesign.fasta", "--max-cross-dimer", "30", "--cross-dimer-redesign", "--verbose",
                  "--write-uncovered-regions", gaps)
    assert _starts(g, _read(out)) == [0, 100, 300, 225, 125]
    assert open(gaps).read().splitlines()[1:] == []
    said = [r.getMessage() for r in caplog.records if "cross-dimer redesign" in r.getMessage()]
    assert said == ["g.fasta: cross-dimer redesign: 2 rounds, 3 candidates banned, 1 picks dropped, 5 probes kept"]
    assert not any("cross-dimer filter" in r.getMessage() for r in caplog.records)
    assert cd.walk(_read(out), 30).all()
    # one round only: the three probes, and the warning
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        capped = run("capped.fasta", "--max-cross-dimer", "30", "--cross-dimer-redesign", "--cross-dimer-rounds", "1")
    assert _starts(g, _read(capped)) == [0, 100, 300]
    assert any("group 1: round cap 1 reached, 1 picks dropped without a redesign" in r.getMessage() for r in caplog.records)
    # a threshold nothing reaches: the plain design, byte for byte
    same = run("same.fasta", "--max-cross-dimer", "100", "--cross-dimer-redesign")
    assert open(same, "rb").read() == open(plain, "rb").read()
    # --write-probe-report keeps its contract: the report of the output, judged with this run's options
    from catch_amd import probe_report
    report, again = str(tmp_path / "report.tsv"), str(tmp_path / "again.tsv")
    out = run("reported.fasta", "--max-cross-dimer", "30", "--cross-dimer-redesign", "--write-probe-report", report)
    probe_report.main(probe_report.parse_args(["-f", out, "-o", again, "--max-cross-dimer", "30"]))
    capsys.readouterr()
    assert open(report).read() == open(again).read()
    assert all(line.endswith("\tok") for line in open(report).read().splitlines()[1:])


@pytest.mark.gpu
def test_library_attributes_and_the_host_path_on_the_provable_case(ctx, monkeypatch):
    from catch_amd.genome import Genome
    g = _provable()
    w = _windows(g)
    genomes = [[Genome.from_one_seq(g)]]
    outs = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        f = _filter(m=0, e=0, max_cross_dimer=30)
        ids = f._filter_strs([w], genomes, assume_unique=True)[0]
        assert [STARTS[i] for i in ids] == [0, 100, 300, 225, 125]
        assert (f.last_cross_rounds, f.last_cross_banned, f.last_cross_dropped) == ([2], [3], [1])
        t = f.last_timings
        assert t["cross_rounds"] == 2 and t["ban_pairs"] == 13 * 3 and t["picks"] == 5
        assert (t["ban_ms"] > 0.0) == (not host)
        outs.append(ids)
    assert outs[0] == outs[1]


@pytest.mark.gpu
def test_two_datasets(ctx, tmp_path, capsys, caplog):
    """G has no planted stretch; H holds the reverse complement of G's first 31 bases: H's windows 150, 175 and 200
    conflict with G's window 0, are banned before H's first solve, and H needs one round."""
    from catch_amd import design
    from catch_amd.genome import Genome
    cd = _cd()
    G = _genome(1)
    H = _genome(2, _rc(G[0:31]))
    wg, wh = _windows(G), _windows(H)
    m = cd.run_matrix(wg + wh)
    assert {(i, j) for i in range(26) for j in range(i + 1, 26) if m[i, j] > 30} == {(0, 13 + 6), (0, 13 + 7), (0, 13 + 8)}
    fa, fb = _write_fasta(tmp_path / "G.fasta", [("G", G)]), _write_fasta(tmp_path / "H.fasta", [("H", H)])
    out = str(tmp_path / "out.fasta")
    with caplog.at_level(logging.INFO):
        design.main(design.parse_args([fa, fb] + BASE + ["-o", out, "--max-cross-dimer", "30", "--cross-dimer-redesign",
                                                         "--verbose"]))
    capsys.readouterr()
    said = [r.getMessage() for r in caplog.records if "cross-dimer redesign" in r.getMessage()]
    assert said == ["G.fasta: cross-dimer redesign: 1 rounds, 0 candidates banned, 0 picks dropped, 4 probes kept",
                    "H.fasta: cross-dimer redesign: 1 rounds, 3 candidates banned, 0 picks dropped, 5 probes kept"]
    model = _model(ctx, [wg, wh], [[Genome.from_one_seq(G)], [Genome.from_one_seq(H)]], 30, 8, m=0, e=0)
    assert [(r, d) for _k, r, d in model] == [(1, 0), (1, 0)]
    assert sorted(_starts(G, model[0][0])) == [0, 100, 200, 300]
    assert sorted(_starts(H, model[1][0])) == [0, 100, 125, 225, 300]
    probes = _read(out)
    assert probes == model[0][0] + model[1][0]
    assert cd.walk(probes, 30).all() and int(cd.run_matrix(probes).max()) <= 30
    f = _filter(m=0, e=0, max_cross_dimer=30)
    ids = f._filter_strs([wg, wh], [[Genome.from_one_seq(G)], [Genome.from_one_seq(H)]], assume_unique=True)
    assert [[w[i] for i in sel] for w, sel in zip((wg, wh), ids)] == [model[0][0], model[1][0]]
    assert (f.last_cross_rounds, f.last_cross_banned, f.last_cross_dropped) == ([1, 1], [0, 3], [0, 0])


# ------------------------------------------------------------------ real data
def _covered(ctx, strs, genomes):
    """Bases of every genome that the probes cover, at 4 mismatches and extension 50."""
    from catch_amd import engine, probe
    k, uniq, owner, ep, eo = probe.anchor_table(strs, 4, 100, min_k=20, k=20)
    targets = engine.Targets(ctx, [g.seqs for g in genomes])
    probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
    rows = engine.Rows.scan(ctx, probes, targets, 4, 100, 0, 50)
    try:
        return rows.stats(len(genomes))[1]
    finally:
        for h in (rows, probes, targets):
            h.close()


@pytest.mark.gpu
def test_real_genomes_in_both_orientations_equal_the_loop_of_the_definition(ctx):
    """The five Ebola genomes of test_either_strand._mixed() (two of them reverse-complemented) as one group, candidates
    of 100 bases at stride 50, 4 mismatches, extension 50, full coverage, X = 30, at most 8 rounds: the values the
    issue names; they meet both conditions below as they stand."""
    cd = _cd()
    genomes, cands = _mixed()
    X, R = 30, 8
    plain = [cands[i] for i in _filter()._filter_strs([cands], [genomes], assume_unique=True)[0]]
    keep = cd.walk(plain, X)
    post = [p for p, k in zip(plain, keep) if k]
    f = _filter(max_cross_dimer=X, cross_dimer_rounds=R)
    got = [cands[i] for i in f._filter_strs([cands], [genomes], assume_unique=True)[0]]
    (want, rounds, dropped), = _model(ctx, [cands], [genomes], X, R)
    print("plain %d, post-filter %d, redesign %d probes in %d rounds, %d picks dropped, %d candidates banned of %d"
          % (len(plain), len(post), len(got), rounds, dropped, f.last_cross_banned[0], len(cands)))
    # conditions: something is repaired here
    assert len(post) < len(plain)
    assert rounds >= 2
    assert got == want
    assert (f.last_cross_rounds, f.last_cross_dropped) == ([rounds], [dropped])
    assert f.last_timings["cross_rounds"] == rounds and f.last_timings["ban_pairs"] > 0 and f.last_timings["ban_ms"] > 0
    assert cd.walk(got, X).all()
    have, before = _covered(ctx, got, genomes), _covered(ctx, post, genomes)
    print("covered per genome: redesign %s, post-filter %s" % (have.tolist(), before.tolist()))
    assert (have >= before).all()


@pytest.mark.gpu
def test_real_genomes_beside_owned_probes(ctx):
    """The first two genomes, the second one reverse-complemented: the design of the first is the owned panel, the new
    probes for both must not anneal to it."""
    from catch_amd import engine
    cd = _cd()
    genomes, _cands = _mixed()
    from test_extend_probes import _candidates
    two = genomes[:2]
    first, both = _candidates(two[:1]), _candidates(two)
    X = 30
    owned = [first[i] for i in _filter(max_cross_dimer=X)._filter_strs([first], [two[:1]], assume_unique=True)[0]]
    assert cd.walk(owned, X).all()
    # the extension alone anneals to the panel
    ext = [both[i] for i in _filter(fixed_probes=owned)._filter_strs([both], [two], assume_unique=True)[0]]
    assert engine.cross_against_flags(ctx, ext, owned, X).any()
    f = _filter(fixed_probes=owned, max_cross_dimer=X)
    new = [both[i] for i in f._filter_strs([both], [two], assume_unique=True)[0]]
    (want, rounds, dropped), = _model(ctx, [both], [two], X, 8, E=owned)
    assert new == want and (f.last_cross_rounds, f.last_cross_dropped) == ([rounds], [dropped])
    assert len(new) > 0 and not engine.cross_against_flags(ctx, new, owned, X).any()
    assert cd.walk(owned + new, X).all()
