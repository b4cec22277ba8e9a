"""--max-cross-dimer-dg and --cross-dimer-dg through the filter, the set cover filter's redesign rounds, the design
command and the probe report (catch_amd/filter/cross_duplex.py has the rule): the host-front-end legs without a GPU;
on the GPU the provable case of test_cross_dimer_redesign.py under the energy rule and the five Ebola genomes of
test_cross_dimer_design.py, two of them reverse-complemented.  The models are cross_duplex.py's NumPy forms."""
import logging

import numpy as np
import pytest

from test_cross_dimer_redesign import BASE as SMALL, STARTS, _covered, _filter, _genome, _provable, _rc, _starts, _windows
from test_either_strand import _mixed, _write_fasta

REAL = ["-pl", "100", "-ps", "200", "-m", "4", "-l", "100", "-e", "50", "-c", "0.75"]
G_SMALL = "30"          # kcal/mol: the planted 31 pairs of the provable case give 33.28, every other pair at most 25.05
G_REAL = "40"           # about 30 pairs of average composition, the length tests' X


def _cx():
    from catch_amd.filter import cross_duplex
    return cross_duplex


def _read(path):
    from catch_amd.utils import seq_io
    return list(seq_io.iterate_fasta(str(path)))


def _walk(matrix, above):
    keep = []
    for i in range(matrix.shape[0]):
        keep.append(not any(keep[j] and matrix[i, j] > above for j in range(i)))
    return np.array(keep, dtype=bool)


# ------------------------------------------------------------------ without a GPU
def test_keywords_name_one_rule():
    cx = _cx()
    from catch_amd.filter import cross_dimer
    off, on = _filter(), _filter(max_cross_dimer_dg=G_SMALL)
    assert off.cross_rule is None and off.max_cross_dimer_dg is None and not off.needs_rows
    assert isinstance(on.cross_rule, cx.DgRule) and on.cross_rule.above == 3000 and on.needs_rows
    assert on.max_cross_dimer is None and on.max_cross_dimer_dg == G_SMALL and on.cross_dimer_rounds == 8
    length = _filter(max_cross_dimer=30, cross_dimer_rounds=3)
    assert isinstance(length.cross_rule, cross_dimer.LengthRule) and length.cross_rule.above == 30
    assert length.max_cross_dimer == 30 and length.max_cross_dimer_dg is None and length.cross_dimer_rounds == 3
    assert _filter(max_cross_dimer_dg="17.92").cross_rule.above == 1792
    with pytest.raises(ValueError, match="one"):
        _filter(max_cross_dimer=30, max_cross_dimer_dg=G_SMALL)
    for bad in (-1, "600.5", 2.5, "x", True):
        with pytest.raises(ValueError):
            _filter(max_cross_dimer_dg=bad)
    with pytest.raises(ValueError, match="cross_dimer_rounds"):
        _filter(max_cross_dimer_dg=G_SMALL, cross_dimer_rounds=0)
    for kw in (dict(coverage_depth=2), dict(prune_redundant=True), dict(max_probes=5), dict(pick_gains=True)):
        with pytest.raises(NotImplementedError, match="max_cross_dimer_dg"):
            _filter(max_cross_dimer_dg=G_SMALL, **kw)


def test_command_line_errors(tmp_path, capsys):
    from catch_amd import design, design_grid, design_naively, probe_report, prune_probes
    fa = _write_fasta(tmp_path / "t.fasta", [("a", "ACGT" * 100)])
    out, report = str(tmp_path / "o.fasta"), str(tmp_path / "r.tsv")
    on = [fa, "-o", out, "--max-cross-dimer-dg", "25"]
    for argv, said in (
            (on + ["--max-cross-dimer", "30"], "two conflict rules"),
            (on + ["--add-reverse-complements"], "--max-cross-dimer-dg cannot go with --add-reverse-complements"),
            (on + ["--skip-set-cover"], "--max-cross-dimer-dg cannot go with --skip-set-cover"),
            ([fa, "-o", out, "--cross-dimer-dg"], "--cross-dimer-dg adds columns to --write-probe-report"),
            ([fa, "-o", out, "--max-cross-dimer-dg", "-1"], "0 .. 600"),
            ([fa, "-o", out, "--max-cross-dimer-dg", "600.01"], "0 .. 600"),
            ([fa, "-o", out, "--max-cross-dimer-dg", "x"], "not a number"),
            ([fa, "-o", out, "--cross-dimer-redesign"], "needs --max-cross-dimer"),
            (on + ["--cross-dimer-redesign", "--max-probes", "10"], "--max-probes")):
        for args_type in ("basic", "large"):
            with pytest.raises(SystemExit) as exc:
                design.parse_args(argv, args_type=args_type)
            assert exc.value.code == 2
            assert said in capsys.readouterr().err, argv
    args = design.parse_args(on + ["--cross-dimer-redesign"])
    assert args.max_cross_dimer_dg == "25" and args.max_cross_dimer is None and args.cross_dimer_rounds == 8
    args = design.parse_args([fa, "-o", out, "--cross-dimer-dg", "--cross-dimer", "--write-probe-report", report])
    assert args.cross_dimer_dg and args.max_cross_dimer_dg is None
    # in the report the two families are independent: both thresholds may be given
    args = probe_report.parse_args(["-f", fa, "--max-cross-dimer", "20", "--max-cross-dimer-dg", "25/2"])
    judge = probe_report.Judge(args, load=False)
    assert (judge.max_cross_dimer, judge.max_cross_dg, judge.cross_dimer, judge.cross_dg) == (20, 1250, True, True)
    with pytest.raises(SystemExit):
        probe_report.parse_args(["-f", fa, "--max-cross-dimer-dg", "700"])
    capsys.readouterr()
    # the other commands do not learn the options
    for parse, argv in ((design_grid.parse_args, [fa, "-o", out, "--grid-mismatches", "1", "--grid-cover-extension", "0"]),
                        (design_naively.parse_args, [fa, "-o", out]), (prune_probes.parse_args, [])):
        with pytest.raises(SystemExit):
            parse(argv + ["--max-cross-dimer-dg", "25"])
        capsys.readouterr()


def _small_records():
    probe = "CACACA" + "AT" * 8 + "CACACA" + "GC" * 5 + "CACACA"
    return [probe, "TCTCTC" + "AT" * 8 + "TCTCTC", "TCTCTC" + "GC" * 5 + "TCTCTC", "ACCATTCAACTTACCATCACTCCAATCTAC", "NNNN", "A"]


def test_probe_report_on_the_host_path(tmp_path, monkeypatch, capsys):
    from catch_amd import probe_report
    cx = _cx()
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    seqs = _small_records()
    fa = _write_fasta(tmp_path / "p.fasta", [("r%d" % i, s) for i, s in enumerate(seqs)])
    panel = _write_fasta(tmp_path / "panel.fasta", [("a", "GGGG" + "GC" * 5), ("b", "AT" * 8)])
    length_only, both, dg_only, judged = (str(tmp_path / n) for n in ("l.tsv", "b.tsv", "d.tsv", "j.tsv"))
    length_opts = ["--max-cross-dimer", "12", "--cross-dimer-against", panel]
    probe_report.main(probe_report.parse_args(["-f", fa, "-o", length_only] + length_opts))
    probe_report.main(probe_report.parse_args(["-f", fa, "-o", both, "--cross-dimer-dg"] + length_opts))
    old = [line.split("\t") for line in open(length_only).read().splitlines()]
    new = [line.split("\t") for line in open(both).read().splitlines()]
    assert old[0][-5:] == ["cross_dimer", "cross_partner", "cross_against", "cross_against_partner", "verdict"]
    assert new[0][-5:] == ["cross_dg", "cross_dg_partner", "cross_dg_against", "cross_dg_against_partner", "verdict"]
    # the columns of the length options and the verdict are what they are without the new option
    assert [r[:-5] + r[-1:] for r in new] == old
    values, partners = cx.dcross_list(seqs)
    panel_seqs = ["GGGG" + "GC" * 5, "AT" * 8]
    against = [cx.cross_duplex_against(s, panel_seqs) for s in seqs]
    assert [r[-5:-1] for r in new[1:]] == [
        [str(v), str(p + 1) if v else "NA", str(av), str(ap + 1) if av else "NA"]
        for v, p, (av, ap) in zip(values, partners, against)]
    assert partners[0] == 2 and new[1][-5:-3] == [str(values[0]), "3"] and old[1][-5:-3] == ["17", "2"]
    # --cross-dimer-dg alone: its two columns where they would stand, no verdict
    probe_report.main(probe_report.parse_args(["-f", fa, "-o", dg_only, "--cross-dimer-dg"]))
    rows = [line.split("\t") for line in open(dg_only).read().splitlines()]
    assert rows[0][-3:] == ["background_hits", "cross_dg", "cross_dg_partner"]
    assert [r[-2:] for r in rows[1:]] == [r[-5:-3] for r in new[1:]]
    # the threshold implies the columns and names its two rules; exactly at a value is no conflict
    failed = probe_report.main(probe_report.parse_args(
        ["-f", fa, "-o", judged, "--max-cross-dimer-dg", "15", "--cross-dimer-against", panel]))
    rows = [line.split("\t") for line in open(judged).read().splitlines()]
    assert rows[0][-7:] == ["cross_against", "cross_against_partner", "cross_dg", "cross_dg_partner", "cross_dg_against",
                            "cross_dg_against_partner", "verdict"]
    want = [[name for name, v in (("cross-dg", values[i]), ("cross-dg-against", against[i][0])) if v > 1500]
            for i in range(len(seqs))]
    assert failed == want and want[0] == ["cross-dg", "cross-dg-against"] and want[1] == [] and want[2] == want[0]
    assert [r[-1] for r in rows[1:]] == [",".join(w) if w else "ok" for w in want]
    exact = "%d/100" % values[0]
    failed = probe_report.main(probe_report.parse_args(["-f", fa, "-o", judged, "--max-cross-dimer-dg", exact]))
    assert failed[0] == [] and failed[2] == []
    capsys.readouterr()


# ------------------------------------------------------------------ small and provable, on the GPU
@pytest.mark.gpu
def test_the_provable_case_through_the_command(ctx, tmp_path, capsys, caplog):
    from catch_amd import design, probe_report
    cx = _cx()
    g = _provable()
    w = _windows(g)
    m = cx.duplex_matrix(w)
    gc = cx.threshold(G_SMALL)
    assert {(STARTS[i], STARTS[j]) for i in range(13) for j in range(i + 1, 13) if m[i, j] > gc} == {
        (0, 150), (0, 175), (0, 200)}
    fa = _write_fasta(tmp_path / "g.fasta", [("g", g)])

    def run(name, *more):
        out = str(tmp_path / name)
        design.main(design.parse_args([fa] + SMALL + ["-o", out] + list(more)))
        capsys.readouterr()
        return out
    plain = run("plain.fasta")
    assert sorted(_starts(g, _read(plain))) == [0, 100, 200, 300]
    # the post-filter: the earlier probe of the pair stays, the later one goes
    with caplog.at_level(logging.INFO, logger="catch_amd.design"):
        dropped = run("dropped.fasta", "--max-cross-dimer-dg", G_SMALL, "--verbose")
    assert _starts(g, _read(dropped)) == [s for s in _starts(g, _read(plain)) if s != 200]
    said = [r.getMessage() for r in caplog.records if "cross-dimer filter" in r.getMessage()]
    kept = [w[STARTS.index(s)] for s in _starts(g, _read(dropped))]
    assert said == ["cross-dimer filter: 1 of 4 probes dropped (largest cross-dimer dG %d before, %d after)"
                    % (int(m[0, 8]), int(cx.dcross_numpy(kept)[0].max()))]
    # the redesign: what the length rule gives at X = 30 (test_cross_dimer_redesign.py), from the energy rule
    caplog.clear()
    with caplog.at_level(logging.INFO):
        out = run("redesign.fasta", "--max-cross-dimer-dg", G_SMALL, "--cross-dimer-redesign", "--verbose")
    assert _starts(g, _read(out)) == [0, 100, 300, 225, 125]
    said = [r.getMessage() for r in caplog.records if "cross-dimer redesign" in r.getMessage()]
    assert said == ["g.fasta: cross-dimer redesign: 2 rounds, 3 candidates banned, 1 picks dropped, 5 probes kept"]
    assert cx.walk(_read(out), gc).all()
    # G = 600: the plain design, byte for byte, from the filter and from the redesign
    for more in (("--max-cross-dimer-dg", "600"), ("--max-cross-dimer-dg", "600", "--cross-dimer-redesign")):
        assert open(run("same.fasta", *more), "rb").read() == open(plain, "rb").read()
    # --write-probe-report keeps its contract, with the threshold and with the columns alone
    report, again = str(tmp_path / "report.tsv"), str(tmp_path / "again.tsv")
    for more in (["--max-cross-dimer-dg", G_SMALL], ["--cross-dimer-dg"], ["--cross-dimer-dg", "--cross-dimer"]):
        out = run("reported.fasta", "--write-probe-report", report, *more)
        probe_report.main(probe_report.parse_args(["-f", out, "-o", again] + more))
        capsys.readouterr()
        assert open(report).read() == open(again).read()
        rows = [line.split("\t") for line in open(report).read().splitlines()]
        if "--max-cross-dimer-dg" in more:
            assert rows[0][-3:] == ["cross_dg", "cross_dg_partner", "verdict"] and all(r[-1] == "ok" for r in rows[1:])
        else:
            assert rows[0][-2:] == ["cross_dg", "cross_dg_partner"] and len(rows) == 5
            assert "%d" % int(m[0, 8]) in [r[-2] for r in rows[1:]]


@pytest.mark.gpu
def test_host_and_device_paths_pick_the_same_probes(ctx, monkeypatch):
    from catch_amd.genome import Genome
    G = _genome(1)
    H = _genome(2, _rc(G[0:31]))
    groups, genomes = [_windows(G), _windows(H)], [[Genome.from_one_seq(G)], [Genome.from_one_seq(H)]]
    outs = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        f = _filter(m=0, e=0, max_cross_dimer_dg=G_SMALL)
        ids = f._filter_strs(groups, genomes, assume_unique=True)
        assert (f.last_cross_rounds, f.last_cross_banned, f.last_cross_dropped) == ([1, 1], [0, 3], [0, 0])
        assert (f.last_timings["ban_ms"] > 0.0) == (not host) and f.last_timings["ban_pairs"] == 13 * 4
        outs.append(ids)
    assert outs[0] == outs[1]
    assert sorted(_starts(H, [groups[1][i] for i in outs[0][1]])) == [0, 100, 125, 225, 300]


# ------------------------------------------------------------------ real data, on the GPU
_cache = {}


def _plain(tmp_path_factory, capsys):
    """The plain design of the five genomes (two of them reverse-complemented), and the duplex matrix of its probes."""
    if "p" not in _cache:
        from catch_amd import design
        genomes, _cands = _mixed()
        d = tmp_path_factory.mktemp("cross_duplex")
        fa = _write_fasta(d / "mixed.fasta", [("g%d" % j, g.seqs[0]) for j, g in enumerate(genomes)])
        out = str(d / "plain.fasta")
        design.main(design.parse_args([fa] + REAL + ["-o", out]))
        capsys.readouterr()
        probes = _read(out)
        _cache["p"] = (fa, out, probes, _cx().duplex_matrix(probes))
    return _cache["p"]


@pytest.mark.gpu
def test_design_keeps_what_the_host_walk_keeps_on_real_probes(ctx, tmp_path_factory, tmp_path, capsys):
    from catch_amd import design, engine, probe_report
    cx = _cx()
    fa, plain, probes, m = _plain(tmp_path_factory, capsys)
    gc, n = cx.threshold(G_REAL), len(probes)
    keep = _walk(m, gc)
    print("probes %d, largest dcross %d, kept at G = %s: %d" % (n, int(m.max()), G_REAL, int(keep.sum())))
    assert n >= 50 and 0 < int(keep.sum()) < n          # G drops some picks, not all
    capsys.readouterr()
    values, partners = engine.cross_duplex(ctx, probes)
    assert values.tolist() == m.max(axis=1).tolist() and partners.tolist() == m.argmax(axis=1).tolist()
    out = str(tmp_path / "kept.fasta")
    design.main(design.parse_args([fa] + REAL + ["-o", out, "--max-cross-dimer-dg", G_REAL]))
    assert capsys.readouterr().out.split() == [str(int(keep.sum()))]
    got = _read(out)
    assert got == [s for s, k in zip(probes, keep) if k]
    # no two output probes conflict, and of every conflicting pair of picks the earlier one stayed
    assert int(cx.duplex_matrix(got).max()) <= gc
    first = int(np.flatnonzero(~keep)[0])
    assert any(keep[j] and m[first, j] > gc for j in range(first))
    # G = 600 is the plain design, byte for byte
    same = str(tmp_path / "same.fasta")
    design.main(design.parse_args([fa] + REAL + ["-o", same, "--max-cross-dimer-dg", "600"]))
    capsys.readouterr()
    assert open(same, "rb").read() == open(plain, "rb").read()
    # the report on the device equals the NumPy form
    report = str(tmp_path / "r.tsv")
    probe_report.main(probe_report.parse_args(["-f", plain, "-o", report, "--max-cross-dimer-dg", G_REAL]))
    capsys.readouterr()
    rows = [line.split("\t") for line in open(report).read().splitlines()]
    assert rows[0][-3:] == ["cross_dg", "cross_dg_partner", "verdict"]
    assert [r[-3] for r in rows[1:]] == [str(int(v)) for v in m.max(axis=1)]
    assert [r[-1] for r in rows[1:]] == ["cross-dg" if v > gc else "ok" for v in m.max(axis=1)]


def _model(ctx, C, gs, gc, R, E=()):
    """_cross_rounds' definition for one group, spelled out under the energy rule: SetCoverFilter(fixed_probes=...)
    once per round, engine.cross_duplex_against_flags (held to the NumPy form in test_cross_duplex.py) and the host
    walk -> (selected strings in the order kept, rounds, picks dropped)."""
    from catch_amd import engine
    cx = _cx()
    Kg, rounds, dropped = [], 0, 0
    while True:
        against = list(E) + Kg
        flags = engine.cross_duplex_against_flags(ctx, C, against, gc) if against else np.zeros(len(C), bool)
        A = [c for c, f in zip(C, flags) if c not in set(Kg) and not f]
        picks = []
        if A:
            f = _filter(fixed_probes=against) if against else _filter()
            picks = [A[i] for i in f._filter_strs([A], [gs], assume_unique=True)[0]]
        keep = cx.walk(picks, gc)
        kept = [p for p, k in zip(picks, keep) if k]
        Kg += kept
        rounds += 1
        dropped += len(picks) - len(kept)
        if not picks or len(kept) == len(picks) or rounds == R:
            return Kg, rounds, dropped


@pytest.mark.gpu
def test_redesign_on_real_genomes_in_both_orientations(ctx):
    """The inputs of test_cross_dimer_redesign.py's real-data test under the energy rule: no conflict in the output,
    the coverage of the reversed genomes restored, the selection that of the definition's loop."""
    cx = _cx()
    genomes, cands = _mixed()
    gc, R = cx.threshold(G_REAL), 8
    plain = [cands[i] for i in _filter()._filter_strs([cands], [genomes], assume_unique=True)[0]]
    post = [p for p, k in zip(plain, cx.walk(plain, gc)) if k]
    f = _filter(max_cross_dimer_dg=G_REAL, cross_dimer_rounds=R)
    got = [cands[i] for i in f._filter_strs([cands], [genomes], assume_unique=True)[0]]
    want, rounds, dropped = _model(ctx, cands, genomes, gc, R)
    print("plain %d, post-filter %d, redesign %d probes in %d rounds, %d picks dropped, %d candidates banned of %d"
          % (len(plain), len(post), len(got), rounds, dropped, f.last_cross_banned[0], len(cands)))
    assert len(post) < len(plain) and rounds >= 2          # something is repaired here
    assert got == want
    assert (f.last_cross_rounds, f.last_cross_dropped) == ([rounds], [dropped])
    assert f.last_timings["cross_rounds"] == rounds and f.last_timings["ban_pairs"] > 0 and f.last_timings["ban_ms"] > 0
    assert cx.walk(got, gc).all()                          # (every probe kept: no pair of the output conflicts)
    have, before = _covered(ctx, got, genomes), _covered(ctx, post, genomes)
    print("covered per genome: redesign %s, post-filter %s" % (have.tolist(), before.tolist()))
    assert (have >= before).all() and (have > before).any()


@pytest.mark.gpu
def test_redesign_beside_owned_probes(ctx):
    """The first two genomes, the second one reverse-complemented: the design of the first is the owned panel
    (--extend-probes), and the new probes for both must not anneal to it."""
    from catch_amd import engine
    from test_extend_probes import _candidates
    cx = _cx()
    genomes, _cands = _mixed()
    two = genomes[:2]
    first, both = _candidates(two[:1]), _candidates(two)
    gc = cx.threshold(G_REAL)
    owned = [first[i] for i in _filter(max_cross_dimer_dg=G_REAL)._filter_strs([first], [two[:1]], assume_unique=True)[0]]
    assert cx.walk(owned, gc).all()
    ext = [both[i] for i in _filter(fixed_probes=owned)._filter_strs([both], [two], assume_unique=True)[0]]
    assert engine.cross_duplex_against_flags(ctx, ext, owned, gc).any()      # the extension alone anneals to the panel
    f = _filter(fixed_probes=owned, max_cross_dimer_dg=G_REAL)
    new = [both[i] for i in f._filter_strs([both], [two], assume_unique=True)[0]]
    want, rounds, dropped = _model(ctx, both, two, gc, 8, E=owned)
    assert new == want and (f.last_cross_rounds, f.last_cross_dropped) == ([rounds], [dropped])
    assert len(new) > 0 and not engine.cross_duplex_against_flags(ctx, new, owned, gc).any()
    assert cx.walk(owned + new, gc).all()
