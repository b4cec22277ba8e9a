"""The design command's optional filters: poly(A) (a kernel on the device front
end, catchhip_candidates_drop_polya), FASTA, N expansion, reverse complements,
--skip-set-cover and the two --limit-target-genomes options -- against
tests/golden/design_filters.json.gz, recorded from the live reference by
tests/golden/make_design_filters_golden.py."""
import argparse
import functools
import gzip
import json
import logging
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EBOLA = os.path.join(GOLDEN, "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
POLYA_COMBOS = [(ln, mm, gate) for ln in ("4", "12", "L", "L+1") for mm in (0, 1, 2, 4) for gate in (0, 6)]


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(GOLDEN, "design_filters.json.gz"), "rt") as f:
        return json.load(f)


def _write_records(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _read_records(path):
    recs = []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                recs.append([line[1:], ""])
            else:
                recs[-1][1] += line
    return recs


def _ebola_records(n):
    recs = []
    with gzip.open(EBOLA, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if len(recs) == n:
                    break
                recs.append([line[1:], ""])
            else:
                recs[-1][1] += line
    return recs


# ------------------------------------------------------------------ host
def test_polya_filter_host_equals_reference():
    """_filter (objects), _filter_strs on mixed lengths (per string) and on equal lengths (NumPy) all keep what the
    reference's PolyAFilter kept, string by string."""
    from catch_amd import probe
    from catch_amd.filter.polya_filter import PolyAFilter
    g = golden()["polya"]
    assert len(g["cases"]) >= 2000 and g["gate_decides"] >= 50
    by_combo = {}
    for s, length, mm, gate, kept in g["cases"]:
        by_combo.setdefault((length, mm, gate), []).append((s, kept))
    for (length, mm, gate), cases in by_combo.items():
        f = PolyAFilter(length, mm, min_exact_length_to_consider=gate)
        strs = [s for s, _ in cases]
        want = [s for s, kept in cases if kept]
        assert [p.seq_str for p in f._filter([probe.Probe.from_str(s) for s in strs])] == want
        assert [s for s in strs if f._keeps(s)] == want
        assert f._filter_strs(strs + strs[:1] * 3) == want + ([strs[0]] * 3 if cases[0][1] else [])
    defaults = PolyAFilter(12, 2)
    assert (defaults.length, defaults.mismatches, defaults.min_exact_length_to_consider) == (12, 2, 6)
    assert defaults._filter([]) == [] and defaults._filter_strs([]) == []


def test_polya_filter_on_ebola_candidates_drops_what_the_reference_drops():
    """First 10 Ebola records, -pl 100 -ps 50: the reference's candidate generator, DuplicateFilter and
    PolyAFilter(12, 2) give 3,778 candidates, 3,063 unique ones, 46 of them dropped.  (Stride windows alone, without
    the window flush with each sequence's end, are 3,056 unique and 43 dropped.)"""
    from catch_amd.filter import candidate_probes
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.utils import seq_io
    cand = []
    for g in seq_io.read_genomes_from_fasta(EBOLA)[:10]:
        cand += candidate_probes.candidate_strings_from_sequences(list(g.seqs), 100, 50)
    uniq = list(dict.fromkeys(cand))
    f = PolyAFilter(12, 2)
    kept = f._filter_strs(uniq)
    assert (len(cand), len(uniq), len(uniq) - len(kept)) == (3778, 3063, 46)
    # before or after the duplicate filter: the same list
    assert list(dict.fromkeys(f._filter_strs(cand))) == kept
    assert kept == [s for s in uniq if f._keeps(s)]


def test_fasta_filter_equals_reference(tmp_path):
    from catch_amd import probe
    from catch_amd.filter.fasta_filter import FastaFilter
    g = golden()["fasta"]
    fn = tmp_path / "keep.fasta"
    fn.write_text(g["fasta"])
    assert FastaFilter(str(fn)).skip_reverse_complements is False
    for skip, key in ((False, "all"), (True, "skip")):
        f = FastaFilter(str(fn), skip_reverse_complements=skip)
        assert f._filter_strs(g["candidates"]) == g["kept"][key]
        assert [p.seq_str for p in f._filter([probe.Probe.from_str(c) for c in g["candidates"]])] == g["kept"][key]
    assert g["kept"]["all"] != g["kept"]["skip"]


def test_n_expansion_filter_equals_reference_draw_for_draw():
    from catch_amd import probe
    from catch_amd.filter.n_expansion_filter import NExpansionFilter
    g = golden()["nexp"]
    assert NExpansionFilter().limit_n_expansion_randomly == 3
    assert sorted(set(p.count("N") for p in g["probes"])) == [0, 1, 2, 3, 5]
    for case in g["cases"]:
        f = NExpansionFilter(limit_n_expansion_randomly=case["limit"])
        random.seed(case["seed"])
        assert [p.seq_str for p in f._filter([probe.Probe.from_str(p) for p in g["probes"]])] == case["out"]
        assert random.random() == case["next_draw"]
        random.seed(case["seed"])
        assert f._filter_strs(g["probes"]) == case["out"]
    # first N first, bases in the order A, T, C, G
    assert NExpansionFilter(None)._filter_strs(["ANNA"])[:5] == ["AAAA", "AATA", "AACA", "AAGA", "ATAA"]


def test_reverse_complement_filter_equals_reference():
    from catch_amd import probe
    from catch_amd.filter.reverse_complement_filter import ReverseComplementFilter
    g = golden()["rc"]
    assert any("N" in p for p in g["probes"])
    out = ReverseComplementFilter()._filter([probe.Probe.from_str(p) for p in g["probes"]])
    assert [[p.header, p.seq_str] for p in out] == g["out"]
    assert probe.Probe.from_str("ACGTNX").reverse_complement().seq_str == "XNACGT"


def _parser_of(parse, monkeypatch, *args):
    """The ArgumentParser a parse_args function builds."""
    caught = []

    class Caught(Exception):
        pass

    def grab(self, *a, **k):
        caught.append(self)
        raise Caught()
    with monkeypatch.context() as m:
        m.setattr(argparse.ArgumentParser, "parse_args", grab)
        with pytest.raises(Caught):
            parse(*args)
    return caught[0]


def test_option_surface_equals_reference(monkeypatch):
    from catch_amd import design, design_large
    want = golden()["options"]
    assert len(want) == 7
    assert design_large.design is design            # (design_large: the same parser, "large" profile)
    for profile in ("basic", "large"):
        parser = _parser_of(design.parse_args, monkeypatch, ["x.fasta"], profile)
        for w in want:
            act = [a for a in parser._actions if w["option"] in a.option_strings]
            assert len(act) == 1, w["option"]
            act = act[0]
            got = dict(option=w["option"], nargs=act.nargs, type=act.type.__name__ if act.type else None,
                       default=act.default, const=act.const, dest=act.dest)
            assert got == w
    a = design.parse_args(["x.fasta", "--filter-polya", "12", "2", "--expand-n"])
    assert (a.filter_polya, a.expand_n, a.skip_set_cover, a.add_reverse_complements) == ([12, 2], 3, False, False)
    assert design.parse_args(["x.fasta", "--expand-n", "0"]).expand_n == 0
    assert design.parse_args(["x.fasta"]).expand_n is None
    with pytest.raises(SystemExit):
        design.parse_args(["x.fasta", "--filter-polya", "12"])


def _design_without_designing(monkeypatch, argv):
    """design.main up to ProbeDesigner.design: returns the designer it built."""
    from catch_amd import design
    from catch_amd.filter import probe_designer
    made = []

    def fake_design(self):
        made.append(self)
        self.final_probes = []
    monkeypatch.setattr(probe_designer.ProbeDesigner, "design", fake_design)
    design.main(design.parse_args(argv))
    return made[0]


def test_errors_warnings_filter_order_and_limits(tmp_path, monkeypatch, caplog, capsys):
    from catch_amd import design
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    out = str(tmp_path / "o.fasta")
    with pytest.raises(Exception, match="Cannot --limit-target-genomes and "
                       "--limit-target-genomes-randomly-with-replacement at the same time"):
        design.main(design.parse_args([fa, "-o", out, "--limit-target-genomes", "2",
                                       "--limit-target-genomes-randomly-with-replacement", "2"]))
    with caplog.at_level(logging.WARNING):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--filter-polya", "120", "11"])
    text = caplog.text
    assert "Length of poly(A) stretch to filter (120) is greater than PROBE_LENGTH (100)" in text
    assert "mismatches to tolerate when searching for poly(A) stretches (11) is high" in text
    assert "is short" not in text
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        _design_without_designing(monkeypatch, [fa, "-o", out, "--filter-polya", "9", "2"])
    assert "Length of poly(A) stretch to filter (9) is short, and may lead to many probes being filtered" in caplog.text
    assert "is high" not in caplog.text and "greater than" not in caplog.text
    # bin/design.py:255-385: fasta, poly(A), dup | ndf, scf, adapters, N expansion, reverse complements
    pd = _design_without_designing(monkeypatch, [
        fa, "-o", out, "--add-reverse-complements", "--expand-n", "--add-adapters", "--filter-polya", "12", "2",
        "--filter-from-fasta", fa, "--filter-with-lsh-hamming", "0"])
    assert [type(f).__name__ for f in pd.filters] == [
        "FastaFilter", "PolyAFilter", "NearDuplicateFilterWithHammingDistance", "SetCoverFilter", "AdapterFilter",
        "NExpansionFilter", "ReverseComplementFilter"]
    assert pd.filters[0].skip_reverse_complements is True and pd.filters[5].limit_n_expansion_randomly == 3
    assert pd._strings_path_ok(pd.filters)
    pd = _design_without_designing(monkeypatch, [
        fa, "-o", out, "--skip-set-cover", "--filter-polya", "12", "2", "--cluster-and-design-separately", "0.2"])
    assert [type(f).__name__ for f in pd.filters] == ["PolyAFilter", "DuplicateFilter"]
    assert pd.cluster_merge_after is pd.filters[1]           # the filter that stood before the set cover
    assert not pd._strings_path_ok(pd.filters)
    # the limits: right after reading, the random one before any other draw
    pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--limit-target-genomes", "3"])
    everything = _design_without_designing(monkeypatch, [fa, "-o", out]).genomes[0]
    assert [g.seqs for g in pd.genomes[0]] == [g.seqs for g in everything[:3]]
    random.seed(7)
    pd = _design_without_designing(monkeypatch, [fa, fa, "-o", out, "--limit-target-genomes-randomly-with-replacement", "4"])
    random.seed(7)
    want = [random.choices(range(5), k=4) for _ in range(2)]
    assert [[g.seqs for g in grp] for grp in pd.genomes] == [[everything[i].seqs for i in w] for w in want]
    capsys.readouterr()


def test_symbol_declared_and_bound():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name in ("catchhip_candidates_drop_polya", "catchhip_candidates_multiplicities"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
    assert "polya_filter.py" in hdr           # cites what it replaces
    assert "prefilter.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert hasattr(engine.Candidates, "drop_polya")


def test_strings_path_and_front_end_mode(tmp_path, monkeypatch):
    from catch_amd import genome
    from catch_amd.filter import probe_designer
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.filter.fasta_filter import FastaFilter
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithHammingDistance
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    PD = probe_designer.ProbeDesigner
    paf, ff, dup = PolyAFilter(12, 2), FastaFilter(str(tmp_path / "none.fasta")), DuplicateFilter()
    ndf = NearDuplicateFilterWithHammingDistance(2, 100)
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    genomes = [[genome.Genome.from_one_seq("ACGT" * 100)]]
    pd = PD(genomes, [paf, dup, scf], probe_length=100, probe_stride=50)
    for filters in ([dup, scf], [paf, dup, scf], [paf, ndf, scf], [ff, paf, dup, scf], [paf, paf, ff, dup, scf, paf]):
        assert PD._strings_path_ok(filters), filters
    for filters in ([paf, dup], [ff, dup], [paf, scf], [dup, paf, scf], [paf]):
        assert not PD._strings_path_ok(filters), filters
    plain = pd._device_front_end_mode(genomes, dup, scf)
    assert plain == "per group"
    assert pd._device_front_end_mode(genomes, dup, scf, [paf]) == plain
    assert pd._device_front_end_mode(genomes, ndf, scf, [paf, paf]) == pd._device_front_end_mode(genomes, ndf, scf)
    many = [[genome.Genome.from_one_seq("ACGT" * 100)] for _ in range(9)]
    assert pd._device_front_end_mode(many, dup, scf, [paf]) == pd._device_front_end_mode(many, dup, scf) == "union"
    assert pd._device_front_end_mode(genomes, dup, scf, [ff]) is None
    assert pd._device_front_end_mode(genomes, dup, scf, [ff, paf]) is None
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    assert pd._device_front_end_mode(genomes, dup, scf, [paf]) is None


def test_design_grid_refuses_six_and_accepts_polya(tmp_path, capsys):
    from catch_amd import design_grid
    base = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", str(tmp_path)]
    assert design_grid.parse_args(base + ["--filter-polya", "12", "2"]).filter_polya == [12, 2]
    assert design_grid.parse_args(base).filter_polya is None
    for opt in (["--expand-n"], ["--expand-n", "0"], ["--add-reverse-complements"], ["--filter-from-fasta", "p.fasta"],
                ["--skip-set-cover"], ["--limit-target-genomes", "3"],
                ["--limit-target-genomes-randomly-with-replacement", "3"]):
        with pytest.raises(SystemExit):
            design_grid.parse_args(base + opt)
        err = capsys.readouterr().err
        assert opt[0] + " is not supported by a grid design" in err


# ------------------------------------------------------------------ GPU
def _np_keep(strs, L, length, mm, gate):
    """NumPy restatement of the rule: dropped iff an exact run of >= gate 'A' or 'T' (gate 0: always) and a window of
    >= length characters with <= mm mismatches against 'A' or against 'T' -- the longest such window is >= length iff
    some window of exactly `length` qualifies."""
    if not strs:
        return np.zeros(0, dtype=bool)
    rows = np.frombuffer("".join(strs).encode(), dtype=np.uint8).reshape(len(strs), L)

    def window(width, k):
        if width > L:
            return np.zeros(len(strs), dtype=bool)
        if width == 0:
            return np.ones(len(strs), dtype=bool)
        hit = np.zeros(len(strs), dtype=bool)
        for base in b"AT":
            w = np.lib.stride_tricks.sliding_window_view(rows != base, width, axis=1)
            hit |= w.sum(axis=2).min(axis=1) <= k
        return hit
    return ~(window(gate, 0) & window(length, mm))


def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


def _sequences_with_unique_windows(rng, L, stride, nuniq):
    """Sequences over ACGTN, A/T-heavy with planted stretches, whose windows hold exactly nuniq different strings,
    many of them more than once."""
    from catch_amd.filter import candidate_probes
    n = L + stride * (4 * nuniq + 50)
    s = rng.choice(list("ATCGN"), p=[0.42, 0.3, 0.12, 0.12, 0.04], size=n)
    for _ in range(n // 60):                        # stretches, some spoilt
        at, ln = int(rng.integers(0, n)), int(rng.integers(4, 30))
        s[at:at + ln] = rng.choice(list("AT"))
        if ln > 8:
            s[at + int(rng.integers(0, min(ln, n - at)))] = rng.choice(list("CGN"))
    s = "".join(s).replace("NN", "NA")
    # the shortest prefix whose stride windows hold nuniq different strings
    seen, m = set(), 0
    while len(seen) < nuniq:
        seen.add(s[m * stride:m * stride + L])
        m += 1
    s = s[:L + stride * (m - 1)]
    seqs = [s, s[:L + stride * (m // 2)], s[stride * (m // 3):]]      # the same windows again
    cand = [c for q in seqs for c in candidate_probes.candidate_strings_from_sequences([q], L, stride)]
    assert len(set(cand)) == nuniq and len(cand) > nuniq
    return seqs


# the kernel's workgroup by candidate length (csrc/prefilter.hip): rows copied into LDS at an odd pitch of
# 4 * ceil((L + 15) / 16) + 1 dwords, as many of 256 / 128 / 64 rows as fit 64 KB, and read from global memory when 64 do not
POLYA_TIER_EDGES = [(225, 40), (226, 40), (481, 97), (482, 97), (993, 200), (994, 200)]


def _polya_workgroup(L):
    """(rows per workgroup, bytes of dynamic LDS) of the poly(A) kernel's launch; (256, 0): unstaged."""
    pitch = 4 * ((L + 30) // 16) + 1
    for rows in (256, 128, 64):
        if rows * pitch * 4 <= 65536:
            return rows, rows * pitch * 4
    return 256, 0


def _polya_sizes(L):
    """Unique-candidate counts around one and two workgroups of every size the kernel uses."""
    if any(L == edge for edge, _ in POLYA_TIER_EDGES):
        return [1, 63, 64, 65, 127, 128, 129, 257]
    return [0, 1, 255, 256, 257] + ([3000] if L in (65, 100) else [])


def test_polya_tier_edges_sit_on_the_workgroup_sizes_claimed():
    """No GPU: the lengths added to the kernel test are the last of one workgroup size and the first of the next --
    256 rows up to 225 bases (62,464 bytes of LDS, the largest launch), 128 rows for 226..481, 64 rows for 482..993,
    unstaged from 994 -- and the lengths tested before all take 256 rows within 48 KB."""
    assert [_polya_workgroup(L) for L, _ in POLYA_TIER_EDGES] == [
        (256, 62464), (128, 33280), (128, 64000), (64, 33024), (64, 64768), (256, 0)]
    assert all(_polya_workgroup(L)[0] == 256 and 0 < _polya_workgroup(L)[1] <= 48 * 1024 for L in (8, 63, 64, 65, 100, 130))
    assert _polya_workgroup(130) == (256, 41984)
    for L, stride in POLYA_TIER_EDGES:
        sizes, rows = _polya_sizes(L), _polya_workgroup(L)[0]
        assert {63, 64, 65, 127, 128, 129} <= set(sizes) and max(sizes) > rows and stride < L


@pytest.mark.gpu
@pytest.mark.parametrize("L,stride", [(8, 3), (63, 20), (64, 32), (65, 17), (100, 50), (130, 50)] + POLYA_TIER_EDGES)
def test_drop_polya_kernel_equals_numpy(ctx, L, stride):
    """catchhip_candidates_drop_polya against the NumPy rule: the surviving positions, multiplicities and groups are
    the unfiltered list's, masked; 0, 1 and 255..257 unique candidates (a block is 256 rows) and ~3,000.  At the
    lengths of POLYA_TIER_EDGES, where a block is 256, 128 or 64 rows: 1, 63..65, 127..129 and 257."""
    from catch_amd import engine
    rng = np.random.default_rng(1000 + L)
    sizes = _polya_sizes(L)
    for nuniq in sizes:
        seqs = ["N" * (L + 40)] if nuniq == 0 else _sequences_with_unique_windows(rng, L, stride, nuniq)
        concat = "".join(seqs)
        targets = engine.Targets(ctx, [[s] for s in seqs])
        try:
            base = engine.Candidates(ctx, targets, L, stride)
            pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
            base.close()
            assert len(strs0) == nuniq and (nuniq < 2 or mult0.max() > 1)
            for ln, mm, gate in POLYA_COMBOS:
                length = {"4": 4, "12": 12, "L": L, "L+1": L + 1}[ln]
                keep = _np_keep(strs0, L, length, mm, gate)
                c = engine.Candidates(ctx, targets, L, stride)
                try:
                    ncand = c.ncandidates
                    c.drop_polya(length, mm, gate)
                    pos, mult, grp, _ = _snapshot(c, concat, L)
                    assert c.n == int(keep.sum()) and c.ncandidates == ncand
                    assert pos.tolist() == pos0[keep].tolist(), (nuniq, length, mm, gate)
                    assert mult.tolist() == mult0[keep].tolist(), (nuniq, length, mm, gate)
                    assert grp.tolist() == grp0[keep].tolist()
                finally:
                    c.close()
        finally:
            targets.close()


@pytest.mark.gpu
def test_drop_polya_kernel_grouped_and_errors(ctx):
    """Three groups: the second loses every candidate, the first and third share strings (one string, two groups:
    two candidates); then all candidates dropped, and the two EINVALs."""
    from catch_amd import engine
    rng = np.random.default_rng(77)
    L, stride = 64, 16
    mixed = "".join(rng.choice(list("ACGT"), size=L + stride * 299))
    mixed = mixed[:500] + "A" * 30 + mixed[530:2000] + "TTTTTTCTTTTTTTTGTTTT" + mixed[2020:]
    polya = "".join(rng.choice(list("ATC"), p=[0.9, 0.06, 0.04], size=L + stride * 280))
    polya = "".join("A" if (j % 16) < 7 else c for j, c in enumerate(polya))     # a run of 7 in every window
    genomes = [[mixed], [polya], [mixed[:L + stride * 100], mixed[stride * 7:]]]
    concat = "".join(s for g in genomes for s in g)
    targets = engine.Targets(ctx, genomes)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        for ln, mm, gate in POLYA_COMBOS:
            length = {"4": 4, "12": 12, "L": L, "L+1": L + 1}[ln]
            keep = _np_keep(strs0, L, length, mm, gate)
            c = engine.Candidates(ctx, targets, L, stride)
            try:
                c.drop_polya(length, mm, gate)
                pos, mult, grp, _ = _snapshot(c, concat, L)
                assert (pos.tolist(), mult.tolist(), grp.tolist()) == (
                    pos0[keep].tolist(), mult0[keep].tolist(), grp0[keep].tolist()), (length, mm, gate)
                if (length, mm, gate) == (12, 2, 6):
                    assert 1 not in grp.tolist() and 0 in grp.tolist() and 2 in grp.tolist()
                    assert 0 < c.n < len(strs0) - int((grp0 == 1).sum())
            finally:
                c.close()
    finally:
        targets.close()
    targets = engine.Targets(ctx, [[polya]])
    try:
        c = engine.Candidates(ctx, targets, L, stride)
        assert c.n > 256
        c.drop_polya(12, 2, 6)
        assert c.n == 0 and c.positions().size == 0 and c.ncandidates > 256
        c.drop_polya(12, 2, 6)                   # nothing in: still valid
        assert c.n == 0
        c.close()
        c = engine.Candidates(ctx, targets, L, stride)
        n = c.n
        for bad in ((0, 2, 6), (12, -1, 6), (12, 2, -1)):
            with pytest.raises(ValueError, match="drop_polya"):
                c.drop_polya(*bad)
        assert c.n == n
        c.ndf_hamming(np.arange(8, dtype=np.int32).reshape(2, 4), 1)
        with pytest.raises(ValueError, match="near-duplicate filter was already applied"):
            c.drop_polya(12, 2, 6)
        c.close()
    finally:
        targets.close()


def _run_design(argv, seed, capsys):
    from catch_amd import design
    random.seed(seed)
    np.random.seed(seed)
    capsys.readouterr()
    design.main(design.parse_args(argv))
    return capsys.readouterr().out


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"], ["--filter-with-lsh-minhash", "0.6"],
                                   ["--cluster-and-design-separately", "0.15"], "nine datasets"],
                         ids=["dup", "hamming", "minhash", "clustered", "union"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, extra):
    """--filter-polya 12 2 on the first 10 Ebola records: the kernel on the device's candidates and the host's
    strings give the same probes -- per group, clustered, and with nine one-genome datasets, which (eight or more
    small groups) go through one union instance with grouped candidates."""
    from catch_amd import engine
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    unions = []
    real_union = SetCoverFilter._filter_genomes_device_union

    def spied_union(self, *a, **k):
        unions.append(len(k.get("pre_filters", ())))
        return real_union(self, *a, **k)
    monkeypatch.setattr(SetCoverFilter, "_filter_genomes_device_union", spied_union)
    if extra == "nine datasets":
        files = [_write_records(tmp_path / ("d%d.fasta" % i), [r]) for i, r in enumerate(_ebola_records(9))]
        plain, extra = files + BASE, ["union"]
    else:
        plain = [EBOLA, "--limit-target-genomes", "10"] + BASE + extra
    argv = plain + ["--filter-polya", "12", "2"]
    outs, calls = {}, []
    real = engine.Candidates.drop_polya

    def counted(self, *a):
        calls.append(self.n)
        real(self, *a)
        calls.append(self.n)
    monkeypatch.setattr(engine.Candidates, "drop_polya", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn = tmp_path / (front + ".fasta")
        printed = _run_design(argv + ["-o", str(fn)], 5, capsys)
        outs[front] = fn.read_bytes()
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        if front == "device":
            assert calls, "the device front end did not run the kernel"
            if not extra:
                assert calls == [3063, 3017]
            if extra == ["union"]:
                assert unions == [1] and len(calls) == 2, "nine small groups are one union instance"
            n_calls = len(calls)
    assert len(calls) == n_calls, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"]
    # and the filter matters: another selection without it
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "nofilter.fasta"
    _run_design(plain + ["-o", str(fn)], 5, capsys)
    assert fn.read_bytes() != outs["device"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain10", "run1", "run2", "run3", "run4", "run5", "run6"])
def test_recorded_reference_runs(tmp_path, capsys, name):
    """bin/design.py's output, record for record (sorted), and what it printed: the probe count, or the analysis."""
    runs = {r["name"]: r for r in golden()["runs"]}
    r = runs[name]
    options = list(r["options"])
    if "<plain10>" in options:
        options[options.index("<plain10>")] = _write_records(tmp_path / "plain10.fasta",
                                                             runs["plain10"]["records_in_file_order"])
    out = tmp_path / "out.fasta"
    printed = _run_design([os.path.join(GOLDEN, r["dataset"])] + BASE + ["-o", str(out)] + options, r["seed"], capsys)
    got = _read_records(str(out))
    assert len(got) == len(r["records"])
    assert sorted(got) == r["records"]
    assert printed == r["stdout"]
    if name != "run3":
        assert int(printed.strip()) == len(got)


@pytest.mark.gpu
def test_grid_point_with_polya_equals_design(tmp_path, capsys):
    from catch_amd import design_grid
    fa = _write_records(tmp_path / "ebola10.fasta", _ebola_records(10))
    outdir = tmp_path / "grid"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "1", "2", "--grid-cover-extension", "0", "50",
                                             "-o", str(outdir), "--filter-polya", "12", "2"]))
    capsys.readouterr()
    single = tmp_path / "single.fasta"
    _run_design([fa, "-pl", "100", "-ps", "50", "-m", "2", "-e", "50", "-o", str(single), "--filter-polya", "12", "2"],
                1, capsys)
    assert (outdir / "ebola10.m2.e50.fasta").read_bytes() == single.read_bytes()
    plain = tmp_path / "plain.fasta"
    _run_design([fa, "-pl", "100", "-ps", "50", "-m", "2", "-e", "50", "-o", str(plain)], 1, capsys)
    assert plain.read_bytes() != single.read_bytes()
