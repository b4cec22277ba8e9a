"""The composition filters of the design command -- GC range, homopolymer, low complexity (--filter-gc,
--max-homopolymer, --filter-low-complexity; not in the reference).  The rule exists three times in
catch_amd/filter/composition_filter.py: _keeps (straight from the definitions: the oracle), the NumPy form of the
host path and the kernel of the device front end (catchhip_candidates_drop_composition).  Here: hand-computed cases
against _keeps, NumPy against _keeps, the kernel against NumPy, and the design command on both front ends.

Random ACGT almost never trips these rules, so the synthetic targets splice random segments of varying GC content
with homopolymers around H, di- and tri-nucleotide repeats and isolated Ns; every case asserts that each rule that
is on drops between 5 % and 95 % of the candidates, so that none can pass vacuously."""
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
EBOLA_OPTIONS = ["--filter-gc", "0.35", "0.50", "--max-homopolymer", "5", "--filter-low-complexity", "12"]


def CF(*a, **k):
    from catch_amd.filter.composition_filter import CompositionFilter
    return CompositionFilter(*a, **k)


# ------------------------------------------------------------------ inputs
def _spliced(rng, n, L, H):
    """n characters: random segments of GC content 0.15 .. 0.85, homopolymers of H - 1 .. H + 2 bases, di- and
    tri-nucleotide repeats of 6 .. 48 bases and isolated Ns, the segments about as long as a candidate."""
    out, size = [], 0
    while size < n:
        kind = rng.random()
        if kind < 0.45:
            gc = rng.choice([0.15, 0.3, 0.42, 0.5, 0.58, 0.7, 0.85])
            ln = int(rng.integers(max(2, L // 3), max(4, 2 * L)))
            seg = "".join(rng.choice(list("GCAT"), p=[gc / 2, gc / 2, (1 - gc) / 2, (1 - gc) / 2], size=ln))
        elif kind < 0.65:
            seg = str(rng.choice(list("ACGT"))) * int(rng.integers(max(1, H - 1), H + 3))
        elif kind < 0.9:
            unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(2, 4))))
            ln = int(rng.integers(6, 49))
            seg = (unit * ln)[:ln]
        else:
            seg = "N"
        out.append(seg)
        size += len(seg)
    return "".join(out)[:n]


def _targets(seed, L, stride, ncand):
    """Sequences whose windows give about ncand candidates, a good part of them more than once."""
    rng = np.random.default_rng(seed)
    s = _spliced(rng, L + stride * (ncand - 1), L, _H(L))
    if L == 300:        # a homopolymer longer than the largest window: a byte counter of the kernel reaches 254
        s = s[:5000] + "A" * 270 + s[5270:]
    half = L + stride * (ncand // 2)
    return [s, s[:half], s[stride * (ncand // 3):]]


def _windows(seqs, L, stride):
    from catch_amd.filter import candidate_probes
    return [c for q in seqs for c in candidate_probes.candidate_strings_from_sequences([q], L, stride)]


def _H(L):
    return 1 if L <= 3 else 2 if L <= 8 else 5


def _rule_sets(L):
    """(name, CompositionFilter arguments) for candidates of L bases: each rule alone, all three, none; the low-
    complexity rule at W = 64 everywhere, at W = 3 and 5 for L = 65 and 100 and at W = 256 for L = 300.  The
    thresholds are fixed per window: a window of We bases of random sequence scores about 10 (We - 2) / 128."""
    gc = dict(gc_range=("0.35", "0.6") if L > 3 else ("1/3", "2/3"))
    run = dict(max_homopolymer=_H(L))
    dust = dict(max_dust=3 if L <= 8 else 20)
    both = dict(gc, **run, **dust)
    sets = [("gc", gc), ("run", run), ("dust", dust), ("all", both), ("off", {})]
    if L in (65, 100):
        sets += [("dustW3", dict(max_dust=0, dust_window=3)), ("dustW5", dict(max_dust=8, dust_window=5))]
    if L == 300:
        sets += [("dustW256", dict(max_dust=40, dust_window=256))]
    return sets


def _dust_can_fire(L, kwargs):
    """A window needs two triplets (T >= 2) to be dropped: four bases."""
    return kwargs.get("max_dust") is not None and min(L, kwargs.get("dust_window", 64)) >= 4


def _assert_not_vacuous(name, L, kwargs, fails, n):
    """Every rule that is on drops 5 % .. 95 % of the n candidates through THAT rule -- or, where its definition
    lets it drop nothing (fewer than two triplets in a window), exactly none."""
    on = [kwargs.get("gc_range") is not None, kwargs.get("max_homopolymer") is not None,
          kwargs.get("max_dust") is not None]
    for k, rule in enumerate(("gc", "run", "dust")):
        dropped = int(np.sum(fails[k]))
        if not on[k] or (rule == "dust" and not _dust_can_fire(L, kwargs)):
            assert dropped == 0, (name, L, rule)
        else:
            assert 0.05 * n <= dropped <= 0.95 * n, (name, L, rule, dropped, n)


SHAPES = [(2, 1), (3, 1), (8, 3), (63, 20), (64, 32), (65, 17), (100, 50), (130, 50), (300, 100)]
# the kernel's workgroup by candidate length (csrc/prefilter.hip): rows copied into LDS at an odd pitch of
# 4 * ceil((L + 15) / 16) + 1 dwords and, with the low-complexity rule, 64 counter bytes per row behind them; as many
# of 256 / 128 / 64 rows as fit 64 KB, and read from global memory when 64 do not
TIER_EDGES_PLAIN = [(225, 40), (226, 40), (481, 97), (482, 97), (993, 200), (994, 200)]     # (POLYA_TIER_EDGES)
TIER_EDGES_DUST = [(161, 40), (162, 40), (417, 97), (418, 97), (929, 200), (930, 200)]
UNSTAGED = [(1000, 500)]


def _composition_workgroup(L, dust):
    """(rows per workgroup, bytes of dynamic LDS) of the kernel's launch; 256 rows and only the counters: unstaged."""
    pitch, counters = 4 * ((L + 30) // 16) + 1, 64 if dust else 0
    for rows in (256, 128, 64):
        if rows * (pitch * 4 + counters) <= 65536:
            return rows, rows * (pitch * 4 + counters)
    return 256, 256 * counters


def _score(s):
    """(10 S, T - 1) of the whole string as one window, from the definition."""
    counts = {}
    for j in range(len(s) - 2):
        t = s[j:j + 3]
        if all(c in "ACGT" for c in t):
            counts[t] = counts.get(t, 0) + 1
    return 10 * sum(c * (c - 1) // 2 for c in counts.values()), sum(counts.values()) - 1


# ------------------------------------------------------------------ host: the definition, by hand
def test_gc_rule_by_hand():
    f = CF(gc_range=("0.4", "0.6"))
    assert f._gc_bounds(10) == (4, 6)
    at = {3: "GCGAAAATTT", 4: "GCGCAAATTT", 6: "GCGCGCATTT", 7: "GCGCGCGTTT"}
    assert [f._keeps(at[g]) for g in (3, 4, 6, 7)] == [False, True, True, False]
    # exact fractions: 0.4 of 100 is 40 (a float says 40.00000000000001, whose ceiling is 41), 1/3 of 100 is 34 / 33
    assert CF(gc_range=("0.4", "1"))._gc_bounds(100) == (40, 100)
    assert CF(gc_range=("1/3", "1"))._gc_bounds(100) == (34, 100)
    assert CF(gc_range=(Fraction(0), Fraction(1, 3)))._gc_bounds(100) == (0, 33)
    f = CF(gc_range=("0.4", "1"))
    assert f._keeps("G" * 40 + "A" * 60) and not f._keeps("G" * 39 + "A" * 61)
    # L counts every character: 4 of 10 with N in it, and N is neither G nor C
    assert f._keeps("GCGCNNNNNN") and not f._keeps("GCGNNNNNNN")
    # MIN = MAX between two counts: nothing is kept
    assert CF(gc_range=("0.333", "0.333"))._gc_bounds(100) == (34, 33)
    assert f.dropped == [0, 0, 0, 0]          # (_keeps counts nothing: _filter_strs and the device do)


def test_homopolymer_rule_by_hand():
    f = CF(max_homopolymer=4)
    assert f._keeps("ACGTAAAACGT") and not f._keeps("ACGTAAAAACGT")
    assert f._keeps("CCCC") and not f._keeps("CCCCC") and not f._keeps("ACGTTTTT") and not f._keeps("GGGGGA")
    assert f._keeps("AAANAAA") and f._keeps("AAAANAAAA")          # N breaks a run
    assert f._keeps("NNNNNNNNNN") and f._keeps("ACNNNNNNGT")       # and a run of N is none
    assert f._keeps("aaaaaaaa") and f._keeps("--------")           # bytes as they are: only ACGT are bases
    assert CF(max_homopolymer=1)._keeps("ACGTACGT") and not CF(max_homopolymer=1)._keeps("ACGGT")
    assert f._keeps("")


def test_low_complexity_rule_by_hand():
    # a 64-base window of A: T = 62, S = 62 * 61 / 2 = 1891, score 10 * 1891 / 61 = 310 exactly (a tie at X = 310)
    assert _score("A" * 64) == (18910, 61)
    assert CF(max_dust=310)._keeps("A" * 64) and not CF(max_dust=309)._keeps("A" * 64)
    # (AC)n: ACA and CAC 31 times each, S = 930, score 152.46
    assert _score("AC" * 32) == (9300, 61)
    assert CF(max_dust=153)._keeps("AC" * 32) and not CF(max_dust=152)._keeps("AC" * 32)
    # (ACG)n, 66 bases: every 64-base window holds its three triplets 21, 21 and 20 times, S = 610, score 100: a tie
    assert _score(("ACG" * 22)[:64]) == _score(("ACG" * 22)[1:65]) == _score(("ACG" * 22)[2:]) == (6100, 61)
    assert CF(max_dust=100)._keeps("ACG" * 22) and not CF(max_dust=99)._keeps("ACG" * 22)
    # a 40-base repeat in random sequence: the whole string scores below the threshold, a window does not
    rng = np.random.default_rng(3)
    r = "".join(rng.choice(list("ACGT"), size=200))
    s = r[:90] + "AC" * 20 + r[130:]
    whole = _score(s)
    assert whole[0] <= 40 * whole[1]
    assert CF(max_dust=40, dust_window=200)._keeps(s) and not CF(max_dust=40)._keeps(s)
    assert CF(max_dust=40)._keeps(r)
    # 64 bases of random sequence: 62 triplets over 64 codes, about 10 * (62 / 64) / 2 = 5, far below sdust's 20
    assert all(_score(r[a:a + 64])[0] < 12 * 61 for a in range(0, 137))
    # triplets with an N are skipped: AAAANAAAA has four valid ones, all AAA -- S = 6, T - 1 = 3: a tie at X = 20
    assert _score("AAAANAAAA") == (60, 3) and _score("AAAAAAAAA") == (210, 6)
    assert CF(max_dust=20)._keeps("AAAANAAAA") and not CF(max_dust=19)._keeps("AAAANAAAA")
    assert not CF(max_dust=20)._keeps("AAAAAAAAA")
    # T < 2 drops nothing, whatever X; T = 2 can
    assert CF(max_dust=0)._keeps("AAANNNN") and CF(max_dust=0)._keeps("NAAAN") and not CF(max_dust=0)._keeps("AAAA")
    assert CF(max_dust=0)._keeps("ACGT")             # two different triplets: S = 0, and 0 > 0 is false
    # L < 3, and W = 3 (one triplet per window)
    assert CF(max_dust=0)._keeps("AA") and CF(max_dust=0)._keeps("") and CF(max_dust=0, dust_window=3)._keeps("A" * 50)
    # W > L: one window of L
    s = "ACACACACAC"
    assert _score(s) == (120, 7)
    for x in (17, 18):
        assert CF(max_dust=x, dust_window=64)._keeps(s) == CF(max_dust=x, dust_window=10)._keeps(s) == (x == 18)
    # W < L: the windows are W wide, not wider -- AAAA is in the middle, AAAAA nowhere
    assert not CF(max_dust=4, dust_window=4)._keeps("CGTAAAACGT") and CF(max_dust=4, dust_window=4)._keeps("CGTAAACGT")


def test_arguments_are_validated():
    for bad in (dict(gc_range=("0.6", "0.4")), dict(gc_range=("-0.1", "0.5")), dict(gc_range=("0.1", "1.5")),
                dict(gc_range=(0.4, 0.6)), dict(gc_range=("x", "1")), dict(gc_range="0.4"), dict(gc_range=("0.4",)),
                dict(max_homopolymer=0), dict(max_homopolymer=-3), dict(max_homopolymer=2.5),
                dict(max_dust=-1), dict(max_dust="20"), dict(dust_window=2), dict(dust_window=257),
                dict(max_dust=20, dust_window=0)):
        with pytest.raises(ValueError):
            CF(**bad)
    f = CF(gc_range=("0.25", Fraction(3, 4)), max_homopolymer=1, max_dust=0, dust_window=256)
    assert (f.gc_min, f.gc_max, f.max_homopolymer, f.max_dust, f.dust_window) == (Fraction(1, 4), Fraction(3, 4), 1, 0, 256)
    assert CF()._keeps("A" * 500) and CF().dust_window == 64


# ------------------------------------------------------------------ host: NumPy against the definition
@pytest.mark.parametrize("L,stride,ncand", [(70, 20, 2500), (100, 50, 400), (8, 3, 1500), (3, 1, 300)])
def test_numpy_rule_equals_definition(L, stride, ncand):
    """_filter_strs (NumPy, equal lengths, in chunks) against [s for s in strs if _keeps(s)], every rule set of the
    kernel test, and `dropped` against counts taken from _fails -- duplicates counted."""
    strs = _windows(_targets(50 + L, L, stride, ncand), L, stride)
    assert len(strs) > len(set(strs)) > ncand // 8
    for name, kwargs in _rule_sets(L):
        f = CF(**kwargs)
        fails = [f._fails(s) for s in strs]
        _assert_not_vacuous(name, L, kwargs, np.array(fails).T, len(strs))
        got = f._filter_strs(strs)
        assert got == [s for s, x in zip(strs, fails) if not any(x)], name          # (_keeps(s) is not any(_fails(s)))
        assert f.dropped == [sum(x[k] for x in fails) for k in range(3)] + [sum(any(x) for x in fails)], name
        assert f._filter_strs(got) == got and f._filter_strs([]) == []


def test_numpy_rule_in_chunks_and_mixed_lengths():
    from catch_amd import probe
    a = _windows(_targets(7, 40, 3, 18000), 40, 3)            # more than one chunk of 16,384
    assert len(a) > (1 << 14) + 1000
    kwargs = dict(gc_range=("0.35", "0.6"), max_homopolymer=5, max_dust=20, dust_window=16)
    f, g = CF(**kwargs), CF(**kwargs)
    got = f._filter_strs(a)
    tail = a[(1 << 14) - 50:(1 << 14) + 1000]                  # (the oracle across the chunk boundary)
    kept = set(got)
    assert [g._keeps(s) for s in tail] == [s in kept for s in tail]
    assert f.dropped[3] == len(a) - len(got) and 0.05 * len(a) < len(got) < 0.95 * len(a)
    # mixed lengths: string by string, the GC bounds per length
    mixed = a[:700] + _windows(_targets(8, 70, 20, 700), 70, 20) + ["", "A", "GC", "ACN"]
    random.Random(1).shuffle(mixed)
    f = CF(**kwargs)
    fails = [f._fails(s) for s in mixed]
    assert f._filter_strs(mixed) == [s for s, x in zip(mixed, fails) if not any(x)]
    assert f.dropped == [sum(x[k] for x in fails) for k in range(3)] + [sum(any(x) for x in fails)]
    assert all(0.05 * len(mixed) < d < 0.95 * len(mixed) for d in f.dropped)
    assert f._gc_bounds(40) == (14, 24) and f._gc_bounds(70) == (25, 42) and f._gc_bounds(1) == (1, 0)
    # Probe objects: the same rule, counted the same way
    h = CF(**kwargs)
    probes = [probe.Probe.from_str(s) for s in mixed[:300] if s]
    left = h._filter(probes)
    assert [p.seq_str for p in left] == [p.seq_str for p in probes if h._keeps(p.seq_str)]
    assert h.dropped[3] == len(probes) - len(left) > 0 and h._filter([]) == []


# ------------------------------------------------------------------ host: the option surface
def _write_records(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _ebola_records(n):
    import gzip
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


GRID_BASE = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", "out"]


def test_options_parse_and_refuse_bad_values(capsys):
    from catch_amd import design, design_grid, design_large
    assert design_large.design is design
    for parse, base in ((design.parse_args, ["x.fasta"]), (design_grid.parse_args, GRID_BASE)):
        a = parse(base)
        assert (a.filter_gc, a.max_homopolymer, a.filter_low_complexity, a.low_complexity_window) == (None, None, None, 64)
        a = parse(base + ["--filter-gc", "0.4", "2/3", "--max-homopolymer", "5", "--filter-low-complexity", "20",
                          "--low-complexity-window", "32"])
        assert (a.filter_gc, a.max_homopolymer, a.filter_low_complexity, a.low_complexity_window) == (["0.4", "2/3"], 5, 20, 32)
        assert parse(base + ["--filter-low-complexity", "0", "--low-complexity-window", "256"]).filter_low_complexity == 0
        assert parse(base + ["--filter-gc", "0", "1"]).filter_gc == ["0", "1"]
        for bad in (["--filter-gc", "0.6", "0.4"], ["--filter-gc", "-0.1", "0.5"], ["--filter-gc", "0.2", "1.01"],
                    ["--filter-gc", "0.2"], ["--filter-gc", "low", "high"], ["--max-homopolymer", "0"],
                    ["--max-homopolymer", "-1"], ["--max-homopolymer", "2.5"], ["--filter-low-complexity", "-1"],
                    ["--filter-low-complexity", "1.5"], ["--filter-low-complexity", "20", "--low-complexity-window", "2"],
                    ["--filter-low-complexity", "20", "--low-complexity-window", "257"],
                    ["--low-complexity-window", "1000"]):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert "error:" in capsys.readouterr().err, bad
    text = _help_of(design)
    for opt in ("--filter-gc", "--max-homopolymer", "--filter-low-complexity", "--low-complexity-window"):
        assert opt in text
    assert text.count("uncoverable") >= 3          # the help says what dropping costs, as for --filter-polya


def _help_of(design):
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        design.parse_args(["--help"])
    return " ".join(buf.getvalue().split())


def test_filter_order_and_strings_path(tmp_path, monkeypatch, capsys):
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    out = str(tmp_path / "o.fasta")
    every = ["--filter-gc", "0.3", "0.7", "--max-homopolymer", "6", "--filter-low-complexity", "20"]
    for first, name in ((["--filter-with-lsh-hamming", "0"], "NearDuplicateFilterWithHammingDistance"),
                        (["--filter-with-lsh-minhash", "0.6"], "NearDuplicateFilterWithMinHash"), ([], "DuplicateFilter")):
        pd = _design_without_designing(monkeypatch, [
            fa, "-o", out, "--add-adapters", "--filter-polya", "12", "2", "--filter-from-fasta", fa] + every + first)
        assert [type(f).__name__ for f in pd.filters] == [
            "FastaFilter", "PolyAFilter", "CompositionFilter", name, "SetCoverFilter", "AdapterFilter"]
        assert pd._strings_path_ok(pd.filters) and pd._strings_prefix(pd.filters) == 5
        cf = pd.filters[2]
        assert (cf.gc_min, cf.gc_max, cf.max_homopolymer, cf.max_dust, cf.dust_window) == (
            Fraction(3, 10), Fraction(7, 10), 6, 20, 64)
    # any one of the options adds ONE filter; without them the list is what it was
    for opts in (every[:3], every[3:5], every[5:], every[5:] + ["--low-complexity-window", "16"]):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out] + opts)
        assert [type(f).__name__ for f in pd.filters] == ["CompositionFilter", "DuplicateFilter", "SetCoverFilter"]
    assert pd.filters[0].dust_window == 16 and pd.filters[0].gc_min is None and pd.filters[0].max_homopolymer is None
    for opts in ([], ["--low-complexity-window", "16"]):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out] + opts)
        assert [type(f).__name__ for f in pd.filters] == ["DuplicateFilter", "SetCoverFilter"]
    capsys.readouterr()


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
    cf, paf, ff, dup = CF(max_homopolymer=5), PolyAFilter(12, 2), FastaFilter(str(tmp_path / "none.fasta")), DuplicateFilter()
    ndf = NearDuplicateFilterWithHammingDistance(2, 100)
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    genomes = [[genome.Genome.from_one_seq("ACGT" * 100)]]
    pd = PD(genomes, [cf, dup, scf], probe_length=100, probe_stride=50)
    for filters in ([cf, dup, scf], [paf, cf, ndf, scf], [ff, paf, cf, dup, scf], [cf, cf, ff, dup, scf, cf]):
        assert PD._strings_path_ok(filters), filters
    for filters in ([cf, dup], [cf, scf], [dup, cf, scf], [cf]):
        assert not PD._strings_path_ok(filters), filters
    plain = pd._device_front_end_mode(genomes, dup, scf)
    assert plain == "per group"
    assert pd._device_front_end_mode(genomes, dup, scf, [cf]) == plain
    assert pd._device_front_end_mode(genomes, dup, scf, [paf, cf]) == plain
    assert pd._device_front_end_mode(genomes, ndf, scf, [cf, cf]) == pd._device_front_end_mode(genomes, ndf, scf)
    many = [[genome.Genome.from_one_seq("ACGT" * 100)] for _ in range(9)]
    assert pd._device_front_end_mode(many, dup, scf, [cf]) == pd._device_front_end_mode(many, dup, scf) == "union"
    assert pd._device_front_end_mode(genomes, dup, scf, [ff, cf]) is None
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    assert pd._device_front_end_mode(genomes, dup, scf, [cf]) is None


def test_symbol_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib, engine
    name = "catchhip_candidates_drop_composition"
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    at = re.search(r"\b%s\s*\(" % name, hdr)
    assert at and "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 9
    assert hasattr(_lib.lib(), name)
    assert hasattr(engine.Candidates, "drop_composition")


def test_tier_edges_sit_on_the_workgroup_sizes_claimed():
    """No GPU: the lengths added to the kernel test are the last of one workgroup size and the first of the next, with
    and without the 64 counter bytes per row -- and the plain edges are the poly(A) kernel's."""
    assert [_composition_workgroup(L, False) for L, _ in TIER_EDGES_PLAIN] == [
        (256, 62464), (128, 33280), (128, 64000), (64, 33024), (64, 64768), (256, 0)]
    assert [_composition_workgroup(L, True) for L, _ in TIER_EDGES_DUST] == [
        (256, 62464), (128, 33280), (128, 64000), (64, 33024), (64, 64768), (256, 16384)]     # (pitch + 64 B: 244, 260, ..)
    assert all(_composition_workgroup(L, d)[0] == 256 for L, _ in SHAPES[:-1] for d in (False, True))
    assert _composition_workgroup(300, False)[0] == _composition_workgroup(300, True)[0] == 128
    assert _composition_workgroup(1000, False) == (256, 0) and _composition_workgroup(1000, True) == (256, 16384)
    assert all(stride < L for L, stride in SHAPES + TIER_EDGES_PLAIN + TIER_EDGES_DUST + UNSTAGED)


# ------------------------------------------------------------------ GPU: the kernel against the NumPy rule
def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


def _expect(f, strs, mult, L):
    """(keep mask, [GC, homopolymer, low complexity, any] with multiplicity) by the NumPy rule."""
    if not strs:
        return np.zeros(0, dtype=bool), [0, 0, 0, 0]
    fails = f._fail_masks_equal_length(strs, L)
    drop = fails[0] | fails[1] | fails[2]
    return ~drop, [int(mult[x].sum()) for x in fails] + [int(mult[drop].sum())]


@pytest.mark.gpu
@pytest.mark.parametrize("L,stride", SHAPES + TIER_EDGES_PLAIN + TIER_EDGES_DUST + UNSTAGED)
def test_drop_composition_kernel_equals_numpy(ctx, L, stride):
    """catchhip_candidates_drop_composition against the NumPy rule, every rule set of _rule_sets: the surviving
    positions, multiplicities and groups are the unfiltered list's, masked, and the four counts are the failing
    candidates' multiplicities -- on a few hundred unique candidates (several workgroups, the last one partial)."""
    from catch_amd import engine
    seqs = _targets(1000 + L, L, stride, 700 if L < 400 else 330)
    concat = "".join(seqs)
    targets = engine.Targets(ctx, [[s] for s in seqs])
    try:
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        n = len(strs0)
        assert mult0.max() > 1 and n % 64 != 0 and (n > 256 or L <= 3)
        if L == 300:
            assert any("A" * 256 in s for s in strs0)
        for name, kwargs in _rule_sets(L):
            f = CF(**kwargs)
            keep, want = _expect(f, strs0, mult0, L)
            _assert_not_vacuous(name, L, kwargs, f._fail_masks_equal_length(strs0, L), n)
            c = engine.Candidates(ctx, targets, L, stride)
            try:
                ncand = c.ncandidates
                f._apply_to_candidates(c)
                print(name, L, n, "kept", c.n, "dropped", f.dropped, "want", want)
                assert f.dropped == want, name
                pos, mult, grp, _ = _snapshot(c, concat, L)
                assert c.n == int(keep.sum()) and c.ncandidates == ncand
                assert pos.tolist() == pos0[keep].tolist(), name
                assert mult.tolist() == mult0[keep].tolist(), name
                assert grp.tolist() == grp0[keep].tolist(), name
                if name == "all":        # a second call on the filtered list: valid, and nothing more goes
                    assert c.drop_composition(*_library_arguments(f, L)) == [0, 0, 0, 0] and c.n == int(keep.sum())
                    assert c.positions().tolist() == pos.tolist()
            finally:
                c.close()
    finally:
        targets.close()


def _library_arguments(f, L):
    lo, hi = f._gc_bounds(L) if f.gc_min is not None else (-1, -1)
    return (lo, hi, -1 if f.max_homopolymer is None else f.max_homopolymer,
            -1 if f.max_dust is None else f.max_dust, f.dust_window)


@pytest.mark.gpu
def test_drop_composition_kernel_grouped_and_errors(ctx):
    """Three groups, the first and third sharing strings (one string, two groups: two candidates), the second all
    low complexity; then an empty list, the bad arguments and the call after a near-duplicate filter."""
    from catch_amd import engine
    L, stride = 64, 16
    mixed = _targets(5, L, stride, 300)[0]
    low = ("AC" * 40 + "AAAAAAAAAT" * 6 + "ACG" * 30) * 12
    genomes = [[mixed], [low], [mixed[:L + stride * 100], mixed[stride * 7:]]]
    concat = "".join(s for g in genomes for s in g)
    kwargs = dict(gc_range=("0.35", "0.6"), max_homopolymer=5, max_dust=20)
    f = CF(**kwargs)
    targets = engine.Targets(ctx, genomes)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        keep, want = _expect(f, strs0, mult0, L)
        _assert_not_vacuous("grouped", L, kwargs, f._fail_masks_equal_length(strs0, L), len(strs0))
        c = engine.Candidates(ctx, targets, L, stride)
        f._apply_to_candidates(c)
        pos, mult, grp, _ = _snapshot(c, concat, L)
        c.close()
        assert f.dropped == want
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (
            pos0[keep].tolist(), mult0[keep].tolist(), grp0[keep].tolist())
        assert 1 not in grp.tolist() and 0 in grp.tolist() and 2 in grp.tolist()
    finally:
        targets.close()
    targets = engine.Targets(ctx, [[low]])
    try:
        c = engine.Candidates(ctx, targets, L, stride)
        n, total = c.n, c.ncandidates
        assert total > n > 0
        assert c.drop_composition() == [0, 0, 0, 0] and c.n == n                       # every rule off
        assert c.drop_composition(0, L, -1, -1, 64) == [0, 0, 0, 0] and c.n == n        # GC "off" by its bounds
        for bad in ((-2, -1, -1, -1, 64), (-1, -2, -1, -1, 64), (-1, -1, 0, -1, 64), (-1, -1, -2, -1, 64),
                    (-1, -1, -1, -2, 64), (-1, -1, -1, 20, 2), (-1, -1, -1, 20, 257)):
            with pytest.raises(ValueError, match="drop_composition"):
                c.drop_composition(*bad)
        assert c.n == n
        assert c.drop_composition(-1, -1, -1, -1, 0) == [0, 0, 0, 0]                    # (the window is not read: rule off)
        assert c.drop_composition(-1, -1, -1, 20, 64) == [0, 0, total, total]           # all low complexity
        assert c.n == 0 and c.positions().size == 0 and c.ncandidates == total
        assert c.drop_composition(10, 20, 3, 20, 64) == [0, 0, 0, 0] and c.n == 0       # an empty list is valid
        c.close()
        c = engine.Candidates(ctx, targets, L, stride)
        c.ndf_hamming(np.arange(8, dtype=np.int32).reshape(2, 4), 1)
        with pytest.raises(ValueError, match="candidates_drop_composition: a near-duplicate filter was already applied"):
            c.drop_composition(10, 20, 3, 20, 64)
        c.close()
    finally:
        targets.close()


# ------------------------------------------------------------------ GPU: the design command
def _run_design(argv, seed, capsys):
    from catch_amd import design
    random.seed(seed)
    np.random.seed(seed)
    capsys.readouterr()
    pb = design.main(design.parse_args(argv))
    return pb, capsys.readouterr().out


def _read_sequences(path):
    with open(path) as f:
        return [line.strip() for line in f if not line.startswith(">")]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"], ["--filter-with-lsh-minhash", "0.6"]],
                         ids=["dup", "hamming", "minhash"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, extra):
    """The three rules on the first 5 Ebola genomes: the kernel on the device's candidates and the host's strings give
    the same probes and the same counts; every probe written passes the rules; the design differs from the one
    without them.  (--filter-low-complexity 12, not sdust's 20: at 20 the rule drops nothing of these genomes.)"""
    from catch_amd import engine
    from catch_amd.filter.composition_filter import CompositionFilter
    plain = [EBOLA, "--limit-target-genomes", "5"] + BASE + extra
    argv = plain + EBOLA_OPTIONS
    outs, dropped, calls = {}, {}, []
    real = engine.Candidates.drop_composition

    def counted(self, *a):
        calls.append(self.n)
        got = real(self, *a)
        calls.append(self.n)
        return got
    monkeypatch.setattr(engine.Candidates, "drop_composition", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn = tmp_path / (front + ".fasta")
        pb, printed = _run_design(argv + ["-o", str(fn)], 5, capsys)
        outs[front] = fn.read_bytes()
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        cf = [f for f in pb.filters if type(f) is CompositionFilter]
        assert len(cf) == 1
        dropped[front] = list(cf[0].dropped)
        if front == "device":
            assert len(calls) == 2 and calls[0] > calls[1] > 0, "the device front end did not run the kernel"
    assert len(calls) == 2, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"]
    assert dropped["device"] == dropped["host"]
    print("dropped", dropped["device"], "unique candidates", calls)
    ncand = 1888                                    # windows of the 5 genomes
    assert all(d >= 1 for d in dropped["device"][:3]) and ncand - dropped["device"][3] >= ncand / 2
    f = CF(gc_range=("0.35", "0.50"), max_homopolymer=5, max_dust=12)
    probes = _read_sequences(tmp_path / "device.fasta")
    assert probes and all(f._keeps(s) for s in probes)
    # and the filter matters: another selection without it
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "nofilter.fasta"
    _run_design(plain + ["-o", str(fn)], 5, capsys)
    assert fn.read_bytes() != outs["device"]
    assert not all(f._keeps(s) for s in _read_sequences(fn))


@pytest.mark.gpu
def test_grid_point_with_composition_equals_design(tmp_path, capsys):
    from catch_amd import design_grid
    fa = _write_records(tmp_path / "ebola5.fasta", _ebola_records(5))
    outdir = tmp_path / "grid"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "2", "--grid-cover-extension", "50",
                                             "-o", str(outdir)] + EBOLA_OPTIONS))
    capsys.readouterr()
    single = tmp_path / "single.fasta"
    _run_design([fa] + BASE + ["-o", str(single)] + EBOLA_OPTIONS, 1, capsys)
    assert (outdir / "ebola5.m2.e50.fasta").read_bytes() == single.read_bytes()
    plain = tmp_path / "plain.fasta"
    _run_design([fa] + BASE + ["-o", str(plain)], 1, capsys)
    assert plain.read_bytes() != single.read_bytes()
