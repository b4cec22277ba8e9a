"""The melting temperature filter of the design command (--filter-tm, --tm-sodium, --tm-oligo, --tm-formamide,
--write-tm-histogram; not in the reference).  The rule exists three times in catch_amd/filter/tm_filter.py: _tm_c and
_keeps (straight from the definition: the oracle), the NumPy form of the host path and the kernel of the device front
end (catchhip_candidates_drop_tm).  Here: the issue's hand-computed values against _tm_c, NumPy against _tm_c, the
kernel against NumPy, and the design command on both front ends.

The synthetic targets splice random segments of GC content 0.15 .. 0.85 with repeats, isolated Ns, stretches of
(AN)n and (NG)n longer than a window and, for the long candidates, GC-rich stretches that take |E| and |H| past 65,535.
The sliding windows make no candidate with two adjacent Ns (candidate_probes.py), so an all-N window cannot reach
either front end: a window of (AN)n is what takes the H >= 0 branch there -- no dinucleotide of two bases, like all-N.
The all-N strings themselves go through _tm_c and the NumPy path directly.
The filtering cases take their bounds from the 30th and 70th percentile of the input's own _tm_c and assert that
"below" and "above" each drop 5 % .. 95 % of the candidates, so that none can pass vacuously; at L <= 3 a candidate has
too few different values for that, and the counts are asserted against the definition instead."""
import logging
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
NAME = "catchhip_candidates_drop_tm"


def TF(*a, **k):
    from catch_amd.filter.tm_filter import TmFilter
    return TmFilter(*a, **k)


def _h_e(s):
    from catch_amd.filter.tm_filter import TmFilter
    return TmFilter._h_e(s)


# ------------------------------------------------------------------ inputs
def _spliced(rng, n, L, stride):
    """n characters: random segments of GC content 0.15 .. 0.85, di- and tri-nucleotide repeats, isolated Ns and now
    and then a stretch of (AN)n or (NG)n that holds a whole window, the segments about as long as a candidate."""
    out, size = [], 0
    while size < n:
        kind = rng.random()
        if kind < 0.6:
            gc = rng.choice([0.15, 0.3, 0.42, 0.5, 0.58, 0.7, 0.85])
            ln = int(rng.integers(max(2, L // 3), max(4, 2 * L)))
            seg = "".join(rng.choice(list("GCAT"), p=[gc / 2, gc / 2, (1 - gc) / 2, (1 - gc) / 2], size=ln))
        elif kind < 0.85:
            unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(2, 4))))
            ln = int(rng.integers(6, 49))
            seg = (unit * ln)[:ln]
        elif kind < 0.98:
            seg = "N"
        else:
            seg = (str(rng.choice(["AN", "NG"])) * (L + stride))[:L + stride]
        out.append(seg)
        size += len(seg)
    return "".join(out)[:n]


def _targets(seed, L, stride, ncand):
    """Sequences whose windows give about ncand candidates, a good part of them more than once; one window of (AN)n, one
    that begins and one that ends with an N for certain, and for L >= 300 a stretch of (GC)n longer than a window."""
    rng = np.random.default_rng(seed)
    s = _spliced(rng, L + stride * (ncand - 1), L, stride)
    a = stride * (ncand // 5)
    s = s[:a] + ("AN" * (L + stride))[:L + stride] + s[a + L + stride:]
    while "NN" in s:                    # (two adjacent Ns end a window: candidate_probes.py leaves such windows out)
        s = s.replace("NN", "NA")
    for at in (stride * (ncand // 7), stride * (ncand // 9) + L - 1):        # a window that begins, one that ends with N
        s = s[:at - 1] + "ANA" + s[at + 2:]
    if L >= 300:
        a = stride * (ncand // 2)
        s = s[:a] + "GC" * ((L + stride + 1) // 2) + s[a + 2 * ((L + stride + 1) // 2):]
    half = L + stride * (ncand // 2 + 3)
    return [s, s[:half], s[stride * (ncand // 3):]]


def _windows(seqs, L, stride):
    from catch_amd.filter import candidate_probes
    return [c for q in seqs for c in candidate_probes.candidate_strings_from_sequences([q], L, stride)]


def _percentile_range(tm, lo=30, hi=70):
    """(MIN, MAX) as exact Fractions of degrees: the lo-th and hi-th percentile of the tm_c values (nearest rank)."""
    v = sorted(tm)
    return Fraction(v[len(v) * lo // 100], 100), Fraction(v[len(v) * hi // 100], 100)


def _definition(f, strs):
    """(keep list, [below, above, any], histogram) straight from _tm_c, string by string."""
    tm = [f._tm_c(s) for s in strs]
    side = [f._side(t) for t in tm]
    hist = [0] * 128
    for t in tm:
        if t is not None:
            hist[min(max(t // 100, 0), 127)] += 1
    return [x == 0 for x in side], [side.count(-1), side.count(1), side.count(-1) + side.count(1)], hist


SHAPES = [(2, 1), (3, 1), (8, 3), (63, 20), (64, 32), (65, 17), (100, 50), (130, 50), (300, 100)]
# the kernel's workgroup by candidate length (csrc/thermo.hip): rows copied into LDS as the poly(A) kernel copies them,
# at an odd pitch of 4 * ceil((L + 15) / 16) + 1 dwords, and behind them, once per workgroup, the 16-dword table and 130
# 64-bit counters (1,104 bytes); as many of 256 / 128 / 64 rows as fit 64 KB, read from global memory when 64 do not.
# The first two edges are the poly(A) kernel's; the third comes 16 bases sooner (64 rows of 993 bases leave 768 bytes).
TIER_EDGES = [(225, 40), (226, 40), (481, 97), (482, 97), (977, 200), (978, 200)]
UNSTAGED = [(1000, 500)]
TM_EXTRA = 16 * 4 + 130 * 8


def _tm_workgroup(L):
    """(rows per workgroup, bytes of dynamic LDS) of the kernel's launch; 256 rows and only the extras: unstaged."""
    pitch = 4 * ((L + 30) // 16) + 1
    for rows in (256, 128, 64):
        if rows * pitch * 4 + TM_EXTRA <= 65536:
            return rows, rows * pitch * 4 + TM_EXTRA
    return 256, TM_EXTRA


# ------------------------------------------------------------------ host: the definition, by hand
def test_q_of_length():
    f = TF()
    assert [f._q(L) for L in (2, 4, 20, 100)] == [-37261, -39466, -57105, -145299]
    assert TF(sodium_mm="825")._q(100) == -43167
    assert TF(sodium_mm=Fraction(825), oligo_nm=Fraction(50))._q(100) == -43167
    # L - 1 counts every character; Q above -8200 is refused, at the length where it happens
    salty = TF(sodium_mm="2000", oligo_nm="50")
    assert salty._q(2) < -8200
    with pytest.raises(ValueError, match="-8200"):
        salty._q(200)
    with pytest.raises(ValueError, match="-8200"):
        TF(oligo_nm="1000000000")._q(2)


def test_values_by_hand():
    f, salty = TF(), TF(sodium_mm="825")
    assert f._h_e("ACGT") == (-228, -638) and 100 * -638 + f._q(4) == -103266 and f._tm_c("ACGT") == -5237
    assert f._h_e("A" * 100) == (-7775, -21896) and f._tm_c("A" * 100) == 5984 and salty._tm_c("A" * 100) == 7507
    assert f._h_e("GC" * 50) == (-10092, -25584) and f._tm_c("GC" * 50) == 10011 and salty._tm_c("GC" * 50) == 11477
    assert f._tm_c("ACGT" * 25) == 7533
    s = "GATTACA" * 3
    assert f._h_e(s) == (-1554, -4343) and 100 * -4343 + f._q(21) == -492507 and f._tm_c(s) == 4237
    assert f._h_e("AN" * 10)[0] == 46 and f._tm_c("AN" * 10) == -27315          # H >= 0: T = 0
    # formamide: 0.62 degrees per percent, rounded half up to hundredths
    assert TF(formamide_pct="20")._tm_c(s) == 4237 - 1240 and TF(formamide_pct="20").offset_c == 27315 + 1240
    assert TF(formamide_pct="1/124").offset_c == 27316 and TF(formamide_pct="1/125").offset_c == 27315
    assert f.dropped == [0, 0, 0] and f.histogram == [0] * 128         # (_tm_c counts nothing)


def test_table_symmetries_and_n():
    from catch_amd.filter.tm_filter import NN
    comp = str.maketrans("ACGT", "TGCA")
    assert len(NN) == 16
    for d, v in NN.items():             # a dinucleotide and its reverse complement are the same stack
        assert NN[d.translate(comp)[::-1]] == v, d
    assert NN["AA"] == NN["TT"] and NN["CA"] == NN["TG"] and NN["GT"] == NN["AC"] and NN["CT"] == NN["AG"]
    assert NN["GA"] == NN["TC"] and NN["GG"] == NN["CC"] and NN["AT"] != NN["TA"] and NN["CG"] != NN["GC"]
    f = TF()
    # L = 2: one stack and two ends
    assert f._h_e("CG") == (-106 + 2, -272 - 56) and f._h_e("AT") == (-72 + 46, -204 + 82)
    assert f._h_e("GA") == (-82 + 24, -222 + 13) and f._h_e("NN") == (46, 82) and f._h_e("GN") == (24, 13)
    assert f._tm_c("CG") == 10 ** 7 * 104 // (32800 + 37261) - 27315
    assert f._tm_c("NN") == f._tm_c("GN") == f._tm_c("Nn") == -27315
    # an inner N removes the two stacks it is in; a terminal N removes one and ends like A or T
    assert f._h_e("ACNGT") == (-84 - 84 + 46, -224 - 224 + 82)
    assert f._h_e("NCGT") == (-106 - 84 + 46, -272 - 224 + 82) and f._h_e("GCGN") == (-98 - 106 + 24, -244 - 272 + 13)
    assert f._h_e("acgt") == (46, 82)              # bytes as they are: only ACGT are bases
    # L < 2: no value, nothing dropped, nothing counted
    g = TF(tm_range=("50", "60"))
    assert g._tm_c("") is None and g._tm_c("A") is None and g._keeps("") and g._keeps("G")
    assert g._filter_strs(["A", "C", "A"]) == ["A", "C", "A"] and g._filter_strs([""]) == [""]
    assert g._filter_strs(["", "A", "AC"]) == ["", "A"]
    assert g.dropped == [1, 0, 1] and sum(g.histogram) == 1 and g.histogram[0] == 1


def test_bounds_from_text():
    f = TF(tm_range=("76.65", "76.65"))
    assert (f.lo_c, f.hi_c) == (7665, 7665)
    f = TF(tm_range=("229/3", "230/3"))
    assert (f.lo_c, f.hi_c) == (7634, 7666)
    f = TF(tm_range=(Fraction(-1, 3), "0.005"))
    assert (f.lo_c, f.hi_c) == (-33, 0)
    assert (TF(tm_range=("-300", "300")).lo_c, TF(tm_range=("-300", "300")).hi_c) == (-30000, 30000)
    for bad in (dict(tm_range=(76.65, "80")), dict(tm_range=("70", 80.0)), dict(tm_range=("80", "70")),
                dict(tm_range=("-301", "70")), dict(tm_range=("70", "300.01")), dict(tm_range=("x", "70")),
                dict(tm_range="70"), dict(tm_range=("70",)), dict(sodium_mm=50.0), dict(oligo_nm=0.5),
                dict(formamide_pct=1.5), dict(sodium_mm="0"), dict(sodium_mm="-1"), dict(oligo_nm="0"),
                dict(formamide_pct="-1"), dict(formamide_pct="100.5"), dict(sodium_mm="salt")):
        with pytest.raises(ValueError):
            TF(**bad)
    f = TF()
    assert (f.lo_c, f.hi_c, f.sodium_mm, f.oligo_nm, f.formamide_pct) == (None, None, 50, 50, 0)
    assert f._keeps("A" * 100) and f._keeps("NN")             # measuring only keeps everything
    k = TF(tm_range=("59.84", "75.33"))
    assert k._keeps("A" * 100) and k._keeps("ACGT" * 25) and not k._keeps("GC" * 50) and not k._keeps("ACGT")
    assert not TF(tm_range=("59.85", "75.33"))._keeps("A" * 100) and not TF(tm_range=("59.84", "75.32"))._keeps("ACGT" * 25)


# ------------------------------------------------------------------ host: NumPy against the definition
def _settings(strs):
    """(name, TmFilter arguments): the percentile range, measuring only, other conditions with a range of their own."""
    other = dict(sodium_mm="825", formamide_pct="20")
    plain, salty = TF(), TF(**other)
    lo, hi = _percentile_range([plain._tm_c(s) for s in strs])
    lo2, hi2 = _percentile_range([salty._tm_c(s) for s in strs])
    return [("range", dict(tm_range=(lo, hi))), ("measure", {}), ("na825f20", dict(tm_range=(lo2, hi2), **other))]


def _assert_not_vacuous(name, L, kwargs, three, n):
    if "tm_range" not in kwargs:
        assert three == [0, 0, 0], name
    elif L > 3:                 # (L <= 3: the callers compare with the definition's exact counts)
        assert 0.05 * n <= three[0] <= 0.95 * n and 0.05 * n <= three[1] <= 0.95 * n, (name, L, three, n)


@pytest.mark.parametrize("L,stride,ncand", [(100, 50, 400), (70, 20, 2500), (8, 3, 1500), (2, 1, 300)])
def test_numpy_rule_equals_definition(L, stride, ncand):
    """_filter_strs (NumPy, equal lengths) against the definition: what is kept, `dropped` and `histogram`."""
    strs = _windows(_targets(50 + L, L, stride, ncand), L, stride)
    assert len(strs) > len(set(strs)) > min(ncand // 8, 20)
    flat = [s for s in strs if _h_e(s)[0] >= 0]                 # no dinucleotide of two bases: T = 0
    assert ("AN" * L)[:L] in flat and any(s[0] == "N" for s in strs) and any(s[-1] == "N" for s in strs)
    for name, kwargs in _settings(strs):
        f = TF(**kwargs)
        keep, three, hist = _definition(f, strs)
        _assert_not_vacuous(name, L, kwargs, three, len(strs))
        got = f._filter_strs(strs)
        assert got == [s for s, k in zip(strs, keep) if k], name
        assert f.dropped == three and f.histogram == hist and sum(hist) == len(strs), name
        assert hist[0] >= len(flat) > 0
        assert f._filter_strs(got) == got and f._filter_strs([]) == []
        assert f.dropped[2] == three[2] and sum(f.histogram) == len(strs) + len(got)      # (a second pass counts again)


def test_numpy_rule_in_chunks_and_mixed_lengths():
    from catch_amd import probe
    a = _windows(_targets(7, 40, 3, 18000), 40, 3)            # more than one chunk of 16,384
    assert len(a) > (1 << 14) + 1000
    g0 = TF()
    lo, hi = _percentile_range([g0._tm_c(s) for s in a[:3000]])
    f, g = TF(tm_range=(lo, hi)), TF(tm_range=(lo, hi))
    got = f._filter_strs(a)
    tail = a[(1 << 14) - 50:(1 << 14) + 1000]                  # (the oracle across the chunk boundary)
    kept = set(got)
    assert [g._keeps(s) for s in tail] == [s in kept for s in tail]
    assert f.dropped[2] == len(a) - len(got) and 0.05 * len(a) < len(got) < 0.95 * len(a)
    assert sum(f.histogram) == len(a)
    # mixed lengths: string by string, Q per length
    mixed = a[:700] + _windows(_targets(8, 70, 20, 700), 70, 20) + ["", "A", "GC", "ACN", "NN"]
    random.Random(1).shuffle(mixed)
    lo, hi = _percentile_range([t for t in (g0._tm_c(s) for s in mixed) if t is not None])
    f = TF(tm_range=(lo, hi))
    keep, three, hist = _definition(f, mixed)
    assert f._filter_strs(mixed) == [s for s, k in zip(mixed, keep) if k]
    assert f.dropped == three and f.histogram == hist and sum(hist) == len(mixed) - 2
    assert all(0.05 * len(mixed) < d < 0.95 * len(mixed) for d in three)
    assert set(f._q_of) == {2, 3, 40, 70} and f._q(40) != f._q(70)
    # Probe objects: the same rule, counted the same way
    h = TF(tm_range=(lo, hi))
    probes = [probe.Probe.from_str(s) for s in mixed[:300] if s]
    left = h._filter(probes)
    assert [p.seq_str for p in left] == [p.seq_str for p in probes if h._keeps(p.seq_str)]
    assert h.dropped[2] == len(probes) - len(left) > 0 and h._filter([]) == []
    assert sum(h.histogram) == sum(1 for p in probes if len(p.seq_str) >= 2)


def test_write_histogram(tmp_path):
    f = TF()
    fn = tmp_path / "h.tsv"
    f.write_histogram(str(fn))
    assert fn.read_text() == "tm_c\tcandidates\n"             # nothing counted: the header alone
    f._filter_strs(["A" * 100, "A" * 100, "ACGT" * 25])          # 59.84 twice, 75.33 once
    f.write_histogram(str(fn))
    rows = fn.read_text().splitlines()
    assert rows[0] == "tm_c\tcandidates" and rows[1] == "59\t2" and rows[-1] == "75\t1"
    assert rows[2:-1] == ["%d\t0" % b for b in range(60, 75)]           # empty bins between them are written
    g = TF(tm_range=("-300", "300"))
    assert g._filter_strs(["N" * 100, "NN" * 50, "A" * 100]) == ["N" * 100, "NN" * 50, "A" * 100] and g.histogram[0] == 2
    assert g._tm_c_equal_length(["N" * 100, "AN" * 50, "NG" * 50], 100).tolist() == [-27315] * 3
    g = TF(sodium_mm="1000", oligo_nm="1000000")                # (G)n at 1 M sodium and 1 mM oligo: 128.4 degrees
    g._filter_strs(["NN" * 500, "G" * 1000])                   # below 0 and above 127: the end bins
    assert g.histogram[0] == 1 and g.histogram[127] == 1 and sum(g.histogram) == 2 and g._tm_c("G" * 1000) > 12800


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


def _help_of(design):
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        design.parse_args(["--help"])
    return " ".join(buf.getvalue().split())


GRID_BASE = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", "out"]


def test_options_parse_and_refuse_bad_values(capsys):
    from catch_amd import design, design_grid, design_large
    assert design_large.design is design
    large = lambda argv: design.parse_args(argv, args_type="large")          # noqa: E731
    for parse, base in ((design.parse_args, ["x.fasta"]), (large, ["x.fasta"]), (design_grid.parse_args, GRID_BASE)):
        a = parse(base)
        assert (a.filter_tm, a.tm_sodium, a.tm_oligo, a.tm_formamide, a.write_tm_histogram) == (None,) * 5
        a = parse(base + ["--filter-tm", "74", "229/3", "--tm-sodium", "825", "--tm-oligo", "2.5", "--tm-formamide",
                          "20", "--write-tm-histogram", "h.tsv"])
        assert (a.filter_tm, a.tm_sodium, a.tm_oligo, a.tm_formamide, a.write_tm_histogram) == (
            ["74", "229/3"], "825", "2.5", "20", "h.tsv")
        assert parse(base + ["--write-tm-histogram", "h.tsv", "--tm-sodium", "100"]).filter_tm is None
        assert parse(base + ["--filter-tm", "-300", "300"]).filter_tm == ["-300", "300"]
        for bad in (["--filter-tm", "80", "70"], ["--filter-tm", "70"], ["--filter-tm", "low", "high"],
                    ["--filter-tm", "70", "301"], ["--filter-tm", "-300.5", "70"],
                    ["--filter-tm", "70", "80", "--tm-sodium", "0"], ["--filter-tm", "70", "80", "--tm-sodium", "-5"],
                    ["--filter-tm", "70", "80", "--tm-sodium", "salt"], ["--filter-tm", "70", "80", "--tm-oligo", "0"],
                    ["--write-tm-histogram", "h.tsv", "--tm-oligo", "-1"],
                    ["--filter-tm", "70", "80", "--tm-formamide", "-1"],
                    ["--write-tm-histogram", "h.tsv", "--tm-formamide", "100.5"],
                    ["--tm-sodium", "50"], ["--tm-oligo", "50"], ["--tm-formamide", "0"],
                    # Q(100) above -8200: 5 M of sodium, or 2 M with a micromolar of oligo
                    ["--filter-tm", "70", "80", "--tm-sodium", "5000"],
                    ["--write-tm-histogram", "h.tsv", "--tm-sodium", "2000", "--tm-oligo", "1000"]):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert "error:" in capsys.readouterr().err, bad
        # the same 2 M of sodium is fine for a probe short enough
        assert parse(base + ["--write-tm-histogram", "h.tsv", "--tm-sodium", "2000", "--tm-oligo", "1000", "-pl", "20",
                             "-ps", "10"]).tm_sodium == "2000"
    text = _help_of(design)
    for opt in ("--filter-tm", "--tm-sodium", "--tm-oligo", "--tm-formamide", "--write-tm-histogram"):
        assert opt in text
    assert "uncoverable" in text.split("--filter-tm MIN MAX")[-1].split("--tm-sodium")[0]
    assert "survive the filters before this one" in text


def test_filter_order_and_strings_path(tmp_path, monkeypatch, capsys):
    from catch_amd.filter.probe_designer import ProbeDesigner
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    out = str(tmp_path / "o.fasta")
    every = ["--filter-polya", "12", "2", "--filter-from-fasta", fa, "--filter-gc", "0.3", "0.7", "--max-hairpin-stem",
             "9", "--filter-tm", "70", "80", "--tm-formamide", "10"]
    for first, name in ((["--filter-with-lsh-hamming", "0"], "NearDuplicateFilterWithHammingDistance"),
                        (["--filter-with-lsh-minhash", "0.6"], "NearDuplicateFilterWithMinHash"), ([], "DuplicateFilter")):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--add-adapters"] + every + first)
        assert [type(f).__name__ for f in pd.filters] == [
            "FastaFilter", "PolyAFilter", "CompositionFilter", "StructureFilter", "TmFilter", name, "SetCoverFilter",
            "AdapterFilter"]
        assert pd._strings_path_ok(pd.filters) and pd._strings_prefix(pd.filters) == 7
        tf = pd.filters[4]
        assert (tf.lo_c, tf.hi_c, tf.offset_c, tf.sodium_mm) == (7000, 8000, 27315 + 620, 50)
    # --write-tm-histogram alone adds ONE measuring filter; without the options the list is what it was
    pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--write-tm-histogram", str(tmp_path / "h.tsv")])
    assert [type(f).__name__ for f in pd.filters] == ["TmFilter", "DuplicateFilter", "SetCoverFilter"]
    assert pd.filters[0].lo_c is None and (tmp_path / "h.tsv").read_text() == "tm_c\tcandidates\n"
    pd = _design_without_designing(monkeypatch, [fa, "-o", out])
    assert [type(f).__name__ for f in pd.filters] == ["DuplicateFilter", "SetCoverFilter"]
    capsys.readouterr()
    # the device front end takes the filter, alone and behind the others
    from catch_amd import genome
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    tf, dup = TF(), DuplicateFilter()
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    genomes = [[genome.Genome.from_one_seq("ACGT" * 100)]]
    pd = ProbeDesigner(genomes, [tf, dup, scf], probe_length=100, probe_stride=50)
    assert pd._device_front_end_mode(genomes, dup, scf, [tf]) == pd._device_front_end_mode(genomes, dup, scf) == "per group"
    assert pd._device_front_end_mode(genomes, dup, scf, [PolyAFilter(12, 2), tf]) == "per group"
    assert not ProbeDesigner._strings_path_ok([dup, tf, scf])
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    assert pd._device_front_end_mode(genomes, dup, scf, [tf]) is None


def test_histogram_alone_leaves_the_design_unchanged(tmp_path, monkeypatch, capsys, caplog):
    """A design that runs on the host alone (the host front end, --skip-set-cover: the filters on Probe objects):
    --write-tm-histogram changes no byte of the FASTA, and the histogram counts every candidate that reached it."""
    from catch_amd import design
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    argv = [EBOLA, "--limit-target-genomes", "3", "-pl", "100", "-ps", "50", "--skip-set-cover", "--filter-polya", "20", "4"]
    plain, measured, hist = tmp_path / "plain.fasta", tmp_path / "measured.fasta", tmp_path / "h.tsv"
    design.main(design.parse_args(argv + ["-o", str(plain)]))
    with caplog.at_level(logging.INFO, logger="catch_amd.design"):
        pb = design.main(design.parse_args(argv + ["-o", str(measured), "--write-tm-histogram", str(hist), "--verbose"]))
    capsys.readouterr()
    assert plain.read_bytes() == measured.read_bytes() and plain.read_bytes().count(b">") > 100
    assert "tm filter: 0 candidates dropped (below 0, above 0)" in caplog.text
    tf = [f for f in pb.filters if type(f).__name__ == "TmFilter"]
    assert len(tf) == 1 and tf[0].dropped == [0, 0, 0]
    rows = [line.split("\t") for line in hist.read_text().splitlines()]
    assert rows[0] == ["tm_c", "candidates"]
    assert [int(r[0]) for r in rows[1:]] == list(range(int(rows[1][0]), int(rows[-1][0]) + 1))
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.utils import seq_io
    genomes = seq_io.read_genomes_from_fasta(EBOLA)[:3]
    cands = PolyAFilter(20, 4)._filter_strs(_windows([s for g in genomes for s in g.seqs], 100, 50))
    assert sum(int(r[1]) for r in rows[1:]) == len(cands) == sum(tf[0].histogram) > 1000
    assert 60 <= int(rows[1][0]) <= 70 and 78 <= int(rows[-1][0]) <= 90


def test_symbol_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    at = re.search(r"\b%s\s*\(" % NAME, hdr)
    assert at and "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 10
    assert hasattr(_lib.lib(), NAME)
    assert hasattr(engine.Candidates, "drop_tm")
    assert "thermo.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()


def test_tier_edges_sit_on_the_workgroup_sizes_claimed():
    """No GPU: the lengths of the kernel test are the last of one workgroup size and the first of the next."""
    assert [_tm_workgroup(L) for L, _ in TIER_EDGES] == [
        (256, 63568), (128, 34384), (128, 65104), (64, 34128), (64, 64848), (256, 1104)]
    assert all(_tm_workgroup(L)[0] == 256 for L, _ in SHAPES[:-1]) and _tm_workgroup(300)[0] == 128
    assert _tm_workgroup(1000) == (256, 1104) and _tm_workgroup(993) == (256, 1104)       # (poly(A) still stages 993)
    assert all(stride < L for L, stride in SHAPES + TIER_EDGES + UNSTAGED)
    assert all(b <= 65536 for b in (_tm_workgroup(L)[1] for L in range(2, 1200)))


# ------------------------------------------------------------------ GPU: the kernel against the NumPy rule
def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


def _expect(f, strs, mult, L):
    """(keep mask, [below, above, any], histogram) by the NumPy rule, multiplicities counted."""
    tm = f._tm_c_equal_length(strs, L)
    hist = np.zeros(128, dtype=np.int64)
    np.add.at(hist, np.clip(tm // 100, 0, 127), mult.astype(np.int64))
    if f.lo_c is None:
        return np.ones(len(strs), dtype=bool), [0, 0, 0], hist.tolist()
    below, above = tm < f.lo_c, tm > f.hi_c
    nb, na = int(mult[below].sum()), int(mult[above].sum())
    return ~(below | above), [nb, na, nb + na], hist.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("L,stride", SHAPES + TIER_EDGES + UNSTAGED)
def test_drop_tm_kernel_equals_numpy(ctx, L, stride):
    """catchhip_candidates_drop_tm against the NumPy rule in the three settings: the surviving positions,
    multiplicities and groups are the unfiltered list's, masked; `dropped` and all 128 bins are equal -- on a few
    hundred unique candidates (several workgroups, the last one partial)."""
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
        h_e = [_h_e(s) for s in strs0]
        assert ("AN" * L)[:L] in strs0 and max(h for h, _ in h_e) >= 24                     # the H >= 0 branch
        assert any(s[0] == "N" for s in strs0) and any(s[-1] == "N" for s in strs0)
        assert L < 3 or any("N" in s[1:-1] and "NA" * 3 not in s and "NG" * 3 not in s for s in strs0)    # an inner N
        if L >= 300:
            assert min(e for _, e in h_e) < -65535
        if L >= 1000:
            assert min(h for h, _ in h_e) < -65535
        for name, kwargs in _settings(strs0):
            f = TF(**kwargs)
            keep, want, hist = _expect(f, strs0, mult0, L)
            side = np.array([f._side(f._tm_c(s)) for s in strs0])       # the definition's exact counts
            assert want[:2] == [int(mult0[side == -1].sum()), int(mult0[side == 1].sum())], name
            _assert_not_vacuous(name, L, kwargs, [int((side == k).sum()) for k in (-1, 1)] + [int((side != 0).sum())], n)
            c = engine.Candidates(ctx, targets, L, stride)
            try:
                ncand = c.ncandidates
                f._apply_to_candidates(c)
                print(name, L, n, "kept", c.n, "dropped", f.dropped, "want", want)
                assert f.dropped == want, name
                assert f.histogram == hist and sum(hist) == ncand == int(mult0.sum()), name
                pos, mult, grp, _ = _snapshot(c, concat, L)
                assert c.n == int(keep.sum()) and c.ncandidates == ncand
                assert pos.tolist() == pos0[keep].tolist(), name
                assert mult.tolist() == mult0[keep].tolist(), name
                assert grp.tolist() == grp0[keep].tolist(), name
                # a second call on the filtered list: valid, nothing more goes, and it counts what is left
                dropped2, hist2 = c.drop_tm(f._q(L), f.offset_c, f.lo_c, f.hi_c)
                assert dropped2 == [0, 0, 0] and c.n == int(keep.sum()) and c.positions().tolist() == pos.tolist()
                assert hist2 == _expect(f, [s for s, k in zip(strs0, keep) if k], mult0[keep], L)[2]
            finally:
                c.close()
    finally:
        targets.close()


@pytest.mark.gpu
def test_drop_tm_kernel_grouped_and_errors(ctx):
    """Three groups, the first and third sharing strings (one string, two groups: two candidates); then the call
    without a histogram, an empty list, the bad arguments and the call after a near-duplicate filter."""
    from catch_amd import engine
    L, stride = 64, 16
    mixed = _targets(5, L, stride, 300)[0]
    rich = "".join(np.random.default_rng(2).choice(list("GCGCAT"), size=1500))
    genomes = [[mixed], [rich], [mixed[:L + stride * 100], mixed[stride * 7:]]]
    concat = "".join(s for g in genomes for s in g)
    targets = engine.Targets(ctx, genomes)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        g0 = TF()
        lo, hi = _percentile_range([g0._tm_c(s) for s in strs0], 20, 60)
        f = TF(tm_range=(lo, hi))
        keep, want, hist = _expect(f, strs0, mult0, L)
        assert 0.05 * len(strs0) <= (~keep).sum() <= 0.95 * len(strs0) and want[0] > 0 and want[1] > 0
        c = engine.Candidates(ctx, targets, L, stride)
        f._apply_to_candidates(c)
        pos, mult, grp, _ = _snapshot(c, concat, L)
        assert f.dropped == want and f.histogram == hist
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (
            pos0[keep].tolist(), mult0[keep].tolist(), grp0[keep].tolist())
        assert set(grp.tolist()) == {0, 1, 2} and (grp == 1).sum() < (grp0 == 1).sum() // 2       # the GC-rich group: above
        c.close()
        # hist = NULL: the same list, the same counts, no histogram
        c = engine.Candidates(ctx, targets, L, stride)
        n, total = c.n, c.ncandidates
        dropped, none = c.drop_tm(f._q(L), f.offset_c, f.lo_c, f.hi_c, histogram=False)
        assert none is None and dropped == want and c.positions().tolist() == pos.tolist()
        c.close()
        c = engine.Candidates(ctx, targets, L, stride)
        q = f._q(L)
        # measuring without a histogram is nothing at all; measuring leaves the list as it is
        assert c.drop_tm(q, 27315, histogram=False) == ([0, 0, 0], None) and c.n == n
        dropped, h = c.drop_tm(q, 27315)
        assert dropped == [0, 0, 0] and h == hist and c.n == n and c.positions().tolist() == pos0.tolist()
        # a range that holds everything: nothing dropped, the list stands
        assert c.drop_tm(q, 27315, -30000, 30000)[0] == [0, 0, 0] and c.n == n
        for bad in ((-8199, 27315, None, None), (0, 27315, 0, 1), (q, 27315, 7001, 7000)):
            with pytest.raises(ValueError, match="candidates_drop_tm"):
                c.drop_tm(*bad)
        with pytest.raises(ValueError, match="go together"):
            c.drop_tm(q, 27315, 7000, None)
        assert c.n == n
        assert c.drop_tm(-8200, 27315, histogram=False) == ([0, 0, 0], None)             # the largest q allowed
        # everything above -300 degrees: the list empties, and an empty list is valid
        dropped, h = c.drop_tm(q, 27315, -30000, -30000)
        assert dropped == [0, total, total] and h == hist and c.n == 0 and c.positions().size == 0
        assert c.drop_tm(q, 27315, 7000, 8000) == ([0, 0, 0], [0] * 128) and c.n == 0 and c.ncandidates == total
        c.close()
    finally:
        targets.close()
    targets = engine.Targets(ctx, [[rich]])
    try:
        c = engine.Candidates(ctx, targets, L, stride)
        c.ndf_hamming(np.arange(8, dtype=np.int32).reshape(2, 4), 1)
        with pytest.raises(ValueError, match="candidates_drop_tm: a near-duplicate filter was already applied"):
            c.drop_tm(q, 27315, 7000, 8000)
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


TM_OPTIONS = ["--filter-tm", "74", "79"]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"], ["--filter-with-lsh-minhash", "0.6"]],
                         ids=["dup", "hamming", "minhash"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, caplog, extra):
    """--filter-tm 74 79 --write-tm-histogram on the first 10 Ebola genomes: the kernel on the device's candidates and
    the host's strings give the same probes, the same histogram file and the same --verbose counts; every probe written
    lies in the range; the design differs from the one without the filter."""
    from catch_amd import engine
    from catch_amd.filter.tm_filter import TmFilter
    plain = [EBOLA, "--limit-target-genomes", "10"] + BASE + extra
    outs, hists, dropped, lines, calls = {}, {}, {}, {}, []
    real = engine.Candidates.drop_tm

    def counted(self, *a, **k):
        calls.append(self.n)
        got = real(self, *a, **k)
        calls.append(self.n)
        return got
    monkeypatch.setattr(engine.Candidates, "drop_tm", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn, hn = tmp_path / (front + ".fasta"), tmp_path / (front + ".tsv")
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="catch_amd.design"):
            pb, printed = _run_design(plain + TM_OPTIONS + ["--write-tm-histogram", str(hn), "--verbose", "-o", str(fn)],
                                      5, capsys)
        outs[front], hists[front] = fn.read_bytes(), hn.read_bytes()
        lines[front] = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tm filter:")]
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        tf = [f for f in pb.filters if type(f) is TmFilter]
        assert len(tf) == 1
        dropped[front] = (list(tf[0].dropped), list(tf[0].histogram))
        if front == "device":
            assert len(calls) == 2 and calls[0] > calls[1] > 0, "the device front end did not run the kernel"
    assert len(calls) == 2, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"] and hists["device"] == hists["host"]
    assert dropped["device"] == dropped["host"] and lines["device"] == lines["host"] and len(lines["device"]) == 1
    print(lines["device"], "unique candidates", calls)
    three, hist = dropped["device"]
    ncand = sum(hist)
    assert three[0] >= 1 and three[1] >= 1 and ncand - three[2] >= ncand / 4 and ncand > 3000
    assert sum(int(line.split(b"\t")[1]) for line in hists["device"].splitlines()[1:]) == ncand
    f = TF(tm_range=("74", "79"))
    probes = _read_sequences(tmp_path / "device.fasta")
    assert probes and all(f._keeps(s) for s in probes)
    # and the filter matters: another selection without it
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "nofilter.fasta"
    _run_design(plain + ["-o", str(fn)], 5, capsys)
    assert fn.read_bytes() != outs["device"]
    assert not all(f._keeps(s) for s in _read_sequences(fn))


@pytest.mark.gpu
def test_histogram_alone_on_the_device(tmp_path, monkeypatch, capsys):
    """--write-tm-histogram without --filter-tm on the device front end: the same probes as without it, and a histogram
    whose counts sum to the candidates that reached the filter."""
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    argv = [EBOLA, "--limit-target-genomes", "5"] + BASE
    plain, measured, hist = tmp_path / "plain.fasta", tmp_path / "measured.fasta", tmp_path / "h.tsv"
    _run_design(argv + ["-o", str(plain)], 3, capsys)
    _run_design(argv + ["-o", str(measured), "--write-tm-histogram", str(hist)], 3, capsys)
    assert plain.read_bytes() == measured.read_bytes() and plain.read_bytes().count(b">") > 0
    rows = [line.split("\t") for line in hist.read_text().splitlines()[1:]]
    assert sum(int(r[1]) for r in rows) == 1888                    # windows of the 5 genomes


@pytest.mark.gpu
def test_grid_point_with_tm_equals_design(tmp_path, capsys):
    """Two grid points of one dataset: each equals the design for that point, and the histogram counts the dataset's
    candidates once, as the single design does."""
    from catch_amd import design_grid
    fa = _write_records(tmp_path / "ebola5.fasta", _ebola_records(5))
    outdir, ghist, shist = tmp_path / "grid", tmp_path / "grid.tsv", tmp_path / "single.tsv"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "2", "--grid-cover-extension", "50", "25",
                                             "-o", str(outdir), "--write-tm-histogram", str(ghist)] + TM_OPTIONS))
    capsys.readouterr()
    single = tmp_path / "single.fasta"
    _run_design([fa] + BASE + ["-o", str(single), "--write-tm-histogram", str(shist)] + TM_OPTIONS, 1, capsys)
    assert (outdir / "ebola5.m2.e50.fasta").read_bytes() == single.read_bytes()
    assert ghist.read_bytes() == shist.read_bytes() and len(ghist.read_text().splitlines()) > 10
    plain = tmp_path / "plain.fasta"
    _run_design([fa] + BASE + ["-o", str(plain)], 1, capsys)
    assert plain.read_bytes() != single.read_bytes()
