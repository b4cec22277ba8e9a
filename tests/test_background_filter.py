"""The background k-mer screen of the design command (--background, --background-kmer, --background-max-hits,
--write-background-histogram; not in the reference).  The rule exists three times in
catch_amd/filter/background_filter.py: _hits and _keeps (straight from the definition, a Python set of strings: the
oracle), the NumPy form of the host path and the kernel of the device front end
(catchhip_candidates_drop_background, against an engine.KmerIndex).  Here: hand-computed values against _hits, NumPy
against _keeps, the index against canonical codes rolled in Python integers, the kernel against NumPy, and the design
commands on both front ends.

Backgrounds and targets are seeded.  A background is random bases with a few Ns plus a CLUSTERED part -- k-mers that
begin with AAAA, so that their canonical codes share the directory's leading bits and a bucket is longer than the 4
codes the kernel compares one by one (asserted on the fetched index).  Targets are random bases with isolated Ns and
planted pieces of the background, K to K + 8 long, forward or reverse-complemented, so that a candidate has from 0 to
more than H hits; every filtering case asserts that it drops between 5 % and 95 %."""
import gzip
import logging
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
NAMES = ("catchhip_kmer_index_create", "catchhip_kmer_index_fetch", "catchhip_kmer_index_destroy",
         "catchhip_candidates_drop_background")
COMP = str.maketrans("ACGT", "TGCA")
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def BF(*a, **k):
    from catch_amd.filter.background_filter import BackgroundFilter
    return BackgroundFilter(*a, **k)


def _rc(s):
    return s.translate(COMP)[::-1]


def _canonical_codes(records, K):
    """The canonical code of every valid k-mer of the records, in Python integers (position order)."""
    out, mask = [], (1 << (2 * K)) - 1
    for s in records:
        fwd = rc = run = 0
        for ch in s:
            c = CODE.get(ch)
            if c is None:
                run = 0
                continue
            fwd = ((fwd << 2) | c) & mask
            rc = (rc >> 2) | ((c ^ 2) << (2 * K - 2))
            run += 1
            if run >= K:
                out.append(min(fwd, rc))
    return out


# ------------------------------------------------------------------ inputs
def _random_bases(rng, n, n_rate=0.0):
    s = "".join(rng.choice(list("ACGT"), size=n))
    if n_rate:
        s = "".join("N" if x else c for c, x in zip(s, (rng.random(n) < n_rate).tolist()))
        while "NN" in s:                # (two adjacent Ns end a window of the candidate generator)
            s = s.replace("NN", "NA")
    return s


def _background(seed, K, n=None):
    """Records: random bases with a few Ns (few of them at a small K, where a random k-mer hits 2 G / 4^K of the time),
    a palindrome of Gs and Cs (K = 32: a canonical code with the top bit set) and 150 k-mers that begin with AAAA (one
    bucket of the directory's, or a few)."""
    rng = np.random.default_rng(seed)
    n = n or (300 if K < 12 else 3000)
    gc = "G" * (K // 2) + "C" * (K - K // 2)
    clustered = ["AAAA" + _random_bases(rng, K - 4) for _ in range(150)]
    return [_random_bases(rng, n, 0.003), "G" + _random_bases(rng, K + 5) + "C", gc, "N".join(clustered)]


def _planted(rng, n, records, K, every):
    """n characters: random bases with isolated Ns, and about every `every` characters a piece of a record (half of
    them of the first), K .. K + 8 long (K + 16 where the pieces stand close: see _every), forward or
    reverse-complemented."""
    s = list(_random_bases(rng, n, 0.004))
    at = int(rng.integers(0, every))
    span = 8 if every >= K else 16
    while at + K + span < n:
        rec = records[0 if rng.random() < 0.5 else int(rng.integers(0, len(records)))]
        ln = min(K + int(rng.integers(0, span + 1)), len(rec))
        a = int(rng.integers(0, len(rec) - ln + 1))
        piece = rec[a:a + ln]
        if rng.random() < 0.5:
            piece = _rc(piece)
        s[at:at + ln] = piece
        at += ln + int(rng.integers(1, 2 * every))
    s = "".join(s)[:n]
    while "NN" in s:
        s = s.replace("NN", "NA")
    return s


def _every(K, L):
    """The spacing of the planted pieces: wide where a candidate holds many k-mers, narrow where it holds a few (a
    window of K or K + 1 characters must lie inside a piece to hit)."""
    return max(L, 2 * K) if L - K >= 8 else K // 2


def _targets(seed, L, stride, ncand, records, K):
    """Sequences whose windows give about ncand candidates, a good part of them more than once."""
    rng = np.random.default_rng(seed)
    s = _planted(rng, L + stride * (ncand - 1), records, K, _every(K, L))
    half = L + stride * (ncand // 2 + 3)
    return [s, s[:half], s[stride * (ncand // 3):]]


def _windows(seqs, L, stride):
    from catch_amd.filter import candidate_probes
    return [c for q in seqs for c in candidate_probes.candidate_strings_from_sequences([q], L, stride)]


def _definition(f, strs):
    """(keep list, dropped, histogram) straight from _hits, string by string."""
    hits = [f._hits(s) for s in strs]
    hist = [0] * 256
    for s, h in zip(strs, hits):
        if len(s) >= f.kmer:
            hist[min(h, 255)] += 1
    keep = [f.max_hits is None or h <= f.max_hits for h in hits]
    return keep, keep.count(False), hist


# the kernel's workgroup by candidate length (csrc/background.hip): rows copied into LDS as the Tm kernel copies them, at
# an odd pitch of 4 * ceil((L + 15) / 16) + 1 dwords, and behind them, once per workgroup, 257 64-bit counters (2,056
# bytes); as many of 256 / 128 / 64 rows as fit 64 KB, read from global memory when 64 do not
SHAPES = [(64, 32), (100, 50), (130, 50), (300, 100)]
TIER_EDGES = [(225, 40), (226, 40), (465, 97), (466, 97), (961, 200), (962, 200)]
UNSTAGED = [(1000, 500)]
BG_EXTRA = 257 * 8


def _bg_workgroup(L):
    """(rows per workgroup, bytes of dynamic LDS) of the kernel's launch; 256 rows and only the extras: unstaged."""
    pitch = 4 * ((L + 30) // 16) + 1
    for rows in (256, 128, 64):
        if rows * pitch * 4 + BG_EXTRA <= 65536:
            return rows, rows * pitch * 4 + BG_EXTRA
    return 256, BG_EXTRA


# ------------------------------------------------------------------ host: the definition, by hand
def test_values_by_hand():
    f = BF(["ACGTACGTAC"], kmer=8, max_hits=0)
    assert f._background_words() == {"ACGTACGT", "CGTACGTA", "GTACGTAC", "TACGTACG"}
    assert f._hits("TTTTGTACGTACTTTT") == 1 and not f._keeps("TTTTGTACGTACTTTT")            # forward
    assert "TACGTACG" not in "ACGTACGTAC" and f._hits("AAAATACGTACGAAAA") == 1              # reverse complement only
    assert f._hits("TTTTGTACNTACTTTT") == 0 and f._keeps("TTTTGTACNTACTTTT")                # an N inside the only match
    assert f._hits("ttttgtacgtactttt") == 0 and f._hits("TTTTGTACgTACTTTT") == 0            # lower case is no base
    assert f._hits("GTACGTAC") == 1 and f._hits("GTACGTA") == 0 and f._keeps("GTACGTA")     # L = K, L = K - 1
    assert f._hits("ACGTACGTAC") == 3 and f._hits("") == 0
    assert BF(["ACGTACGTAC"], kmer=8, max_hits=3)._keeps("ACGTACGTAC")
    assert not BF(["ACGTACGTAC"], kmer=8, max_hits=2)._keeps("ACGTACGTAC")
    assert BF(["ACGTACGTAC"], kmer=8)._keeps("ACGTACGTAC")                                  # measuring only keeps everything
    # background k-mers never span two records: GGGGACGT and ACGTCCCC (each the other's reverse complement) hit, the
    # seven k-mers across the seam do not
    g = BF(["GGGGACGT", "ACGTCCCC"], kmer=8, max_hits=0)
    assert g._background_words() == {"GGGGACGT", "ACGTCCCC"} and g._hits("GGGGACGTACGTCCCC") == 2
    assert BF(["GGGGACGTACGTCCCC"], kmer=8)._hits("GGGGACGTACGTCCCC") == 9
    # a palindromic k-mer is one hit per position, not two
    p = BF(["ACGTACGT"], kmer=8, max_hits=0)
    assert _rc("ACGTACGT") == "ACGTACGT" and p._hits("ACGTACGT") == 1 and p._hits("ACGTACGTACGT") == 2
    # L < K: nothing dropped, nothing counted
    assert f._filter_strs(["GTACGTA", "GTACGTA"]) == ["GTACGTA", "GTACGTA"] and f.dropped == 0 and sum(f.histogram) == 0
    assert f._filter_strs(["GTACGTAC", "GTACGTAA", "GTACGTAC"]) == ["GTACGTAA"]
    assert f.dropped == 2 and f.histogram[:2] == [1, 2] and sum(f.histogram) == 3
    assert f.background_bases == 10 and f.distinct_kmers() == 3              # CGTACGTA and TACGTACG are one canonical k-mer
    for bad in (dict(kmer=7), dict(kmer=33), dict(kmer=8.0), dict(kmer=True), dict(max_hits=-1), dict(max_hits=1.5)):
        with pytest.raises(ValueError):
            BF(["ACGT"], **bad)


def test_background_without_a_valid_kmer_warns_and_drops_nothing(caplog):
    with caplog.at_level(logging.WARNING, logger="catch_amd.filter.background_filter"):
        f = BF(["ACGTACG", "ACGNACGTNACG", ""], kmer=8, max_hits=0)
    assert "no valid 8-mer" in caplog.text
    strs = ["ACGTACGT", "ACGNACGT", "AAAAAAAA"]
    assert f._filter_strs(strs) == strs and f.dropped == 0 and f.histogram[0] == 3 and f.distinct_kmers() == 0
    assert all(f._keeps(s) for s in strs) and f._background_words() == set()
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="catch_amd.filter.background_filter"):
        BF(["ACGTACGT"], kmer=8)
    assert caplog.text == ""
    with caplog.at_level(logging.WARNING, logger="catch_amd.filter.background_filter"):
        BF([], kmer=8)
    assert "no valid 8-mer" in caplog.text


# ------------------------------------------------------------------ host: NumPy against the definition
@pytest.mark.parametrize("K,L", [(8, 8), (8, 20), (16, 100), (31, 100), (32, 100), (32, 32)])
def test_numpy_rule_equals_definition(K, L):
    records = _background(100 + K, K)
    rng = np.random.default_rng(1000 * K + L)
    step = 7 if L - K >= 8 else 1
    s = _planted(rng, L + step * 399, records, K, _every(K, L))
    strs = [s[a:a + L] for a in range(0, len(s) - L + 1, step)] + [records[1][:L], records[2][:L]]
    strs = [x for x in strs if len(x) == L]
    strs += strs[:40]                                   # duplicates are counted
    assert any("N" in x for x in strs) and len(strs) > 400
    oracle = BF(records, kmer=K)
    hits = [oracle._hits(x) for x in strs]
    assert min(hits) == 0 and max(hits) > min(3, L - K) and 0.05 * len(strs) < sum(1 for h in hits if h) < 0.95 * len(strs)
    codes = oracle._background_codes()
    assert codes.dtype == np.uint64 and codes.tolist() == sorted(set(_canonical_codes(records, K)))
    if K == 32:     # canonical codes with the top bit set (the k-mer and its reverse complement begin with G) sort last
        assert int(codes[-1]) >= 1 << 63 and oracle._hits(records[2][:32]) == 1
        assert sum(1 for c in codes.tolist() if c >= 1 << 63) >= 2
    for H in (0, 3, L - K + 1, None):
        f = BF(records, kmer=K, max_hits=H)
        keep, dropped, hist = _definition(f, strs)
        assert keep == [f._keeps(x) for x in strs]
        if H in (0, 3) and L - K >= H:
            assert 0.02 * len(strs) < dropped < 0.95 * len(strs), (K, L, H, dropped)
        if H is None or H == L - K + 1:
            assert dropped == 0
        got = f._filter_strs(strs)
        assert got == [x for x, k in zip(strs, keep) if k], (K, L, H)
        assert f.dropped == dropped and f.histogram == hist and sum(hist) == len(strs)
        assert f._filter_strs(got) == got and f._filter_strs([]) == [] and f.dropped == dropped


def test_numpy_rule_in_chunks_and_mixed_lengths():
    from catch_amd import probe
    K = 12
    records = _background(5, K, 4000)
    rng = np.random.default_rng(6)
    s = _planted(rng, 40 + 3 * 17999, records, K, 60)
    a = [s[i:i + 40] for i in range(0, len(s) - 39, 3)]              # more than one chunk of 16,384
    assert len(a) > (1 << 14) + 1000
    f, g = BF(records, kmer=K, max_hits=1), BF(records, kmer=K, max_hits=1)
    got = f._filter_strs(a)
    tail = a[(1 << 14) - 50:(1 << 14) + 1000]                         # (the oracle across the chunk boundary)
    kept = set(got)
    assert [g._keeps(x) for x in tail] == [x in kept for x in tail]
    assert f.dropped == len(a) - len(got) and 0.05 * len(a) < len(got) < 0.95 * len(a) and sum(f.histogram) == len(a)
    # mixed lengths: the order is kept, strings below K count nothing
    mixed = a[:500] + [s[i:i + 70] for i in range(0, 7000, 20)] + ["", "A", "ACGTACGTACG", records[0][:12], records[0][:13]]
    random.Random(1).shuffle(mixed)
    f = BF(records, kmer=K, max_hits=1)
    keep, dropped, hist = _definition(f, mixed)
    assert f._filter_strs(mixed) == [x for x, k in zip(mixed, keep) if k]
    assert f.dropped == dropped and f.histogram == hist and sum(hist) == len(mixed) - 3
    assert 0.05 * len(mixed) < dropped < 0.95 * len(mixed)
    # Probe objects: the same rule, counted the same way
    h = BF(records, kmer=K, max_hits=1)
    probes = [probe.Probe.from_str(x) for x in mixed[:300] if x]
    left = h._filter(probes)
    assert [p.seq_str for p in left] == [p.seq_str for p in probes if h._keeps(p.seq_str)]
    assert h.dropped == len(probes) - len(left) > 0 and h._filter([]) == []


def test_write_histogram(tmp_path):
    rng = np.random.default_rng(3)
    piece = _random_bases(rng, 400)
    f = BF([piece], kmer=8)
    fn = tmp_path / "h.tsv"
    f.write_histogram(str(fn))
    assert fn.read_text() == "hits\tcandidates\n"                     # nothing counted: the header alone
    far = "".join("AC"[i % 2] for i in range(308))                      # no k-mer of it in the piece (asserted)
    assert f._hits(far) == 0
    strs = [piece[:308], _rc(piece[:308]), far, piece[:8] + far[:300]]
    assert [f._hits(x) for x in strs[:2]] == [301, 301] and 1 <= f._hits(strs[3]) <= 8
    assert f._filter_strs(strs) == strs and f.dropped == 0
    assert f.histogram[255] == 2 and f.histogram[0] == 1 and sum(f.histogram) == 4    # 301 hits: the last bin
    f.write_histogram(str(fn))
    rows = fn.read_text().splitlines()
    assert rows[0] == "hits\tcandidates" and len(rows) == 257 and rows[1] == "0\t1" and rows[-1] == "255\t2"
    assert [r.split("\t")[0] for r in rows[1:]] == [str(b) for b in range(256)]
    g = BF([piece], kmer=8, max_hits=2)
    assert g._filter_strs([far, piece[:10] + far[:298]]) == [far]
    g.write_histogram(str(fn))
    rows = fn.read_text().splitlines()              # rows 0 .. the highest non-empty bin
    assert len(rows) == 2 + g._hits(piece[:10] + far[:298]) and rows[1] == "0\t1" and rows[-1].endswith("\t1")


# ------------------------------------------------------------------ host: the option surface
def _write_records(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


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


def _ebola_background(genome, seed=11):
    """480 random bases alternating with pieces of 20 .. 40 bases cut from the genome every 450 bases, every other
    piece reverse-complemented: one record."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, at in enumerate(range(0, len(genome) - 40, 450)):
        piece = genome[at:at + int(rng.integers(20, 41))]
        parts += [_random_bases(rng, 480), _rc(piece) if n % 2 else piece]
    return "".join(parts)


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
    large = lambda argv: design.parse_args(argv, args_type="large")          # noqa: E731
    for parse, base in ((design.parse_args, ["x.fasta"]), (large, ["x.fasta"]), (design_grid.parse_args, GRID_BASE)):
        a = parse(base)
        assert (a.background, a.background_kmer, a.background_max_hits, a.write_background_histogram) == (None,) * 4
        a = parse(base + ["--background", "h.fa", "r.fa", "--background-kmer", "20", "--background-max-hits", "0",
                          "--write-background-histogram", "h.tsv"])
        assert (a.background, a.background_kmer, a.background_max_hits, a.write_background_histogram) == (
            ["h.fa", "r.fa"], 20, 0, "h.tsv")
        # (the parsers do not open the background: the files above do not exist)
        assert parse(base + ["--background", "h.fa", "--write-background-histogram", "h.tsv"]).background_max_hits is None
        assert parse(base + ["--background", "h.fa", "--background-max-hits", "5"]).background_kmer is None
        for k in ("8", "32"):
            assert parse(base + ["--background", "h.fa", "--background-max-hits", "5", "--background-kmer", k,
                                 "-pl", "32", "-ps", "16"]).background_kmer == int(k)
        for bad in (["--background", "h.fa", "--background-max-hits", "1", "--background-kmer", "7"],
                    ["--background", "h.fa", "--background-max-hits", "1", "--background-kmer", "33"],
                    ["--background", "h.fa", "--background-max-hits", "-1"],
                    ["--background", "h.fa"], ["--background", "h.fa", "--background-kmer", "20"],
                    ["--background-kmer", "20"], ["--background-max-hits", "0"],
                    ["--write-background-histogram", "h.tsv"], ["--background"],
                    ["--background", "h.fa", "--background-max-hits", "x"],
                    # the probe length is known to the parser and below K (24 by default)
                    ["--background", "h.fa", "--background-max-hits", "1", "-pl", "23", "-ps", "10"],
                    ["--background", "h.fa", "--background-max-hits", "1", "--background-kmer", "32", "-pl", "31", "-ps", "10"]):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert "error:" in capsys.readouterr().err, bad
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        design.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    for opt in ("--background FASTA [FASTA ...]", "--background-kmer K", "--background-max-hits H",
                "--write-background-histogram FILE"):
        assert opt in text
    assert "uncoverable" in text.split("--background-max-hits H")[-1].split("--write-background-histogram")[0]


def test_filter_order_and_strings_path(tmp_path, monkeypatch, capsys):
    from catch_amd.filter.probe_designer import ProbeDesigner
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    bg = _write_records(tmp_path / "bg.fasta", [("host", "acgtacgtacgtaryacgtacgtacgtacgtacgt"), ("second", "GGGGGGGGGGGGGGGGGGGGGGGGG")])
    out = str(tmp_path / "o.fasta")
    every = ["--filter-polya", "12", "2", "--filter-from-fasta", fa, "--filter-gc", "0.3", "0.7", "--max-hairpin-stem",
             "9", "--filter-tm", "70", "80", "--background", bg, "--background-kmer", "12", "--background-max-hits", "2"]
    for first, name in ((["--filter-with-lsh-hamming", "0"], "NearDuplicateFilterWithHammingDistance"),
                        (["--filter-with-lsh-minhash", "0.6"], "NearDuplicateFilterWithMinHash"), ([], "DuplicateFilter")):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--add-adapters"] + every + first)
        assert [type(f).__name__ for f in pd.filters] == [
            "FastaFilter", "PolyAFilter", "CompositionFilter", "StructureFilter", "TmFilter", "BackgroundFilter", name,
            "SetCoverFilter", "AdapterFilter"]
        assert pd._strings_path_ok(pd.filters) and pd._strings_prefix(pd.filters) == 8
        bf = pd.filters[5]
        # read with seq_io.read_fasta: upper-cased, degenerate codes N
        assert bf.background_seqs == ["ACGTACGTACGTANNACGTACGTACGTACGTACGT", "G" * 25]
        assert (bf.kmer, bf.max_hits, bf.background_bases) == (12, 2, 58)
    # --write-background-histogram alone adds ONE measuring filter; without the options the list is what it was
    pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--background", bg, "--background", bg,
                                                 "--write-background-histogram", str(tmp_path / "h.tsv")])
    assert [type(f).__name__ for f in pd.filters] == ["BackgroundFilter", "DuplicateFilter", "SetCoverFilter"]
    assert pd.filters[0].max_hits is None and pd.filters[0].kmer == 24
    assert (tmp_path / "h.tsv").read_text() == "hits\tcandidates\n"
    pd = _design_without_designing(monkeypatch, [fa, "-o", out])
    assert [type(f).__name__ for f in pd.filters] == ["DuplicateFilter", "SetCoverFilter"]
    pd = _design_without_designing(monkeypatch, [fa, "-o", out, "--filter-tm", "70", "80"])
    assert [type(f).__name__ for f in pd.filters] == ["TmFilter", "DuplicateFilter", "SetCoverFilter"]
    capsys.readouterr()
    # the device front end takes the filter, alone and behind the others
    from catch_amd import genome
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    bf, dup = BF(["ACGT" * 10], kmer=8, max_hits=0), DuplicateFilter()
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    genomes = [[genome.Genome.from_one_seq("ACGT" * 100)]]
    pd = ProbeDesigner(genomes, [bf, dup, scf], probe_length=100, probe_stride=50)
    assert pd._device_front_end_mode(genomes, dup, scf, [bf]) == pd._device_front_end_mode(genomes, dup, scf) == "per group"
    assert pd._device_front_end_mode(genomes, dup, scf, [PolyAFilter(12, 2), bf]) == "per group"
    assert not ProbeDesigner._strings_path_ok([dup, bf, scf])
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    assert pd._device_front_end_mode(genomes, dup, scf, [bf]) is None


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


def test_host_design_equals_brute_force_and_histogram_alone_changes_nothing(tmp_path, monkeypatch, capsys, caplog):
    """A design that runs on the host alone (the host front end, --skip-set-cover): the probes are the unique
    candidates _keeps keeps, in order; --write-background-histogram without --background-max-hits changes no byte of
    the FASTA, and the histogram counts every candidate that reached the filter."""
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.utils import seq_io
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    recs = _ebola_records(3)
    bg = _write_records(tmp_path / "bg.fasta", [("bg", _ebola_background(recs[0][1]))])
    argv = [EBOLA, "--limit-target-genomes", "3", "-pl", "100", "-ps", "50", "--skip-set-cover"]
    plain, measured, screened, hist = (tmp_path / n for n in ("plain.fasta", "measured.fasta", "screened.fasta", "h.tsv"))
    _run_design(argv + ["-o", str(plain)], 1, capsys)
    with caplog.at_level(logging.INFO, logger="catch_amd.design"):
        pb, _ = _run_design(argv + ["-o", str(measured), "--background", bg, "--background-kmer", "20",
                                    "--write-background-histogram", str(hist), "--verbose"], 1, capsys)
    assert plain.read_bytes() == measured.read_bytes() and plain.read_bytes().count(b">") > 100
    bf = [f for f in pb.filters if type(f) is BackgroundFilter]
    assert len(bf) == 1 and bf[0].dropped == 0
    assert ("background filter: 0 candidates dropped; %d background bases, %d distinct k-mers"
            % (bf[0].background_bases, bf[0].distinct_kmers())) in caplog.text
    genomes = seq_io.read_genomes_from_fasta(EBOLA)[:3]
    cands = _windows([s for g in genomes for s in g.seqs], 100, 50)
    rows = [line.split("\t") for line in hist.read_text().splitlines()]
    assert rows[0] == ["hits", "candidates"] and [int(r[0]) for r in rows[1:]] == list(range(len(rows) - 1))
    oracle = BF(list(seq_io.read_fasta(bg).values()), kmer=20, max_hits=0)
    want_hist = _definition(oracle, cands)[2]
    assert [int(r[1]) for r in rows[1:]] == want_hist[:len(rows) - 1] and sum(want_hist) == len(cands) > 1000
    assert len(rows) - 2 == max(b for b, v in enumerate(want_hist) if v) >= 10
    _run_design(argv + ["-o", str(screened), "--background", bg, "--background-kmer", "20", "--background-max-hits", "0"],
                1, capsys)
    kept = [s for s in cands if oracle._keeps(s)]
    assert 0.05 * len(cands) < len(cands) - len(kept) < 0.5 * len(cands)
    assert _read_sequences(screened) == list(dict.fromkeys(kept)) != _read_sequences(plain)


def test_symbols_declared_and_bound():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name, nargs in zip(NAMES, (8, 3, 1, 8)):
        at = re.search(r"\b%s\s*\(" % name, hdr)
        assert at, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
    at = re.search(r"\bcatchhip_kmer_index_create\s*\(", hdr)
    assert "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    at = re.search(r"\bcatchhip_candidates_drop_background\s*\(", hdr)
    assert "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    assert hasattr(engine.Candidates, "drop_background") and hasattr(engine, "KmerIndex")
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "background.hip" in mk and re.search(r"background\.o[^\n]*: stage\.h", mk)


def test_tier_edges_sit_on_the_workgroup_sizes_claimed():
    """No GPU: the lengths of the kernel test are the last of one workgroup size and the first of the next, by the
    counters the kernel's source keeps behind the rows."""
    src = open(os.path.join(REPO, "catch_amd", "csrc", "background.hip")).read()
    assert "#define BG_WORDS 257u" in src and "#define BG_EXTRA_BYTES (BG_WORDS * 8u)" in src and BG_EXTRA == 2056
    assert "rows * row_bytes + BG_EXTRA_BYTES > POLYA_LDS_BUDGET" in src
    assert [_bg_workgroup(L) for L, _ in TIER_EDGES] == [
        (256, 64520), (128, 35336), (128, 64008), (64, 34056), (64, 64776), (256, 2056)]
    assert all(_bg_workgroup(L)[0] == 256 for L, _ in SHAPES[:-1]) and _bg_workgroup(300)[0] == 128
    assert _bg_workgroup(1000) == (256, 2056) and _bg_workgroup(8)[0] == 256
    assert all(stride < L for L, stride in SHAPES + TIER_EDGES + UNSTAGED)
    assert all(b <= 65536 for b in (_bg_workgroup(L)[1] for L in range(8, 1200)))


# ------------------------------------------------------------------ GPU: the index against Python integers
def _index_backgrounds(K):
    rng = np.random.default_rng(40 + K)
    r = _random_bases(rng, 600)
    every_kth = list(_random_bases(rng, 40 * K))
    every_kth[K - 1::K] = "N" * len(every_kth[K - 1::K])
    big = list(_random_bases(rng, 70001))
    for at, ln in ((100, 1), (5000, K - 1), (20000, 3 * K), (40950, 200), (69990, 5)):
        big[at:at + ln] = "N" * ln
    big = "".join(big)
    cases = {
        "empty": [],
        "empty record": [""],
        "k-1 bases": [r[:K - 1]],
        "k bases": [r[:K]],
        "records of k bases": [r[a:a + K] for a in range(0, 5 * K, K)],         # side by side: no boundary k-mer
        "N every k-th": ["".join(every_kth)],
        "record and reverse complement": [r, _rc(r)],
        "one code": ["A" * 5000],
        "three records": [big[:30000], big[30000:30000 + K - 1], "", big[30000 + K - 1:]],
    }
    # valid positions on both sides of the scan tile (2048) and the sort tile (4096), and 8 sort tiles and one key
    for n in (2047, 2048, 2049, 4095, 4096, 4097, 8 * 4096 + 1):
        cases["%d valid" % n] = [_random_bases(rng, n + K - 1)]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 9, 16, 31, 32])
def test_index_equals_python_integers(ctx, K):
    from catch_amd import engine
    for name, records in _index_backgrounds(K).items():
        codes = _canonical_codes(records, K)
        want = np.array(sorted(set(codes)), dtype=np.uint64)
        index = engine.KmerIndex(ctx, records, K)
        try:
            got = index.fetch()
            print(K, name, "valid", index.n_valid, "unique", index.n_unique)
            assert (index.n_valid, index.n_unique) == (len(codes), len(want)), name
            assert got.dtype == np.uint64 and got.tolist() == want.tolist(), name
        finally:
            index.close()
        if name in ("empty", "empty record", "k-1 bases", "N every k-th"):
            assert len(codes) == 0
        elif name == "k bases":
            assert len(codes) == 1
        elif name == "records of k bases":
            assert len(codes) == 5
        elif name == "record and reverse complement":
            assert len(codes) == 2 * (600 - K + 1) and len(want) == len(set(_canonical_codes(records[:1], K)))
        elif name == "one code":
            assert len(codes) == 5001 - K and want.tolist() == [0]
        elif name.endswith(" valid"):
            assert len(codes) == int(name.split()[0])
        elif name == "three records":
            assert 69000 < len(codes) < 70001 - K and (K < 16 or len(want) > 60000)
    # the numpy form of the host path is the same list
    records = _index_backgrounds(K)["three records"]
    assert BF(records, kmer=K)._background_codes().tolist() == sorted(set(_canonical_codes(records, K)))
    with pytest.raises(ValueError, match="kmer_index_create: k must lie in 8 .. 32"):
        engine.KmerIndex(ctx, ["ACGT" * 20], 7)
    with pytest.raises(ValueError, match="kmer_index_create: k must lie in 8 .. 32"):
        engine.KmerIndex(ctx, ["ACGT" * 20], 33)


# ------------------------------------------------------------------ GPU: the kernel against the NumPy rule
def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


def _expect(f, strs, mult, L):
    """(keep mask, dropped, histogram) by the NumPy rule, multiplicities counted."""
    hits = f._hits_equal_length(strs, L)
    hist = np.zeros(256, dtype=np.int64)
    np.add.at(hist, np.minimum(hits, 255), mult.astype(np.int64))
    if f.max_hits is None:
        return np.ones(len(strs), dtype=bool), 0, hist.tolist()
    keep = hits <= f.max_hits
    return keep, int(mult[~keep].sum()), hist.tolist()


def _longest_bucket(codes, K):
    n = len(codes)
    P = min(max(int(n - 1).bit_length() if n > 1 else 0, 8), min(2 * K, 30))
    return int(np.bincount((codes >> np.uint64(2 * K - P)).astype(np.int64)).max()), P


KERNEL_CASES = [(K, L, s) for K in (8, 32)
                for L, s in [(K, 1), (K + 1, 1)] + SHAPES + TIER_EDGES + UNSTAGED]


@pytest.mark.gpu
@pytest.mark.parametrize("K,L,stride", KERNEL_CASES)
def test_drop_background_kernel_equals_numpy(ctx, K, L, stride):
    """catchhip_candidates_drop_background against the NumPy rule in the three settings: the surviving positions,
    multiplicities and groups are the unfiltered list's, masked; `dropped` and all 256 bins are equal -- on a few
    hundred to a few thousand unique candidates (several workgroups, the last one partial)."""
    from catch_amd import engine
    records = _background(200 + K, K)
    seqs = _targets(3000 + 37 * K + L, L, stride, (2500 if L <= 40 else 700) if L < 400 else 330, records, K)
    concat = "".join(seqs)
    targets = engine.Targets(ctx, [[s] for s in seqs])
    index = engine.KmerIndex(ctx, records, K)
    try:
        codes = index.fetch()
        assert codes.tolist() == sorted(set(_canonical_codes(records, K)))
        longest, P = _longest_bucket(codes, K)
        assert longest > 4, "no bucket takes the binary search"
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        n = len(strs0)
        assert mult0.max() > 1 and n % 64 != 0 and n > 256 and any("N" in s for s in strs0)
        oracle = BF(records, kmer=K)
        assert oracle._hits_equal_length(strs0[:60], L).tolist() == [oracle._hits(s) for s in strs0[:60]]
        hits = oracle._hits_equal_length(strs0, L)
        H = int(np.median(hits))            # (at K = 8 a long candidate meets the background by chance, often)
        assert hits.min() <= H < hits.max() and (L - K < 8 or hits.max() >= 8) and (K == 8 or hits.min() == 0)
        # some candidate looks into a long bucket: a k-mer that begins with AAAA, or ends with TTTT
        assert any("AAAA" in s or "TTTT" in s for s in strs0)
        for name, kwargs in (("filter + histogram", dict(max_hits=H)), ("filter only", dict(max_hits=H)),
                             ("histogram only", {})):
            f = BF(records, kmer=K, **kwargs)
            keep, want, hist = _expect(f, strs0, mult0, L)
            if kwargs:
                assert 0.05 * n <= (~keep).sum() <= 0.95 * n, (name, K, L, int((~keep).sum()), n)
            c = engine.Candidates(ctx, targets, L, stride)
            try:
                ncand = c.ncandidates
                if name == "filter only":
                    dropped, none = c.drop_background(index, H, histogram=False)
                    assert none is None and dropped == want
                else:
                    f._device_indexes[ctx.device] = index            # (the filter's own path, on the index above)
                    f._apply_to_candidates(c)
                    f._device_indexes.clear()
                    print(name, K, L, n, "kept", c.n, "dropped", f.dropped, "want", want, "bucket", longest, "P", P)
                    assert f.dropped == want, name
                    assert f.histogram == hist and sum(hist) == ncand == int(mult0.sum()), name
                pos, mult, grp, _ = _snapshot(c, concat, L)
                assert c.n == int(keep.sum()) and c.ncandidates == ncand
                assert pos.tolist() == pos0[keep].tolist(), name
                assert mult.tolist() == mult0[keep].tolist(), name
                assert grp.tolist() == grp0[keep].tolist(), name
                # a second call on the filtered list: valid, nothing more goes, and it counts what is left
                dropped2, hist2 = c.drop_background(index, f.max_hits)
                assert dropped2 == 0 and c.n == int(keep.sum()) and c.positions().tolist() == pos.tolist()
                assert hist2 == _expect(f, [s for s, k in zip(strs0, keep) if k], mult0[keep], L)[2]
            finally:
                c.close()
    finally:
        index.close()
        targets.close()


@pytest.mark.gpu
def test_drop_background_kernel_grouped_and_errors(ctx):
    """Three groups, the first and third sharing strings; then a threshold nothing passes, a background equal to the
    targets, an empty index, candidates shorter than K, the bad arguments, the call after a near-duplicate filter and
    one index used from two contexts."""
    from catch_amd import engine
    K, L, stride, H = 16, 64, 16, 2
    records = _background(77, K)
    rng = np.random.default_rng(8)
    mixed = _planted(rng, L + stride * 299, records, K, 70)
    other = _planted(rng, 1500, records[3:], K, 40)
    plain = _random_bases(rng, 1500)
    genomes = [[mixed], [other], [mixed[:L + stride * 100], mixed[stride * 7:]]]
    concat = "".join(s for g in genomes for s in g)
    targets = engine.Targets(ctx, genomes)
    index = engine.KmerIndex(ctx, records, K)
    empty = engine.KmerIndex(ctx, ["ACGTNACGT"], K)
    assert (empty.n_valid, empty.n_unique, empty.fetch().size) == (0, 0, 0)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        f = BF(records, kmer=K, max_hits=H)
        keep, want, hist = _expect(f, strs0, mult0, L)
        assert 0.05 * len(strs0) <= (~keep).sum() <= 0.95 * len(strs0)
        c = engine.Candidates(ctx, targets, L, stride)
        n, total = c.n, c.ncandidates
        f._apply_to_candidates(c)                                  # (builds the filter's own index of this device)
        assert list(f._device_indexes) == [ctx.device] and f.distinct_kmers() == index.n_unique
        pos, mult, grp, _ = _snapshot(c, concat, L)
        assert f.dropped == want and f.histogram == hist
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (pos0[keep].tolist(), mult0[keep].tolist(), grp0[keep].tolist())
        assert set(grp.tolist()) == {0, 1, 2}
        c.close()
        own = f._device_indexes[ctx.device]
        c = engine.Candidates(ctx, targets, L, stride)
        f._apply_to_candidates(c)                                  # the same index again, not another build
        assert f._device_indexes[ctx.device] is own and f.dropped == 2 * want and c.n == int(keep.sum())
        c.close()
        f.close()
        assert f._device_indexes == {} and not own._h
        c = engine.Candidates(ctx, targets, L, stride)
        # measuring without a histogram is nothing at all; measuring leaves the list as it is
        assert c.drop_background(index, histogram=False) == (0, None) and c.n == n
        dropped, h = c.drop_background(index)
        assert dropped == 0 and h == hist and c.n == n and c.positions().tolist() == pos0.tolist()
        # a threshold nothing passes: nothing dropped, the list stands
        assert c.drop_background(index, L - K + 1)[0] == 0 and c.n == n and c.positions().tolist() == pos0.tolist()
        # an empty index: nothing dropped, every candidate in bin 0
        dropped, h = c.drop_background(empty, 0)
        assert dropped == 0 and h == [total] + [0] * 255 and c.n == n
        with pytest.raises(ValueError, match="candidates_drop_background: max_hits must be >= 0"):
            c.drop_background(index, -1)
        assert c.n == n
        c.close()
        # candidates shorter than K: nothing dropped, nothing counted
        c = engine.Candidates(ctx, targets, K - 1, 5)
        short = c.n
        assert c.drop_background(index, 0) == (0, [0] * 256) and c.n == short > 0
        c.close()
    finally:
        targets.close()
    # H = 0 against a background equal to the targets drops everything
    targets = engine.Targets(ctx, [[plain]])
    same = engine.KmerIndex(ctx, [plain], K)
    try:
        c = engine.Candidates(ctx, targets, L, stride)
        total = c.ncandidates
        dropped, h = c.drop_background(same, 0)
        assert dropped == total > 50 and c.n == 0 and c.ncandidates == total and c.positions().size == 0
        assert h[L - K + 1] == total and sum(h) == total
        assert c.drop_background(same, 0) == (0, [0] * 256) and c.n == 0             # an empty list is valid
        c.close()
        # one index, two contexts of the device, one after the other
        t1 = engine.Targets(ctx, [[mixed]])
        c = engine.Candidates(ctx, t1, L, stride)
        first = c.drop_background(index, H)
        left = c.positions().tolist()
        assert 0 < first[0] and 0 < c.n < c.ncandidates
        c.close()
        t1.close()
        ctx2 = engine.Context(ctx.device)
        t2 = engine.Targets(ctx2, [[mixed]])
        c2 = engine.Candidates(ctx2, t2, L, stride)
        assert c2.drop_background(index, H) == first and c2.positions().tolist() == left
        assert index.fetch(ctx2).tolist() == index.fetch().tolist()
        c2.close()
        t2.close()
        ctx2.close()
        c = engine.Candidates(ctx, targets, L, stride)
        c.ndf_hamming(np.arange(8, dtype=np.int32).reshape(2, 4), 1)
        with pytest.raises(ValueError, match="candidates_drop_background: a near-duplicate filter was already applied"):
            c.drop_background(index, 0)
        c.close()
    finally:
        same.close()
        index.close()
        empty.close()
        targets.close()


@pytest.mark.gpu
def test_symbols_exported():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib
    for name in NAMES:
        assert hasattr(_lib.lib(), name), name


# ------------------------------------------------------------------ GPU: the design commands
def _ebola5(tmp_path):
    recs = _ebola_records(5)
    fa = _write_records(tmp_path / "ebola5.fasta", recs)
    bg = _write_records(tmp_path / "background.fasta", [("background", _ebola_background(recs[0][1]))])
    return fa, bg, recs


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"], ["--filter-with-lsh-minhash", "0.6"]],
                         ids=["dup", "hamming", "minhash"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, caplog, extra):
    """--background-kmer 20 --background-max-hits 0 --write-background-histogram on the first 5 Ebola genomes: the
    kernel on the device's candidates and the host's strings give the same probes, the same histogram file and the
    same --verbose line; no probe written shares a 20-mer with the background; the design differs from the one without."""
    from catch_amd import engine
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.utils import seq_io
    fa, bg, recs = _ebola5(tmp_path)
    oracle = BF(list(seq_io.read_fasta(bg).values()), kmer=20, max_hits=0)
    cands = _windows([s for _, s in recs], 100, 50)
    share = sum(1 for s in cands if not oracle._keeps(s)) / len(cands)
    print("candidates", len(cands), "share dropped", share)
    assert 0.05 <= share <= 0.5 and len(cands) > 1500                 # (the comparison below is not vacuous)
    plain = [fa] + BASE + extra
    options = ["--background", bg, "--background-kmer", "20", "--background-max-hits", "0"]
    outs, hists, dropped, lines, calls = {}, {}, {}, {}, []
    real = engine.Candidates.drop_background

    def counted(self, *a, **k):
        calls.append(self.n)
        got = real(self, *a, **k)
        calls.append(self.n)
        return got
    monkeypatch.setattr(engine.Candidates, "drop_background", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn, hn = tmp_path / (front + ".fasta"), tmp_path / (front + ".tsv")
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="catch_amd.design"):
            pb, printed = _run_design(plain + options + ["--write-background-histogram", str(hn), "--verbose", "-o", str(fn)],
                                      5, capsys)
        outs[front], hists[front] = fn.read_bytes(), hn.read_bytes()
        lines[front] = [r.getMessage() for r in caplog.records if r.getMessage().startswith("background filter:")]
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        bf = [f for f in pb.filters if type(f) is BackgroundFilter]
        assert len(bf) == 1
        dropped[front] = (bf[0].dropped, list(bf[0].histogram))
        if front == "device":
            assert len(calls) == 2 and calls[0] > calls[1] > 0, "the device front end did not run the kernel"
    assert len(calls) == 2, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"] and hists["device"] == hists["host"]
    assert dropped["device"] == dropped["host"] and lines["device"] == lines["host"] and len(lines["device"]) == 1
    print(lines["device"], "unique candidates", calls)
    gone, hist = dropped["device"]
    assert sum(hist) == len(cands) and gone == sum(1 for s in cands if not oracle._keeps(s))
    assert hist == _definition(oracle, cands)[2]
    assert sum(int(line.split(b"\t")[1]) for line in hists["device"].splitlines()[1:]) == len(cands)
    probes = _read_sequences(tmp_path / "device.fasta")
    assert probes and all(oracle._keeps(s) for s in probes)
    # and the filter matters: another selection without it
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "nofilter.fasta"
    _run_design(plain + ["-o", str(fn)], 5, capsys)
    assert fn.read_bytes() != outs["device"] and not all(oracle._keeps(s) for s in _read_sequences(fn))


@pytest.mark.gpu
def test_histogram_alone_on_the_device(tmp_path, monkeypatch, capsys):
    """--write-background-histogram without --background-max-hits on the device front end: the probes of a run
    without the options, byte for byte, and a histogram that counts every candidate."""
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fa, bg, recs = _ebola5(tmp_path)
    argv = [fa] + BASE
    plain, measured, hist = tmp_path / "plain.fasta", tmp_path / "measured.fasta", tmp_path / "h.tsv"
    _run_design(argv + ["-o", str(plain)], 3, capsys)
    _run_design(argv + ["-o", str(measured), "--background", bg, "--background-kmer", "20",
                        "--write-background-histogram", str(hist)], 3, capsys)
    assert plain.read_bytes() == measured.read_bytes() and plain.read_bytes().count(b">") > 0
    rows = [line.split("\t") for line in hist.read_text().splitlines()[1:]]
    assert sum(int(r[1]) for r in rows) == 1888 and len(rows) > 10            # windows of the 5 genomes


@pytest.mark.gpu
def test_grid_point_and_extend_probes_with_background(tmp_path, monkeypatch, capsys):
    """One grid point equals the design for that point, histogram included (a dataset's candidates counted once);
    an --extend-probes run (the rows loop: the host front end) equals the same run with _keeps in the filter's place."""
    from catch_amd import design_grid
    from catch_amd.filter.background_filter import BackgroundFilter
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fa, bg, recs = _ebola5(tmp_path)
    options = ["--background", bg, "--background-kmer", "20", "--background-max-hits", "0"]
    outdir, ghist, shist = tmp_path / "grid", tmp_path / "grid.tsv", tmp_path / "single.tsv"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "2", "--grid-cover-extension", "50", "25",
                                             "-o", str(outdir), "--write-background-histogram", str(ghist)] + options))
    capsys.readouterr()
    single = tmp_path / "single.fasta"
    _run_design([fa] + BASE + ["-o", str(single), "--write-background-histogram", str(shist)] + options, 1, capsys)
    assert (outdir / "ebola5.m2.e50.fasta").read_bytes() == single.read_bytes()
    assert ghist.read_bytes() == shist.read_bytes() and len(ghist.read_text().splitlines()) > 10
    plain = tmp_path / "plain.fasta"
    _run_design([fa] + BASE + ["-o", str(plain)], 1, capsys)
    assert plain.read_bytes() != single.read_bytes()
    # --extend-probes: the first 20 probes of the plain design exist already
    existing = _write_records(tmp_path / "existing.fasta",
                              [("p%d" % i, s) for i, s in enumerate(_read_sequences(plain)[:20])])
    ext, brute, without = tmp_path / "ext.fasta", tmp_path / "brute.fasta", tmp_path / "without.fasta"
    numpy_calls = []
    real = BackgroundFilter._filter_strs

    def counted(self, strs):
        numpy_calls.append(len(strs))
        return real(self, strs)
    monkeypatch.setattr(BackgroundFilter, "_filter_strs", counted)
    _run_design([fa] + BASE + ["--extend-probes", existing, "-o", str(ext)] + options, 2, capsys)
    assert numpy_calls and sum(numpy_calls) == 1888                 # (the host front end, on every window)
    monkeypatch.setattr(BackgroundFilter, "_filter_strs", lambda self, strs: [s for s in strs if self._keeps(s)])
    _run_design([fa] + BASE + ["--extend-probes", existing, "-o", str(brute)] + options, 2, capsys)
    _run_design([fa] + BASE + ["--extend-probes", existing, "-o", str(without)], 2, capsys)
    assert ext.read_bytes() == brute.read_bytes() != without.read_bytes() and ext.read_bytes().count(b">") > 0
