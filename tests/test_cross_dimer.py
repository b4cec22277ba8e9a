"""Cross-dimers (catch_amd/filter/cross_dimer.py, csrc/cross.hip): the definition, the NumPy host path, the filter and
the command lines without a GPU; the two C entries against the NumPy model on the GPU.  Every comparison is of exact
integers.  The design commands on the GPU are in test_cross_dimer_design.py."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RC = str.maketrans("ACGT", "TGCA")

# the worked table of the specification: record, cross, partner
TABLE = [
    ("GATTACAGATTACCAGGTCA", 11, 1),
    ("TTTTTGGTAATCTGTTTTTT", 11, 0),      # holds revcomp of ACAGATTACCA; ties with 3
    ("CCCCCTGGTAATCCCCCCCC", 10, 0),      # ties with 3
    ("GATTACAGATTACCAGGTCA", 11, 1),      # a duplicate of record 0
    ("NNNNNNNN", 0, -1),
    ("acgtacgt", 0, -1),                  # lower case is no base
    ("TGACCTGGTANTCTGTAATC", 10, 0),      # revcomp of record 0 with an N at index 10
    ("A", 1, 0),
]


def _rc(s):
    return s[::-1].translate(_RC)


def _cd():
    from catch_amd.filter import cross_dimer
    return cross_dimer


def _random(rng, length, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=length)) if length else ""


def _walk(matrix, above):
    """The sequential walk over a run matrix: keep[i] iff no kept j < i has run > above."""
    keep = []
    for i in range(matrix.shape[0]):
        keep.append(not any(keep[j] and matrix[i, j] > above for j in range(i)))
    return np.array(keep, dtype=bool)


def _of_matrix(matrix):
    """(values, partners) of a run matrix with a zero diagonal."""
    n = matrix.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    values = matrix.max(axis=1)
    return values, np.where(values > 0, matrix.argmax(axis=1), -1)


# ------------------------------------------------------------------ without a GPU
def test_definition_gives_the_worked_table_and_the_single_pairs():
    cd = _cd()
    values, partners = cd.cross_dimers([r for r, _v, _p in TABLE])
    assert values == [v for _r, v, _p in TABLE]
    assert partners == [p for _r, _v, p in TABLE]
    assert cd.run("ACGT", "ACGT") == 4
    assert cd.run("AAAA", "TTTT") == 4
    assert cd.run("AAAA", "AAAA") == 0
    assert cd.cross_dimers(["ACGT"]) == ([0], [-1])
    assert cd.cross_dimers([]) == ([], [])


def test_run_is_symmetric_and_the_common_substring_with_the_reverse_complement():
    cd = _cd()
    rng = np.random.default_rng(5)
    for _ in range(40):
        s = _random(rng, int(rng.integers(0, 30)), "ACGTNa")
        t = _random(rng, int(rng.integers(0, 30)), "ACGTNa")
        r = cd.run(s, t)
        assert r == cd.run(t, s)
        # the longest common substring of s and revcomp(t) over bases only ('N' and 'a' stay what they are under _rc)
        u = _rc(t)
        lcs = max([k for k in range(1, min(len(s), len(u)) + 1)
                   for a in range(len(s) - k + 1) if set(s[a:a + k]) <= set("ACGT") and s[a:a + k] in u] + [0])
        assert r == lcs


def _planted_small(rng):
    seqs = [_random(rng, int(rng.integers(1, 41)), "ACGTNa-") for _ in range(12)]
    for i, j, k in ((0, 5, 9), (3, 4, 14), (7, 11, 6), (2, 2, 5)):
        piece = _random(rng, k)
        seqs[i] = (seqs[i] + piece)[-40:] if i != j else piece + seqs[i][:20] + _rc(piece)
        if i != j:
            seqs[j] = (_rc(piece) + seqs[j])[:40]
    return seqs


def test_numpy_host_path_equals_the_definition():
    cd = _cd()
    rng = np.random.default_rng(11)
    for _ in range(3):
        seqs = _planted_small(rng)
        assert sorted(set(len(s) for s in seqs))[0] >= 1 and max(len(s) for s in seqs) <= 40
        want_v, want_p = cd.cross_dimers(seqs)
        assert max(want_v) >= 9
        got_v, got_p = cd.cross_dimers_numpy(seqs)
        assert got_v.dtype == got_p.dtype == np.int32
        assert got_v.tolist() == want_v and got_p.tolist() == want_p
        m = cd.run_matrix(seqs)
        assert m.tolist() == [[0 if i == j else cd.run(s, t) for j, t in enumerate(seqs)] for i, s in enumerate(seqs)]
    v, p = cd.cross_dimers_numpy([r for r, _v, _p in TABLE])
    assert v.tolist() == [x for _r, x, _p in TABLE] and p.tolist() == [x for _r, _v, x in TABLE]
    for seqs in ([], ["ACGT"], ["", ""], ["", "ACGT", ""]):
        v, p = cd.cross_dimers_numpy(seqs)
        assert (v.tolist(), p.tolist()) == cd.cross_dimers(seqs)


def _chain():
    """a - b - c: b conflicts with a and with c at X = 12, a and c do not conflict."""
    rng = np.random.default_rng(3)
    left, right = _random(rng, 16), _random(rng, 16)
    a = left + _random(rng, 24)
    b = _random(rng, 10) + _rc(left) + _rc(right)
    c = _random(rng, 20) + right
    return [a, b, c, _random(rng, 40)]


def test_filter_on_the_host_path_is_the_sequential_walk(monkeypatch):
    cd = _cd()
    from catch_amd.probe import Probe
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    seqs = _chain()
    m = cd.run_matrix(seqs)
    assert m[0, 1] >= 16 and m[1, 2] >= 16 and m[0, 2] <= 12 and m[3].max() <= 12
    probes = [Probe.from_str(s) for s in seqs]
    f = cd.CrossDimerFilter(12)
    kept = f.filter(probes)
    assert [p.seq_str for p in kept] == [seqs[0], seqs[2], seqs[3]]          # a and c stay, b goes
    assert _walk(m, 12).tolist() == [True, False, True, True] == cd.walk(seqs, 12).tolist()
    assert (f.dropped, f.seen) == (1, 4)
    assert f.largest_before == int(m.max()) and f.largest_after == int(m[np.ix_([0, 2, 3], [0, 2, 3])].max())
    # grouped input is one list: b goes from its group although a is in another one
    f = cd.CrossDimerFilter(12)
    out = f.filter([[probes[0], probes[3]], [probes[1], probes[2], probes[0]]], input_is_grouped=True)
    assert [[p.seq_str for p in g] for g in out] == [[seqs[0], seqs[3]], [seqs[2], seqs[0]]]
    assert (f.dropped, f.seen) == (1, 4)
    # nothing above the threshold: nothing goes
    assert len(cd.CrossDimerFilter(int(m.max())).filter(probes)) == 4
    assert cd.CrossDimerFilter(5).filter([]) == []
    # the host path measures as the definition does
    v, p = cd.measure(seqs)
    assert (v.tolist(), p.tolist()) == cd.cross_dimers(seqs)


@pytest.mark.parametrize("bad", [0, -3, 2.5, "7", None, True])
def test_filter_refuses_a_bad_threshold(bad):
    with pytest.raises(ValueError):
        _cd().CrossDimerFilter(bad)


def _small_fasta(tmp_path):
    path = tmp_path / "probes.fasta"
    with open(path, "w") as f:
        for i, (r, _v, _p) in enumerate(TABLE):
            f.write(">r%d\n%s\n" % (i, r))
    return str(path)


def test_command_line_refusals(tmp_path, capsys):
    from catch_amd import design, design_grid, probe_report
    fa = _small_fasta(tmp_path)
    out = str(tmp_path / "o.fasta")
    for argv in (
            [fa, "-o", out, "--max-cross-dimer", "0"],
            [fa, "-o", out, "--max-cross-dimer", "-4"],
            [fa, "-o", out, "--max-cross-dimer", "2.5"],
            [fa, "-o", out, "--max-cross-dimer", "x"],
            [fa, "-o", out, "--max-cross-dimer", "30", "--add-reverse-complements"],
            [fa, "-o", out, "--max-cross-dimer", "30", "--skip-set-cover"],
            [fa, "-o", out, "--cross-dimer"]):
        for args_type in ("basic", "large"):
            with pytest.raises(SystemExit) as exc:
                design.parse_args(argv, args_type=args_type)
            assert exc.value.code == 2
    err = capsys.readouterr().err
    assert "--max-cross-dimer must be at least 1" in err and "--add-reverse-complements" in err
    assert "--skip-set-cover" in err and "--write-probe-report" in err
    args = design.parse_args([fa, "-o", out, "--cross-dimer", "--write-probe-report", str(tmp_path / "r.tsv")])
    assert args.cross_dimer and args.max_cross_dimer is None
    assert design.parse_args([fa, "-o", out, "--max-cross-dimer", "30"]).max_cross_dimer == 30
    for argv in (["-f", fa, "--max-cross-dimer", "0"], ["-f", fa, "--max-cross-dimer", "1.5"]):
        with pytest.raises(SystemExit) as exc:
            probe_report.parse_args(argv)
        assert exc.value.code == 2
    capsys.readouterr()
    # the other commands do not learn the option
    with pytest.raises(SystemExit):
        design_grid.parse_args([fa, "-o", out, "--grid-mismatches", "1", "--grid-cover-extension", "0",
                                "--max-cross-dimer", "30"])
    assert "unrecognized arguments" in capsys.readouterr().err


def test_probe_report_on_the_host_path(tmp_path, monkeypatch, capsys):
    from catch_amd import probe_report
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    fa = _small_fasta(tmp_path)
    plain, cross, judged = (str(tmp_path / n) for n in ("plain.tsv", "cross.tsv", "judged.tsv"))
    probe_report.main(probe_report.parse_args(["-f", fa, "-o", plain]))
    # without the new options: today's columns, today's bytes
    from catch_amd.filter import quality
    want = ["probe\tlength\tgc\thomopolymer\tdust\tstem\tdimer\ttm_c\tbackground_hits"]
    judge = probe_report.Judge(probe_report.parse_args(["-f", fa]))
    for i, (r, _v, _p) in enumerate(TABLE):
        five = quality.measure(r)
        tm = judge.tm._tm_c_equal_length([r], len(r)).tolist()[0] if len(r) >= 2 else None
        want.append("\t".join(["r%d" % i, str(len(r))] + [str(x) for x in five] + ["NA" if tm is None else str(tm), "NA"]))
    assert open(plain).read() == "\n".join(want) + "\n"
    probe_report.main(probe_report.parse_args(["-f", fa, "-o", cross, "--cross-dimer"]))
    rows = [line.split("\t") for line in open(cross).read().splitlines()]
    assert rows[0][-3:] == ["background_hits", "cross_dimer", "cross_partner"]
    assert [r[:-2] for r in rows] == [w.split("\t") for w in want]
    assert [r[-2:] for r in rows[1:]] == [[str(v), "NA" if p < 0 else str(p + 1)] for _r, v, p in TABLE]
    failed = probe_report.main(probe_report.parse_args(["-f", fa, "-o", judged, "--max-cross-dimer", "10"]))
    rows = [line.split("\t") for line in open(judged).read().splitlines()]
    assert rows[0][-3:] == ["cross_dimer", "cross_partner", "verdict"]
    assert [r[-1] for r in rows[1:]] == ["cross-dimer" if v > 10 else "ok" for _r, v, _p in TABLE]
    assert failed == [["cross-dimer"] if v > 10 else [] for _r, v, _p in TABLE]
    capsys.readouterr()


def test_second_header_second_table_library_and_makefile():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "catchhip_cross.h")).read()
    declared = set(re.findall(r"\b(catchhip_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"catchhip_cross_dimer", "catchhip_cross_dimer_graph"} == set(_lib.CROSS_PROTOTYPES)
    assert '#include "catchhip.h"' in hdr
    assert not declared & set(_lib.PROTOTYPES)
    main_hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert "cross_dimer" not in main_hdr
    L = _lib.lib()
    for name, (res, args) in _lib.CROSS_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.catchhip_abi_version() == 2
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "cross.hip" in srcs and "redundant.hip" in srcs


# ------------------------------------------------------------------ on the GPU
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256)
SIZES = (1, 2, 63, 64, 65, 129, 130)
# (i, j, bases, length of record i, where the piece starts in it, length of record j, where its reverse complement
#  starts): pairs on a diagonal tile (0 and 1), in tiles 0 and 1, in tiles 0 and 2 and in tiles 1 and 2; starts at 0, 30
# and 60, across the 32- and 64-bit word edges; "end": the piece runs to the record's last character
PLANTS = (
    (3, 40, 20, 64, 30, 32, 12),          # ... 40: to the end
    (66, 100, 33, 63, 30, 33, 0),         # both to the end
    (5, 70, 64, 128, 60, 64, 0),
    (7, 129, 65, 65, 0, 127, 60),
    (64, 128, 100, 256, 60, 100, 0),
    (10, 11, 100, 255, 30, 100, 0),
    (60, 61, 20, 31, 0, 64, 30),
)
LONG = {20: 129, 50: 255, 90: 256, 110: 127, 120: 128, 125: 100}
_shared = {}


def _master():
    """130 records and their run matrix (the model, computed once): most of at most 64 characters, about a dozen long
    ones, 5 % N and some lower case, reverse-complemented pieces planted between the pairs of PLANTS."""
    if "m" not in _shared:
        cd = _cd()
        rng = np.random.default_rng(20261021)
        short = [x for x in LENGTHS if x <= 65]
        lens = [int(rng.choice(short)) for _ in range(130)]
        for i, n in LONG.items():
            lens[i] = n
        for i, j, _k, li, _oi, lj, _oj in PLANTS:
            lens[i], lens[j] = li, lj
        assert set(lens) == set(LENGTHS) and sum(1 for x in lens if x >= 100) <= 14
        alphabet = list("ACGT") * 23 + ["N"] * 5 + ["a", "c", "g"]          # 5 % N, 3 % lower case
        seqs = [_random(rng, n, alphabet) for n in lens]
        for i, j, k, _li, oi, _lj, oj in PLANTS:
            piece = _random(rng, k)
            seqs[i] = seqs[i][:oi] + piece + seqs[i][oi + k:]
            seqs[j] = seqs[j][:oj] + _rc(piece) + seqs[j][oj + k:]
        assert [len(s) for s in seqs] == lens
        m = cd.run_matrix(seqs)
        for i, j, k, *_rest in PLANTS:
            assert m[i, j] >= k and m[j, i] == m[i, j]
        _shared["m"] = (seqs, m)
    return _shared["m"]


@pytest.mark.gpu
def test_device_gives_the_worked_table(ctx):
    from catch_amd import engine
    values, partners = engine.cross_dimer(ctx, [r for r, _v, _p in TABLE])
    assert values.dtype == partners.dtype == np.int32
    assert values.tolist() == [v for _r, v, _p in TABLE]
    assert partners.tolist() == [p for _r, _v, p in TABLE]
    for a, b, want in (("ACGT", "ACGT", 4), ("AAAA", "TTTT", 4), ("AAAA", "AAAA", 0)):
        values, partners = engine.cross_dimer(ctx, [a, b])
        assert values.tolist() == [want, want] and partners.tolist() == ([1, 0] if want else [-1, -1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_model_at_tile_and_word_edges(ctx, n):
    from catch_amd import engine
    seqs, m = _master()
    want_v, want_p = _of_matrix(m[:n, :n])
    values, partners = engine.cross_dimer(ctx, seqs[:n])
    wrong = [(i, int(values[i]), int(partners[i]), int(want_v[i]), int(want_p[i])) for i in range(n)
             if values[i] != want_v[i] or partners[i] != want_p[i]]
    assert not wrong, wrong[:10]
    # the same call again: the same bytes
    again = engine.cross_dimer(ctx, seqs[:n])
    assert again[0].tobytes() == values.tobytes() and again[1].tobytes() == partners.tobytes()


@pytest.mark.gpu
def test_device_agrees_with_the_host_path_entry(ctx):
    cd = _cd()
    seqs, m = _master()
    want_v, want_p = _of_matrix(m)
    got_v, got_p = cd.cross_dimers_numpy(seqs)
    assert got_v.tolist() == want_v.tolist() and got_p.tolist() == want_p.tolist()
    values, partners = cd.measure(seqs)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()


@pytest.mark.gpu
def test_ties_duplicates_and_a_record_that_is_its_own_reverse_complement(ctx):
    from catch_amd import engine
    cd = _cd()
    rng = np.random.default_rng(8)
    s = _random(rng, 100)
    others = [_random(rng, 100) for _ in range(70)]
    # three equal records and their reverse complement, spread over two tiles: every partner is the smallest index
    seqs = others[:5] + [s] + others[5:30] + [s] + others[30:66] + [_rc(s)] + others[66:] + [s]
    where = [i for i, x in enumerate(seqs) if x == s]
    rc_at = seqs.index(_rc(s))
    assert where == [5, 31, 73] and rc_at == 68
    values, partners = engine.cross_dimer(ctx, seqs)
    want_v, want_p = cd.cross_dimers_numpy(seqs)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()
    assert [int(values[i]) for i in where] == [100] * 3 and [int(partners[i]) for i in where] == [rc_at] * 3
    assert int(values[rc_at]) == 100 and int(partners[rc_at]) == 5
    # (ACGT) x 25 is its own reverse complement: its own pairing is not counted, a second copy is a partner
    own = "ACGT" * 25
    assert _rc(own) == own and cd.run(own, own) == 100
    seqs = others[:3] + [own] + others[3:9]
    values, partners = engine.cross_dimer(ctx, seqs)
    want_v, want_p = cd.cross_dimers_numpy(seqs)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()
    assert 0 < int(values[3]) < 30
    values, partners = engine.cross_dimer(ctx, seqs + [own])
    assert int(values[3]) == 100 == int(values[10]) and int(partners[3]) == 10 and int(partners[10]) == 3


def _edges(ptr, idx):
    return {(i, int(j)) for i in range(len(ptr) - 1) for j in idx[ptr[i]:ptr[i + 1]]}


@pytest.mark.gpu
@pytest.mark.parametrize("above", [5, 10, 11, 99, 100])
def test_graph_equals_the_model(ctx, above):
    from catch_amd import engine
    seqs, m = _master()
    n = len(seqs)
    g = engine.RedundancyGraph.cross_dimer(ctx, seqs, above)
    try:
        ptr, idx = g.fetch()
        want = {(i, j) for i in range(n) for j in range(n) if m[i, j] > above}
        assert g.n == n and g.nedges == len(want) == int(ptr[-1]) == idx.size
        assert _edges(ptr, idx) == want
        assert all((j, i) in want for i, j in want) and not any(i == j for i, j in want)
        for i in range(n):
            row = idx[ptr[i]:ptr[i + 1]]
            assert (np.diff(row.astype(np.int64)) > 0).all()
        assert g.naive().tolist() == _walk(m, above).tolist()
        rows = g.rows()
        try:
            assert rows.n == g.nedges + n
        finally:
            rows.close()
    finally:
        g.close()
    if above == 100:
        assert len(want) == 0                                        # the empty graph of a full list
    if above == 99:
        assert want == {(64, 128), (128, 64), (10, 11), (11, 10)}


@pytest.mark.gpu
def test_graph_of_nothing_of_one_and_of_the_worked_table(ctx):
    from catch_amd import engine
    g = engine.RedundancyGraph.cross_dimer(ctx, [], 5)
    try:
        ptr, idx = g.fetch()
        assert (g.n, g.nedges, ptr.tolist(), idx.size) == (0, 0, [0], 0) and g.naive().tolist() == []
    finally:
        g.close()
    g = engine.RedundancyGraph.cross_dimer(ctx, ["ACGT" * 25], 5)
    try:
        assert (g.n, g.nedges) == (1, 0) and g.fetch()[0].tolist() == [0, 0] and g.naive().tolist() == [True]
    finally:
        g.close()
    seqs = [r for r, _v, _p in TABLE]
    m = _cd().run_matrix(seqs)
    g = engine.RedundancyGraph.cross_dimer(ctx, seqs, 10)
    try:
        assert _edges(*g.fetch()) == {(i, j) for i in range(8) for j in range(8) if m[i, j] > 10} == {
            (0, 1), (1, 0), (1, 3), (3, 1)}
        assert g.naive().tolist() == [True, False, True, True, True, True, True, True]
    finally:
        g.close()
    with pytest.raises(ValueError, match="at least 1"):
        engine.RedundancyGraph.cross_dimer(ctx, seqs, 0)
    v, p = engine.cross_dimer(ctx, [])
    assert v.size == p.size == 0


@pytest.mark.gpu
def test_both_entries_on_poisoned_memory(ctx, monkeypatch):
    from catch_amd import engine
    seqs, m = _master()
    want_v, want_p = _of_matrix(m)
    want_edges = {(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if m[i, j] > 11}
    outs = {}
    for poison in (None, 255, 85):
        # (set before the context is created: its first blocks are poisoned too)
        if poison is None:
            monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
        else:
            monkeypatch.setenv("CATCHHIP_POOL_POISON", str(poison))
        c = engine.Context(ctx.device)
        try:
            values, partners = engine.cross_dimer(c, seqs)
            g = engine.RedundancyGraph.cross_dimer(c, seqs, 11)
            try:
                ptr, idx = g.fetch()
                keep = g.naive()
            finally:
                g.close()
        finally:
            c.close()
        outs[poison] = (values.tobytes(), partners.tobytes(), ptr.tobytes(), idx.tobytes(), keep.tobytes())
        assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist(), poison
        assert _edges(ptr, idx) == want_edges, poison
    monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
    assert outs[None] == outs[255] == outs[85]


@pytest.mark.gpu
def test_a_longer_record_is_refused_by_both_entries_and_measured_on_the_host(ctx, caplog):
    import logging
    from catch_amd import engine
    cd = _cd()
    rng = np.random.default_rng(2)
    long = _random(rng, 257)
    seqs = [_random(rng, 40), long, _rc(long[100:140]), _random(rng, 64)]
    with pytest.raises(ValueError, match="257 characters.*at most 256"):
        engine.cross_dimer(ctx, seqs)
    with pytest.raises(ValueError, match="257 characters.*at most 256"):
        engine.RedundancyGraph.cross_dimer(ctx, seqs, 20)
    with caplog.at_level(logging.WARNING, logger="catch_amd.filter.cross_dimer"):
        values, partners = cd.measure(seqs)
    assert any("host path" in r.getMessage() for r in caplog.records)
    want_v, want_p = cd.cross_dimers_numpy(seqs)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()
    assert int(values[1]) == 40 and int(partners[1]) == 2
    # 256 is taken
    values, partners = engine.cross_dimer(ctx, [long[:256], _rc(long[:256])])
    assert values.tolist() == [256, 256] and partners.tolist() == [1, 0]
    # more records than one call pairs: refused from the sizes alone (the offsets say 2^20 + 1 empty records)
    n = (1 << 20) + 1
    off = np.zeros(n + 1, dtype=np.int64)
    buf = np.zeros(1, dtype=np.uint8)
    out = np.zeros(1, dtype=np.int32)
    rc = ctx._L.catchhip_cross_dimer(ctx._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                     off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == -1 and b"1048576" in ctx._L.catchhip_last_error()
