"""The uncovered regions of a probe set (catchhip_rows_uncovered in csrc/gaps.hip, Rows.uncovered,
Analyzer.uncovered_regions and its writers, --write-uncovered-regions / --write-uncovered-fasta).

The definition is restated here in NumPy (model_uncovered: depth by difference array, runs per sequence, counts
from the bytes); the restatement is checked without a GPU against a walk over every base in plain Python, and the
kernels are then compared with the restatement, exactly.

One refusal of the entry cannot be reached from here: deferred rows.  The library never hands a deferred table to a
caller (they live inside the fused scan + solve), so no test can pass one in; the check is the first thing the entry
does after its pointer checks."""
import ctypes
import functools
import logging
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EBOLA = os.path.join(GOLDEN, "ebola_zaire_100.fasta.gz")
SCAN_TILE = 2048                     # tests/test_primitives.py: elements per tile of the device-wide scan


# ------------------------------------------------------------------ the definition, restated
def model_uncovered(lengths, un, st, en, seqs=None, min_depth=1, min_length=1, min_unambig=1):
    """-> (universe, start, end, unambig, per_universe[ng, 3]): the reported regions by (universe, start), start
    and end local to the universe.  seqs: one str per universe, or None (every base counts as unambiguous)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ng = lengths.size
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    total = int(off[-1])
    un = np.asarray(un, dtype=np.int64)
    diff = np.zeros(total + 1, dtype=np.int64)
    if un.size:
        np.add.at(diff, off[un] + np.asarray(st, dtype=np.int64), 1)
        np.add.at(diff, off[un] + np.asarray(en, dtype=np.int64), -1)
    unc = np.cumsum(diff[:total]) < min_depth
    first = np.zeros(total + 1, dtype=bool)              # first[b]: base b is a sequence's first (or b == total)
    first[off[:-1][lengths > 0]] = True
    first[total] = True
    before = np.concatenate(([False], unc[:-1])) if total else unc
    after = np.concatenate((unc[1:], [False])) if total else unc
    starts = np.flatnonzero(unc & (~before | first[:total]))
    ends = np.flatnonzero(unc & (~after | first[1:])) + 1
    assert starts.size == ends.size
    if seqs is None:
        ua = ends - starts
    else:
        b = np.frombuffer("".join(seqs).encode("latin-1"), dtype=np.uint8)
        assert b.size == total
        csum = np.concatenate(([0], np.cumsum(np.isin(b, np.frombuffer(b"ACGT", dtype=np.uint8))))).astype(np.int64)
        ua = csum[ends] - csum[starts]
    keep = (ends - starts >= min_length) & (ua >= min_unambig)
    starts, ends, ua = starts[keep], ends[keep], ua[keep]
    univ = np.searchsorted(off, starts, side="right") - 1
    per = np.zeros((ng, 3), dtype=np.int64)
    if starts.size:
        per[:, 0] = np.bincount(univ, minlength=ng)
        per[:, 1] = np.bincount(univ, weights=(ends - starts).astype(np.float64), minlength=ng).astype(np.int64)
        np.maximum.at(per[:, 2], univ, ends - starts)
    return univ.astype(np.int32), starts - off[univ], ends - off[univ], ua.astype(np.int64), per


def walk_uncovered(lengths, un, st, en, seqs=None, min_depth=1, min_length=1, min_unambig=1):
    """The same by a walk over every base of every sequence, in plain Python."""
    out, per = [], []
    for u, n in enumerate(lengths):
        depth = [sum(1 for r in range(len(un)) if un[r] == u and st[r] <= b < en[r]) for b in range(n)]
        runs, b = [], 0
        while b < n:
            if depth[b] >= min_depth:
                b += 1
                continue
            a = b
            while b < n and depth[b] < min_depth:
                b += 1
            cnt = b - a if seqs is None else sum(1 for c in seqs[u][a:b] if c in "ACGT")
            if b - a >= min_length and cnt >= min_unambig:
                runs.append((u, a, b, cnt))
        out += runs
        per.append([len(runs), sum(r[2] - r[1] for r in runs), max([r[2] - r[1] for r in runs] + [0])])
    return out, per


def _as_list(result):
    univ, st, en, ua, per = result
    return list(zip(univ.tolist(), st.tolist(), en.tolist(), ua.tolist())), per.tolist()


EDGE_LENGTHS = (1, 63, 0, 64, 65, 127, 0, 0, 128, 129, 200, 0)


def _edge_table():
    """Rows over EDGE_LENGTHS (global offsets 0, 1, 64, 64, 128, 193, 320, .., 448, 577, 777), as (universe, start,
    end), and what each leaves open:
      u0 (1 base, word 0 bit 0)         open: a gap that is a whole sequence, starts at bit 0
      u1 [1, 64)   covered [0, 40)      open [40, 63): ends at bit 63 of word 0 and at the sequence's last base
      u3 [64, 128) no rows              open: fills a whole word
      u4 [128, 193) covered [10, 30)    open [0, 10) from the sequence's first base and bit 0; [30, 65) straddles a word
      u5 [193, 320) covered [0, 120)    open [120, 127): ends at the last base, the boundary 320 is word-aligned
      u8 [320, 448) covered [3, 128)    open [0, 3)
      u9 [448, 577) covered [0, 100)    open [100, 129): with u10's [0, 5) uncovered bases on both sides of the
      u10 [577, 777) covered [5, 150), [140, 199)   boundary 577, which falls mid-word; [199, 200) the last base"""
    rows = [(1, 0, 40), (4, 10, 30), (5, 0, 120), (8, 3, 128), (9, 0, 100), (10, 5, 150), (10, 140, 199)]
    un, st, en = (np.asarray(x) for x in zip(*rows))
    return un, st, en


def _edge_seqs():
    rng = np.random.default_rng(3)
    return ["".join(rng.choice(list("ACGT"), size=n)) for n in EDGE_LENGTHS]


def test_model_equals_the_walk_over_every_base():
    """No GPU: model_uncovered == walk_uncovered on the edge table (with and without sequences, depths 1 to 3,
    length and ambiguity filters) and on small random tables with zero-length sequences and N runs."""
    un, st, en = _edge_table()
    seqs = _edge_seqs()
    want = [(0, 0, 1), (1, 40, 63), (3, 0, 64), (4, 0, 10), (4, 30, 65), (5, 120, 127), (8, 0, 3), (9, 100, 129),
            (10, 0, 5), (10, 199, 200)]
    got, per = _as_list(model_uncovered(EDGE_LENGTHS, un, st, en))
    assert [g[:3] for g in got] == want and [g[3] for g in got] == [b - a for _u, a, b in want]
    assert per[4] == [2, 45, 35] and per[2] == [0, 0, 0]
    for kw in (dict(), dict(min_depth=2), dict(min_depth=3), dict(min_length=5), dict(min_length=36),
               dict(min_unambig=0), dict(min_unambig=24)):
        for s in (None, seqs):
            assert _as_list(model_uncovered(EDGE_LENGTHS, un, st, en, s, **kw)) == \
                tuple(walk_uncovered(EDGE_LENGTHS, un, st, en, s, **kw)), (kw, s is None)
    rng = np.random.default_rng(17)
    for _trial in range(20):
        lengths = rng.integers(0, 70, size=6)
        seqs = ["".join(rng.choice(list("ACGTNRacgt"), size=n, p=[.2, .2, .2, .2, .1, .02, .02, .02, .02, .02]))
                for n in lengths]
        un, st, en = [], [], []
        for u, n in enumerate(lengths):
            for _r in range(int(rng.integers(0, 4)) if n else 0):
                a = int(rng.integers(0, n))
                un.append(u); st.append(a); en.append(int(rng.integers(a + 1, n + 1)))
        for kw in (dict(), dict(min_depth=2), dict(min_length=3, min_unambig=2), dict(min_unambig=0)):
            assert _as_list(model_uncovered(lengths, un, st, en, seqs, **kw)) == \
                tuple(walk_uncovered(lengths, un, st, en, seqs, **kw)), (lengths, kw)


def test_symbol_declared_bound_and_built():
    from catch_amd import _lib, coverage_analysis, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_uncovered\s*\(", hdr)
    assert "catchhip_rows_uncovered" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["catchhip_rows_uncovered"][1]) == 9
    assert "gaps.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert callable(engine.Rows.uncovered)
    for name in ("uncovered_regions", "write_uncovered_regions", "_write_uncovered_rows", "write_uncovered_fasta"):
        assert callable(getattr(coverage_analysis.Analyzer, name))


def test_options_of_the_command_lines():
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd import coverage_analysis, design, design_naively
    base = ["-d", "a.fasta", "-f", "p.fasta", "-m", "2", "-l", "100"]
    for a in (apc.parse_args(base), design.parse_args(["a.fasta"]), design.parse_args(["a.fasta"], args_type="large"),
              design_naively.parse_args(["a.fasta"])):
        assert (a.write_uncovered_regions, a.write_uncovered_fasta, a.uncovered_min_depth, a.uncovered_min_length,
                a.uncovered_keep_ambiguous) == (None, None, 1, 1, False)
        assert coverage_analysis.uncovered_filters(a) == (1, 1, 1)
    a = apc.parse_args(base + ["--write-uncovered-regions", "r.tsv", "--write-uncovered-fasta", "r.fasta",
                               "--uncovered-min-depth", "2", "--uncovered-min-length", "30",
                               "--uncovered-keep-ambiguous"])
    assert (a.write_uncovered_regions, a.write_uncovered_fasta) == ("r.tsv", "r.fasta")
    assert coverage_analysis.uncovered_filters(a) == (2, 30, 0)
    for bad in (["--uncovered-min-depth", "0"], ["--uncovered-min-length", "0"]):
        with pytest.raises(ValueError, match="at least 1"):
            coverage_analysis.uncovered_filters(apc.parse_args(base + bad))


# ------------------------------------------------------------------ on the GPU: the entry against the restatement
class HostTargets:
    """catchhip_targets_create on one str per sequence, every sequence a genome of its own."""

    def __init__(self, ctx, seqs):
        from catch_amd._lib import c_i32p, c_i64p, c_u8p, check
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        buf = np.frombuffer(("".join(seqs) or "\0").encode("latin-1"), dtype=np.uint8).copy()
        off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
        sg = np.arange(max(len(seqs), 1), dtype=np.int32)
        check(ctx._L.catchhip_targets_create(ctx._h, buf.ctypes.data_as(c_u8p), off.ctypes.data_as(c_i64p),
                                             sg.ctypes.data_as(c_i32p), len(seqs), len(seqs), ctypes.byref(self._h)))

    def close(self):
        self.ctx._L.catchhip_targets_destroy(self._h)


def _device(ctx, lengths, un, st, en, seqs=None, **kw):
    """Rows.uncovered of a table with one set id per row (rows may overlap), sorted by (universe, start)."""
    from catch_amd import engine
    un, st, en = np.asarray(un, np.int64), np.asarray(st, np.int64), np.asarray(en, np.int64)
    rows = engine.Rows.from_host(ctx, np.arange(un.size), un, st, en, lengths)
    targets = None if seqs is None else HostTargets(ctx, seqs)
    try:
        return rows.uncovered(targets, **kw)
    finally:
        rows.close()
        if targets is not None:
            targets.close()


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("universe", "start", "end", "unambig", "per_universe")):
        assert g.shape == w.shape and np.array_equal(g, w), \
            (what, name, g.shape, w.shape, np.flatnonzero((g != w).reshape(-1))[:5].tolist() if g.shape == w.shape else None)
    assert got[0].dtype == np.int32 and all(g.dtype == np.int64 for g in got[1:])


@pytest.mark.gpu
def test_word_and_boundary_edges(ctx):
    """Sequences of 1, 63, 64, 65, 127, 128, 129 and 200 bases with zero-length ones between them; gaps at bit 0,
    up to bit 63, across a word, over a whole word, at a sequence's first and last base, and on both sides of a
    sequence boundary in the middle of a word (two regions)."""
    un, st, en = _edge_table()
    seqs = _edge_seqs()
    got = _device(ctx, EDGE_LENGTHS, un, st, en)
    _assert_equal(got, model_uncovered(EDGE_LENGTHS, un, st, en), "edges")
    regions = list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
    assert (9, 100, 129) in regions and (10, 0, 5) in regions and (3, 0, 64) in regions and len(regions) == 10
    for kw in (dict(), dict(min_depth=2), dict(min_length=5), dict(min_unambig=0), dict(min_unambig=24)):
        _assert_equal(_device(ctx, EDGE_LENGTHS, un, st, en, seqs, **kw),
                      model_uncovered(EDGE_LENGTHS, un, st, en, seqs, **kw), ("edges with targets", kw))
    # every boundary uncovered on both sides, at every alignment: sequences of 1 .. 130 bases, no rows at all
    lengths = np.arange(1, 131)
    got = _device(ctx, lengths, [], [], [])
    _assert_equal(got, model_uncovered(lengths, [], [], []), "every alignment")
    assert got[0].tolist() == list(range(130)) and got[2].tolist() == lengths.tolist()


@pytest.mark.gpu
def test_extremes(ctx):
    """A table without rows: one region per non-empty sequence.  Everything covered: no region, an empty table
    back, per_universe all zero.  One region of 1,000,000 bases in one sequence: exactly one."""
    lengths = [120, 0, 30, 1]
    univ, st, en, ua, per = _device(ctx, lengths, [], [], [])
    assert (univ.tolist(), st.tolist(), en.tolist(), ua.tolist()) == ([0, 2, 3], [0, 0, 0], [120, 30, 1], [120, 30, 1])
    assert per.tolist() == [[1, 120, 120], [0, 0, 0], [1, 30, 30], [1, 1, 1]]
    univ, st, en, ua, per = _device(ctx, lengths, [0, 0, 2, 3], [0, 50, 0, 0], [70, 120, 30, 1])
    assert univ.size == st.size == en.size == ua.size == 0 and per.tolist() == [[0, 0, 0]] * 4
    n = 1_000_000
    seq = "ACGT" * (n // 4)
    for lengths, seqs, rows, want in (
            ([n], [seq], ([], [], []), [(0, 0, n, n)]),
            ([77, n, 5], ["A" * 77, seq, "ACGTN"], ([0, 2], [0, 0], [77, 5]), [(1, 0, n, n)]),
            ([77, n + 2, 5], ["A" * 77, "N" + seq + "C", "ACGTN"], ([0, 1, 1, 2], [0, 0, n + 1, 0], [77, 1, n + 2, 5]),
             [(1, 1, n + 1, n)])):
        univ, st, en, ua, per = _device(ctx, lengths, *rows, seqs=seqs)
        assert list(zip(univ.tolist(), st.tolist(), en.tolist(), ua.tolist())) == want, lengths
        assert per[want[0][0]].tolist() == [1, n, n] and int(per[:, 0].sum()) == 1
    # a long region whose unambiguous bases are counted by the wavefront: N runs inside it
    rng = np.random.default_rng(8)
    b = np.frombuffer(seq.encode(), dtype=np.uint8).copy()
    for a in rng.integers(0, n - 5000, size=40):
        b[a:a + int(rng.integers(1, 5000))] = ord("N")
    s = b.tobytes().decode()
    _assert_equal(_device(ctx, [n], [0], [500_000], [500_003], seqs=[s]),
                  model_uncovered([n], [0], [500_000], [500_003], [s]), "long regions with N runs")


@pytest.mark.gpu
def test_depth(ctx):
    """min_depth 1, 2 and 3 on stacked rows of different sets; 70,000 sets over one 10-base range count as covered
    at min_depth 65,537: the depth is not modulo 2^16."""
    lengths = [300, 150]
    un = [0, 0, 0, 0, 1, 1]
    st = [10, 50, 90, 60, 0, 100]
    en = [200, 120, 100, 250, 150, 150]
    spans = {}
    for d in (1, 2, 3, 4):
        got = _device(ctx, lengths, un, st, en, min_depth=d)
        _assert_equal(got, model_uncovered(lengths, un, st, en, min_depth=d), ("stacked", d))
        spans[d] = list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
    assert spans[1] == [(0, 0, 10), (0, 250, 300)] and spans[2] == [(0, 0, 50), (0, 200, 300), (1, 0, 100)]
    assert spans[3] == [(0, 0, 60), (0, 120, 300), (1, 0, 150)] and spans[4] == [(0, 0, 90), (0, 100, 300), (1, 0, 150)]
    nsets = 70_000
    un = np.zeros(nsets + 1, np.int64)
    st = np.concatenate((np.full(nsets, 20), [5]))
    en = np.concatenate((np.full(nsets, 30), [12]))
    univ, a, b, _ua, per = _device(ctx, [100], un, st, en, min_depth=65_537)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 20), (30, 100)] and per.tolist() == [[2, 90, 70]]
    univ, a, b, _ua, per = _device(ctx, [100], un, st, en, min_depth=70_001)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 100)]


@pytest.mark.gpu
def test_filters(ctx):
    """min_length L against gaps of L - 1, L and L + 1; an all-N region is dropped at min_unambig 1 and kept at 0;
    a partly ambiguous region reports its count; R and lower-case letters count as ambiguous."""
    L = 70
    # gaps [0, 69), [100, 170), [200, 271), and the tail [300, 400)
    un, st, en = [0, 0, 0], [69, 170, 271], [100, 200, 300]
    for ml in (L - 1, L, L + 1, L + 2):
        got = _device(ctx, [400], un, st, en, min_length=ml)
        _assert_equal(got, model_uncovered([400], un, st, en, min_length=ml), ("min_length", ml))
        assert got[1].tolist() == [a for a, n in ((0, 69), (100, 70), (200, 71), (300, 100)) if n >= ml]
    seq = ("ACGT" * 10 + "N" * 30 + "ACGT" * 5 + "ACNNGT" * 5 + "ACGT" * 5 + "RYacgtACGTKM" * 5 + "ACGT" * 10 + "n" * 10)
    #      [0, 40) probe  [40, 70) N   probe          [90, 120)     probe          [140, 200)         probe    [240, 250)
    assert len(seq) == 250
    un, st, en = [0, 0, 0, 0], [0, 70, 120, 200], [40, 90, 140, 240]
    kept = _device(ctx, [250], un, st, en, seqs=[seq], min_unambig=0)
    assert list(zip(kept[1].tolist(), kept[2].tolist(), kept[3].tolist())) == \
        [(40, 70, 0), (90, 120, 20), (140, 200, 20), (240, 250, 0)]
    assert kept[4].tolist() == [[4, 130, 60]]
    dropped = _device(ctx, [250], un, st, en, seqs=[seq])
    assert list(zip(dropped[1].tolist(), dropped[2].tolist(), dropped[3].tolist())) == [(90, 120, 20), (140, 200, 20)]
    assert dropped[4].tolist() == [[2, 90, 60]]
    for mu in (0, 1, 20, 21):
        _assert_equal(_device(ctx, [250], un, st, en, seqs=[seq], min_unambig=mu),
                      model_uncovered([250], un, st, en, [seq], min_unambig=mu), ("min_unambig", mu))
    # without targets the count is the length
    plain = _device(ctx, [250], un, st, en)
    assert plain[3].tolist() == (plain[2] - plain[1]).tolist() == [30, 30, 60, 10]


# one covered and one uncovered base in turn: the scans over the bases (length + 1 values), over the bitmap words and
# over the regions (length / 2 + 1 flags) meet the scan's tile (2,048) and its first recursion edge (2,048^2)
ALTERNATING = (2047, 2048, 2049, 4095, 4096, 4097, 2 * SCAN_TILE * 64 - 1, 2 * SCAN_TILE * 64 + 1,
               SCAN_TILE * SCAN_TILE - 1, SCAN_TILE * SCAN_TILE + 1, 2 * SCAN_TILE * SCAN_TILE + 131)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALTERNATING)
def test_alternating_bases(ctx, n):
    st = np.arange(1, n, 2, dtype=np.int64)                 # bases 1, 3, 5 .. are covered
    un = np.zeros(st.size, np.int64)
    univ, a, b, ua, per = _device(ctx, [n], un, st, st + 1)
    want = np.arange(0, n, 2, dtype=np.int64)
    assert np.array_equal(a, want) and np.array_equal(b, want + 1) and not univ.any() and (ua == 1).all()
    assert per.tolist() == [[want.size, want.size, 1]]
    if n == ALTERNATING[0]:
        _assert_equal((univ, a, b, ua, per), model_uncovered([n], un, st, st + 1), "alternating")
    if n == ALTERNATING[-1]:
        assert want.size + 1 > SCAN_TILE * SCAN_TILE         # the flags' scan recurses twice


@functools.lru_cache(maxsize=None)
def _random_case(seed):
    """About 10^6 bases in a few hundred sequences (empty ones among them), random overlapping rows, N runs."""
    rng = np.random.default_rng(seed)
    nseq = int(rng.integers(200, 400))
    lengths = rng.integers(1, 2 * 1_000_000 // nseq, size=nseq)
    lengths[rng.choice(nseq, size=10, replace=False)] = 0
    lengths[rng.choice(nseq, size=5, replace=False)] = rng.integers(1, 130, size=5)
    total = int(lengths.sum())
    b = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=total)
    for a in rng.integers(0, total, size=300):
        b[a:a + int(rng.integers(1, 400))] = ord("N")
    b[rng.integers(0, total, size=2000)] = rng.choice(np.frombuffer(b"RYKMacgtn", dtype=np.uint8), size=2000)
    off = np.concatenate(([0], np.cumsum(lengths)))
    text = b.tobytes().decode("latin-1")
    seqs = [text[off[u]:off[u + 1]] for u in range(nseq)]
    nrows = 6000
    un = np.sort(rng.choice(np.flatnonzero(lengths > 0), size=nrows))
    st = (rng.random(nrows) * lengths[un]).astype(np.int64)
    en = np.minimum(st + 1 + rng.geometric(1 / 150.0, size=nrows), lengths[un])
    order = np.lexsort((st, un))
    return lengths, un[order], st[order], en[order], seqs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", (101, 202, 303))
def test_random_tables_and_the_union_invariant(ctx, seed):
    """Three seeded tables against the restatement, at several depths and filters; and at (1, 1, 0) the uncovered
    bases of every universe are its length minus union_len of catchhip_rows_stats."""
    from catch_amd import engine
    lengths, un, st, en, seqs = _random_case(seed)
    assert 500_000 < lengths.sum() < 1_500_000 and 200 <= lengths.size < 400
    for kw in (dict(), dict(min_depth=2), dict(min_depth=3, min_length=40, min_unambig=35), dict(min_unambig=0)):
        got = _device(ctx, lengths, un, st, en, seqs, **kw)
        _assert_equal(got, model_uncovered(lengths, un, st, en, seqs, **kw), (seed, kw))
        assert got[0].size > 100
    rows = engine.Rows.from_host(ctx, np.arange(un.size), un, st, en, lengths)
    try:
        per = rows.uncovered(None, 1, 1, 0)[4]
        _total_len, union_len, _per_set = rows.stats(lengths.size)
    finally:
        rows.close()
    assert np.array_equal(per[:, 1], np.asarray(lengths) - union_len) and int(union_len.sum()) > 100_000


@pytest.mark.gpu
def test_refusals(ctx):
    """min_depth 0, min_length 0, a negative min_unambig and targets of another shape: CATCHHIP_EINVAL with a
    message.  (Deferred rows are refused first of all, but no caller ever holds one: see the module's docstring.)"""
    from catch_amd import engine
    rows = engine.Rows.from_host(ctx, [0], [0], [2], [9], [20, 10])
    try:
        for kw, what in ((dict(min_depth=0), "min_depth 0"), (dict(min_length=0), "min_length 0"),
                         (dict(min_unambig=-1), "min_unambig -1"), (dict(min_depth=-3), "min_depth -3")):
            with pytest.raises(ValueError, match="rows_uncovered: .*" + what):
                rows.uncovered(None, **kw)
        for seqs in (["ACGT" * 5, "ACGT" * 2 + "AC", "A"],           # one sequence more
                     ["ACGT" * 5],                                   # one fewer
                     ["ACGT" * 4, "ACGT" * 3 + "AC"],                # the same total, other offsets
                     ["ACGT" * 5, "ACGT" * 3]):                      # another total
            t = HostTargets(ctx, seqs)
            try:
                with pytest.raises(ValueError, match="rows_uncovered: the targets .* are not one genome per sequence"):
                    rows.uncovered(t)
            finally:
                t.close()
        # two sequences of ONE genome over the same bases: not one genome per sequence
        two = engine.Targets(ctx, [["ACGT" * 5, "ACGT" * 2 + "AC"]])
        try:
            with pytest.raises(ValueError, match="rows_uncovered: the targets"):
                rows.uncovered(two)
        finally:
            two.close()
        # the raw entry: -1, no table handed out
        from catch_amd._lib import c_i64p
        h, n = ctypes.c_void_p(), ctypes.c_int64(7)
        per = np.zeros(6, np.int64)
        rc = ctx._L.catchhip_rows_uncovered(ctx._h, rows._h, None, 0, 1, 1, ctypes.byref(h), ctypes.byref(n),
                                            per.ctypes.data_as(c_i64p))
        assert rc == -1 and not h.value and n.value == 0
        # and the table is still good
        assert rows.uncovered()[1].tolist() == [0, 9, 0]
        assert rows.last_uncovered_ms > 0 and rows.last_uncovered_launches >= 8
    finally:
        rows.close()


# ------------------------------------------------------------------ the analyzer and the commands
def _write_fasta(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _ebola(n):
    from catch_amd.utils import seq_io
    return list(seq_io.read_fasta(EBOLA).items())[:n]


@functools.lru_cache(maxsize=1)
def _ebola_design():
    """Probes designed for the first 3 Ebola genomes (at 90% coverage, so that they leave gaps even there)."""
    from catch_amd import genome
    from catch_amd.filter import duplicate_filter, probe_designer, set_cover_filter
    recs = _ebola(5)
    np.random.seed(4)
    pb = probe_designer.ProbeDesigner(
        [[genome.Genome.from_one_seq(s) for _h, s in recs[:3]]],
        [duplicate_filter.DuplicateFilter(),
         set_cover_filter.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=0.9)],
        probe_length=100, probe_stride=50)
    pb.design()
    return recs, list(pb.final_probes)


def _host_complement(analyzer, min_depth):
    """The regions from target_covers on the host: per genome the depth by difference array over the genome's
    coordinates, runs cut at the chromosome boundaries."""
    out = {}
    for i, j, gnm, rc in analyzer._iter_target_genomes():
        covers = analyzer.target_covers[i][j][rc]
        lengths = [len(s) for s in gnm.seqs]
        seqs = [s[::-1].translate(str.maketrans("ACGT", "TGCA")) if rc else s for s in gnm.seqs]
        arr = np.asarray(covers, dtype=np.int64).reshape(-1, 2)
        # (a cover range lies inside one chromosome: as one universe each, in genome coordinates)
        off = np.concatenate(([0], np.cumsum(lengths)))
        un = np.searchsorted(off, arr[:, 0], side="right") - 1
        univ, st, en, ua, _per = model_uncovered(lengths, un, arr[:, 0] - off[un], arr[:, 1] - off[un], seqs,
                                                 min_depth=min_depth)
        out.setdefault(i, {}).setdefault(j, {})[rc] = list(zip(univ.tolist(), st.tolist(), en.tolist(), ua.tolist()))
    return out


@pytest.mark.gpu
def test_analyzer_equals_the_complement_of_target_covers(ctx, monkeypatch):
    """Probes designed for 3 Ebola genomes analysed against 5, both strands: uncovered_regions() at depth 1 and 2
    equals the complement of target_covers computed on the host; the summary adds up; nothing but the regions is
    fetched."""
    from catch_amd import coverage_analysis, engine, genome
    recs, probes = _ebola_design()
    gens = [[genome.Genome.from_one_seq(s) for _h, s in recs]]
    a = coverage_analysis.Analyzer(probes, 2, 100, gens, ["ebola"])
    a.run()
    fetched = []
    real_fetch = engine.Rows.fetch
    monkeypatch.setattr(engine.Rows, "fetch", lambda self: (fetched.append(self.n), real_fetch(self))[1])
    got1 = a.uncovered_regions()
    summary1 = a.uncovered_summary
    got2 = a.uncovered_regions(min_depth=2)
    nregions = [sum(len(got[0][j][rc]) for j in range(5) for rc in (False, True)) for got in (got1, got2)]
    assert sorted(fetched) == sorted([sum(len(got[0][j][rc]) for j in range(5)) for got in (got1, got2)
                                      for rc in (False, True)])       # four fetches, of the regions only
    monkeypatch.setattr(engine.Rows, "fetch", real_fetch)
    assert got1 == _host_complement(a, 1)
    assert got2 == _host_complement(a, 2)
    bases = [sum(b - x for j in range(5) for rc in (False, True) for _s, x, b, _u in got[0][j][rc])
             for got in (got1, got2)]
    assert nregions[0] > 5 and bases[1] > bases[0] > 0
    for j in range(5):
        for rc in (False, True):
            regs = got1[0][j][rc]
            assert summary1[0][j][rc] == (len(regs), sum(b - x for _s, x, b, _u in regs),
                                          max([b - x for _s, x, b, _u in regs] + [0]))
            assert sum(b - x for _s, x, b, _u in a.uncovered_regions(1, 1, 0)[0][j][rc]) == \
                gens[0][j].size(False) - a.bp_covered[0][j][rc]
    # the genomes the probes were not designed for have more to fill
    assert sum(summary1[0][j][False][1] for j in (3, 4)) > 0


@pytest.mark.gpu
def test_analyzer_chromosomes_names_and_no_probes(ctx, tmp_path):
    """A genome of two named chromosomes: the Sequence column carries the names, no region crosses from one
    chromosome into the next, rc coordinates are those of the reverse-complemented sequence.  Without probes every
    non-empty sequence is one region."""
    from catch_amd import coverage_analysis, genome, probe
    rng = np.random.default_rng(12)
    c1 = "".join(rng.choice(list("ACGT"), size=700))
    c2 = "".join(rng.choice(list("ACGT"), size=530))
    single = "".join(rng.choice(list("ACGT"), size=400))
    g = genome.Genome.from_chrs({"chrA": c1, "chrB": c2})
    groups = [[g, genome.Genome.from_one_seq(single)]]
    # probes that cover chrA's [100, 300) and [350, 600) and chrB's [100, 430): the end of chrA and the start of chrB
    # are both uncovered
    # and one probe from the other strand: chrA's [350, 450) there, [250, 350) of the reverse complement
    other = c1[350:450][::-1].translate(str.maketrans("ACGT", "TGCA"))
    probes = [probe.Probe.from_str(s) for s in (c1[100:200], c1[200:300], c1[350:450], c1[450:550], c1[500:600],
                                                c2[100:200], c2[200:300], c2[300:400], c2[330:430], other)]
    a = coverage_analysis.Analyzer(probes, 0, 100, groups, ["two"])
    a.run()
    regs = a.uncovered_regions()
    assert regs[0][0][False] == [(0, 0, 100, 100), (0, 300, 350, 50), (0, 600, 700, 100), (1, 0, 100, 100),
                                 (1, 430, 530, 100)]
    assert regs[0][0][True] == [(0, 0, 250, 250), (0, 350, 700, 350), (1, 0, 530, 530)]
    assert regs[0][1][False] == [(0, 0, 400, 400)] and a.uncovered_summary[0][0][False] == (5, 450, 100)
    assert regs == _host_complement(a, 1)
    fn, fa = str(tmp_path / "r.tsv"), str(tmp_path / "r.fasta")
    a.write_uncovered_regions(fn)
    a.write_uncovered_fasta(fa)
    lines = [ln.split("\t") for ln in open(fn).read().splitlines()]
    assert lines[0] == ["Genome", "Sequence", "Start", "End", "Length", "Unambig bases"]
    assert lines[1:6] == [["two, genome 0", "chrA", "0", "100", "100", "100"],
                          ["two, genome 0", "chrA", "300", "350", "50", "50"],
                          ["two, genome 0", "chrA", "600", "700", "100", "100"],
                          ["two, genome 0", "chrB", "0", "100", "100", "100"],
                          ["two, genome 0", "chrB", "430", "530", "100", "100"]]
    assert lines[6:9] == [["two, genome 0 (rc)", "chrA", "0", "250", "250", "250"],
                          ["two, genome 0 (rc)", "chrA", "350", "700", "350", "350"],
                          ["two, genome 0 (rc)", "chrB", "0", "530", "530", "530"]]
    assert lines[9:] == [["two, genome 1", "0", "0", "400", "400", "400"],
                         ["two, genome 1 (rc)", "0", "0", "400", "400", "400"]]
    text = open(fa).read().splitlines()
    assert text[:2] == [">two, genome 0|chrA|0-100", c1[:100]] and text[6:8] == [">two, genome 0|chrB|0-100", c2[:100]]
    assert text[10:] == [">two, genome 1|0|0-400", single] and not any("(rc)" in ln for ln in text)
    # no probes
    withn = genome.Genome.from_chrs({"x": "ACGTN" * 20, "y": "N" * 50, "z": "ACG"})
    b = coverage_analysis.Analyzer([], 0, 100, [[withn]], ["none"])
    b.run()
    assert b.uncovered_regions()[0][0] == {False: [(0, 0, 100, 80), (2, 0, 3, 3)], True: [(0, 0, 100, 80), (2, 0, 3, 3)]}
    assert b.uncovered_regions(min_unambig=0)[0][0][False] == [(0, 0, 100, 80), (1, 0, 50, 0), (2, 0, 3, 3)]
    assert b.uncovered_summary[0][0][True] == (3, 153, 100)


def _read_regions_tsv(fn):
    lines = open(fn).read().splitlines()
    assert lines[0] == "Genome\tSequence\tStart\tEnd\tLength\tUnambig bases"
    return [ln.split("\t") for ln in lines[1:]]


def _library_rows(a, *filters):
    regs = a.uncovered_regions(*filters)
    return [[a._row_header(i, j, rc), str(s), str(x), str(b), str(b - x), str(u)]
            for i, j, _gnm, rc in a._iter_target_genomes() for s, x, b, u in regs[i][j][rc]]


@pytest.mark.gpu
def test_analyze_probe_coverage_writes_the_regions(ctx, tmp_path, capsys, caplog):
    """analyze_probe_coverage --write-uncovered-regions --write-uncovered-fasta: the file's rows are the
    library's, every FASTA record is the slice its header names; --print-analysis prints what it printed without
    the options; two datasets under --params come out in -d order and equal each dataset analysed alone."""
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd.utils import seq_io
    recs, probes = _ebola_design()
    pf = _write_fasta(tmp_path / "probes.fasta", [("p%d" % i, p.seq_str) for i, p in enumerate(probes)])
    d1 = _write_fasta(tmp_path / "first.fasta", recs[:2])
    d2 = _write_fasta(tmp_path / "second.fasta", recs[3:5])
    tsv, fa = str(tmp_path / "r.tsv"), str(tmp_path / "r.fasta")
    base = ["-d", d2, "-f", pf, "-m", "2", "-l", "100", "--print-analysis"]
    capsys.readouterr()
    apc.main(apc.parse_args(base))
    plain_report = capsys.readouterr().out
    with caplog.at_level(logging.INFO, logger="catch_amd.coverage_analysis"):
        (a,) = apc.main(apc.parse_args(base + ["--write-uncovered-regions", tsv, "--write-uncovered-fasta", fa,
                                               "--uncovered-min-length", "20"]))
    assert capsys.readouterr().out == plain_report and "NUMBER OF PROBES" in plain_report
    assert any(re.search(r"second\.fasta: \d+ uncovered regions, \d+ uncovered bases, longest \d+", r.getMessage())
               for r in caplog.records)
    rows = _read_regions_tsv(tsv)
    assert rows == _library_rows(a, 1, 20, 1) and len(rows) > 4
    assert all(int(r[4]) >= 20 and int(r[3]) - int(r[2]) == int(r[4]) for r in rows)
    assert [r[0] for r in rows if r[0].endswith("(rc)")]
    genomes = seq_io.read_genomes_from_fasta(d2)
    records = open(fa).read().split(">")[1:]
    assert len(records) == sum(1 for r in rows if not r[0].endswith("(rc)"))
    for rec, row in zip(records, [r for r in rows if not r[0].endswith("(rc)")]):
        head, seq = rec.rstrip("\n").split("\n")
        name, s, span = head.split("|")
        x, b = (int(v) for v in span.split("-"))
        j = int(re.match(r"second\.fasta, genome (\d+)$", name).group(1))
        assert seq == genomes[j].seqs[int(s)][x:b] and [name, s, str(x), str(b)] == row[:4]

    # --params: each dataset under its own row
    params = tmp_path / "params.tsv"
    params.write_text("dataset\tmismatches\tcover_extension\nfirst\t1\t0\nsecond\t3\t20\n")
    both = str(tmp_path / "both.tsv"), str(tmp_path / "both.fasta")
    apc.main(apc.parse_args(["-d", d2, d1, "-f", pf, "-l", "100", "--params", str(params),
                             "--write-uncovered-regions", both[0], "--write-uncovered-fasta", both[1]]))
    want_tsv, want_fa = [], ""
    for d, m, e in ((d2, 3, 20), (d1, 1, 0)):
        one = str(tmp_path / "one.tsv"), str(tmp_path / "one.fasta")
        apc.main(apc.parse_args(["-d", d, "-f", pf, "-l", "100", "-m", str(m), "-e", str(e),
                                 "--write-uncovered-regions", one[0], "--write-uncovered-fasta", one[1]]))
        want_tsv += _read_regions_tsv(one[0])
        want_fa += open(one[1]).read()
    assert _read_regions_tsv(both[0]) == want_tsv and open(both[1]).read() == want_fa
    names = [r[0].split(",")[0] for r in want_tsv]
    assert names == sorted(names, reverse=True) and set(names) == {"first.fasta", "second.fasta"}


@pytest.mark.gpu
def test_design_writes_the_regions_and_designs_the_same(ctx, tmp_path, capsys):
    """design -c 0.9 --write-uncovered-regions writes the file; its -o output is byte-identical to the same design
    without the option; --print-analysis prints the same with and without the new options."""
    from catch_amd import design
    fa = _write_fasta(tmp_path / "three.fasta", _ebola(3))
    base = [fa, "-pl", "100", "-ps", "50", "-m", "2", "-c", "0.9", "--print-analysis"]
    out = [str(tmp_path / n) for n in ("plain.fasta", "with.fasta", "r.tsv", "r.fasta")]
    capsys.readouterr()
    np.random.seed(1)
    design.main(design.parse_args(base + ["-o", out[0]]))
    plain_report = capsys.readouterr().out
    np.random.seed(1)
    design.main(design.parse_args(base + ["-o", out[1], "--write-uncovered-regions", out[2],
                                          "--write-uncovered-fasta", out[3], "--uncovered-keep-ambiguous"]))
    assert capsys.readouterr().out == plain_report and "NUMBER OF PROBES" in plain_report
    assert open(out[0], "rb").read() == open(out[1], "rb").read() and os.path.getsize(out[0]) > 1000
    rows = _read_regions_tsv(out[2])
    assert len(rows) > 3 and {r[0] for r in rows} <= {"three.fasta, genome %d" % j for j in range(3)}
    assert sum(int(r[4]) for r in rows) > 0 and open(out[3]).read().count(">") == len(rows)
    # without an analysis option the write option alone triggers the analysis (and the count is not printed)
    np.random.seed(1)
    design.main(design.parse_args(base[:-1] + ["-o", out[1], "--write-uncovered-regions", out[2]]))
    assert capsys.readouterr().out == ""
    assert [r for r in _read_regions_tsv(out[2])] == [r for r in rows if int(r[5]) >= 1]
