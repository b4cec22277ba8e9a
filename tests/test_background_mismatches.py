"""--background-mismatches M: the background screen counts a k-mer of a candidate when a background k-mer, either
strand, lies within M substitutions of it (M in 0 .. 2, K >= 8 (M + 1); catch_amd/filter/background_filter.py has the
rule, three times).  Here: the worked values of the rule against the definition, NumPy (views, np.searchsorted, a loop
inside the ranges) against the definition on small inputs, the refusals and the option surface; then, on the GPU, the
views of the index against Python integers, the tolerant kernel (background_flag_tolerant_kernel and the hits family of
measure_rows_kernel) against NumPy, and the design commands on both front ends.

The definition is pure Python -- every position against every background word -- so its runs are small: candidates of
at most 40 characters, backgrounds of a few hundred k-mers.  NumPy, once it equals the definition, is the yardstick of
the kernel at the lengths the kernel test uses.

The worked table is given at K = 16 for M = 0, 1 and 2, and the class refuses K = 16 with M = 2 (K >= 24): the M = 2
column is checked through the definition alone (_hits takes another M than the filter's: it needs no blocks), and the
refusal is asserted next to it."""
import contextlib
import ctypes
import functools
import gzip
import io
import logging
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
GRID_BASE = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", "out"]
COMP = str.maketrans("ACGT", "TGCA")
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
LETTER = "ACTG"
KM = [(16, 1), (17, 1), (24, 2), (25, 2), (26, 2), (31, 1), (32, 1), (32, 2)]

WORKED_BACKGROUND = "GATTACAGATTACCAGGTCATGCA"
WORKED = [("TTACAGATTACCAGGTCATG", (5, 5, 5)),         # background[2:22]
          ("TTACAGATTTCCAGGTCATG", (0, 5, 5)),         # one substitution at index 9
          ("CATGAACTGGTAATCTGTAA", (0, 5, 5)),         # reverse complement of the first, one substitution at index 5
          ("TTACCGATTACCAAGTCATG", (0, 0, 5)),         # substitutions at indices 4 and 13
          ("TTACAGATTNCCAGGTCATG", (0, 0, 0))]         # N at index 9: no valid 16-mer


def BF(*a, **k):
    from catch_amd.filter.background_filter import BackgroundFilter
    return BackgroundFilter(*a, **k)


def _rc(s):
    return s.translate(COMP)[::-1]


def _random_bases(rng, n, n_rate=0.0):
    s = "".join(rng.choice(list("ACGT"), size=n))
    if n_rate:
        s = "".join("N" if x else c for c, x in zip(s, (rng.random(n) < n_rate).tolist()))
        while "NN" in s:                # (two adjacent Ns end a window of the candidate generator)
            s = s.replace("NN", "NA")
    return s


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


def _starts(K, M):
    return [b * K // (M + 1) for b in range(M + 2)]


def _rotl(x, bits, K):
    return ((x << bits) | (x >> (2 * K - bits))) & ((1 << (2 * K)) - 1) if bits else x


def _decode(code, K):
    return "".join(LETTER[(code >> (2 * (K - 1 - t))) & 3] for t in range(K))


def _substitute(s, where, step=1):
    s = list(s)
    for p in where:
        s[p] = "ACGT"[("ACGT".index(s[p]) + step) % 4]
    return "".join(s)


def _definition(f, strs):
    """(keep list, dropped, histogram) straight from _hits, string by string."""
    hits = [f._hits(s) for s in strs]
    hist = [0] * 256
    for s, h in zip(strs, hits):
        if len(s) >= f.kmer:
            hist[min(h, 255)] += 1
    keep = [f.max_hits is None or h <= f.max_hits for h in hits]
    return keep, keep.count(False), hist


# ------------------------------------------------------------------ host: the worked values
def test_worked_values():
    assert len(WORKED_BACKGROUND) == 24 and WORKED[0][0] == WORKED_BACKGROUND[2:22]
    assert WORKED[1][0] == _substitute(WORKED[0][0], [9], 3) and WORKED[3][0] != WORKED[0][0]
    assert sum(a != b for a, b in zip(WORKED[2][0], _rc(WORKED[0][0]))) == 1 and WORKED[2][0][5] != _rc(WORKED[0][0])[5]
    assert [i for i in range(20) if WORKED[3][0][i] != WORKED[0][0][i]] == [4, 13]
    strs = [s for s, _ in WORKED]
    for M in (0, 1):
        f = BF([WORKED_BACKGROUND], kmer=16, max_hits=0, mismatches=M)
        assert [f._hits(s) for s in strs] == [h[M] for _, h in WORKED], M
        assert f._filter_strs(strs) == [s for s, h in WORKED if h[M] == 0], M
        assert f.dropped == sum(1 for _, h in WORKED if h[M]) and f.histogram[0] + f.histogram[5] == 5
        assert f.histogram[5] == f.dropped
    # M = 2 needs K >= 24: the class refuses K = 16, the definition does not need the blocks
    with pytest.raises(ValueError):
        BF([WORKED_BACKGROUND], kmer=16, max_hits=0, mismatches=2)
    f = BF([WORKED_BACKGROUND], kmer=16, max_hits=0)
    for M in (0, 1, 2):
        assert [f._hits(s, mismatches=M) for s in strs] == [h[M] for _, h in WORKED], M


# ------------------------------------------------------------------ host: NumPy against the definition
@functools.lru_cache(maxsize=None)
def _small_case(K, M):
    """(records, {L: candidates}) for the comparison with the definition: records of 70 and 45 bases, one shorter than
    K, one with an N and, for even K, a palindromic k-mer; candidates of L = K, K + 1 and 40 cut around k-mers of the
    background with 0 .. M + 1 substitutions, as they are and reverse-complemented -- at the first and at the last
    character of every block; all M inside one block; one in each of M blocks, for each choice of the block left
    alone; one in every block (no block is left) -- then random ones, ones with N, lower case and the palindrome."""
    rng = np.random.default_rng(100 * K + M)
    a, b = _random_bases(rng, 70), _random_bases(rng, 45)
    b = b[:K + 3] + "N" + b[K + 4:]
    records = [a, b, _random_bases(rng, K - 1)]
    pal = None
    if K % 2 == 0:
        half = _random_bases(rng, K // 2)
        pal = half + _rc(half)
        records.append(pal)
    s = _starts(K, M)
    blocks = [(s[i], s[i + 1] - 1) for i in range(M + 1)]
    sets = [[]]
    for first, last in blocks:
        sets += [[first], [last]]
        if M == 2:
            sets.append([first, last])                                   # all M inside one block
    mid = [(first + last) // 2 for first, last in blocks]
    for left in range(M + 1):                                            # only block `left` can find the match
        sets.append([mid[j] for j in range(M + 1) if j != left])
        sets.append([blocks[j][0] for j in range(M + 1) if j != left])
    sets.append(mid)                                                     # M + 1 substitutions, one per block
    by_length = {}
    for L in (K, K + 1, 40):
        out = []
        for n, at in enumerate((3, 30)):
            w = a[at:at + K]
            for where in sets:
                v = _substitute(w, where, 1 + n)
                for strand in (v, _rc(v)):
                    lead = int(rng.integers(0, L - K + 1))
                    out.append(_random_bases(rng, lead) + strand + _random_bases(rng, L - K - lead))
        out += [_random_bases(rng, L) for _ in range(12)]
        out += [a[5:5 + L], _rc(a[7:7 + L]), a[5:5 + L].lower(), a[5:5 + L // 2] + "N" + a[6 + L // 2:5 + L]]
        out.append(b[:L] if len(b) >= L else b[:K + 3].ljust(L, "A"))   # runs into the record's N
        if pal:
            out.append((pal + _random_bases(rng, L - K))[:L])
        out += out[:5]                                                   # duplicates are counted
        assert all(len(x) == L for x in out)
        by_length[L] = out
    return records, by_length


@pytest.mark.parametrize("K,M", KM)
def test_numpy_rule_equals_definition(K, M):
    records, by_length = _small_case(K, M)
    assert any(len(r) < K for r in records) and any("N" in r for r in records)
    mixed = []
    for L, strs in by_length.items():
        oracle = BF(records, kmer=K, mismatches=M)
        hits = [oracle._hits(x) for x in strs]
        exact = [oracle._hits(x, mismatches=0) for x in strs]
        below = [oracle._hits(x, mismatches=M - 1) for x in strs]
        # the budget matters: candidates that hit at M and not at M - 1, ones that hit at 0, ones that never hit
        assert any(h and not e for h, e in zip(hits, below)) and any(exact) and hits.count(0) > 5, (K, M, L)
        assert all(h >= e for h, e in zip(hits, below)) and all(h >= e for h, e in zip(below, exact))
        assert oracle._hits_equal_length(strs, L).tolist() == hits, (K, M, L)
        for H in (0, 1, None):
            f = BF(records, kmer=K, max_hits=H, mismatches=M)
            keep, dropped, hist = _definition(f, strs)
            assert f._filter_strs(strs) == [x for x, k in zip(strs, keep) if k], (K, M, L, H)
            assert f.dropped == dropped and f.histogram == hist and sum(hist) == len(strs)
            assert (dropped > 0) == (H is not None and H <= L - K)
        mixed += strs[::3]
    # mixed lengths in one call, strings below K among them: the order is kept, the short ones count nothing
    mixed += ["", "ACGT", records[0][:K - 1]]
    random.Random(K + M).shuffle(mixed)
    f = BF(records, kmer=K, max_hits=0, mismatches=M)
    keep, dropped, hist = _definition(f, mixed)
    assert f._filter_strs(mixed) == [x for x, k in zip(mixed, keep) if k]
    assert f.dropped == dropped > 0 and f.histogram == hist and sum(hist) == len(mixed) - 3


def test_zero_mismatches_is_the_filter_without_the_keyword():
    K = 16
    records, by_length = _small_case(K, 1)
    strs = by_length[40] + by_length[K]
    for H in (0, 2, None):
        f, g = BF(records, kmer=K, max_hits=H), BF(records, kmer=K, max_hits=H, mismatches=0)
        assert g.mismatches == f.mismatches == 0
        assert f._filter_strs(strs) == g._filter_strs(strs)
        assert (f.dropped, f.histogram) == (g.dropped, g.histogram) and sum(f.histogram) == len(strs)
        assert [f._hits(s) for s in strs[:20]] == [g._hits(s) for s in strs[:20]] and g._views is None
        assert f.summary() == g.summary() and "mismatch" not in g.summary()
    assert "within 1 mismatches" in BF(records, kmer=K, mismatches=1).summary()


@pytest.mark.parametrize("K,M", KM)
def test_hits_never_fall_when_the_budget_rises(K, M):
    records, by_length = _small_case(K, M)
    for L, strs in by_length.items():
        at = [BF(records, kmer=K, mismatches=m)._hits_equal_length(strs, L) for m in range(M + 1)]
        for m in range(1, M + 1):
            assert (at[m] >= at[m - 1]).all() and (at[m] > at[m - 1]).any(), (K, M, L, m)


# ------------------------------------------------------------------ host: refusals and the option surface
def test_refusals(capsys):
    from catch_amd import design, design_grid, probe_report
    for bad in (dict(kmer=24, mismatches=3), dict(kmer=24, mismatches=-1), dict(kmer=24, mismatches=1.0),
                dict(kmer=24, mismatches=True), dict(kmer=23, mismatches=2), dict(kmer=15, mismatches=1),
                dict(kmer=8, mismatches=1)):
        with pytest.raises(ValueError):
            BF(["ACGT" * 10], **bad)
    assert BF(["ACGT" * 10], kmer=24, mismatches=2).mismatches == 2 and BF(["ACGT" * 10], kmer=16, mismatches=1).kmer == 16
    on = ["--background", "h.fa", "--background-max-hits", "0"]
    parsers = ((design.parse_args, ["x.fasta"], True), (design_grid.parse_args, GRID_BASE, True),
               (probe_report.parse_args, ["-f", "p.fasta"], False))
    for parse, base, designs in parsers:
        assert parse(base).background_mismatches is None
        a = parse(base + on + ["--background-kmer", "32", "--background-mismatches", "2"])
        assert (a.background_kmer, a.background_mismatches) == (32, 2)
        assert parse(base + on + ["--background-mismatches", "2"]).background_mismatches == 2         # K = 24 by default
        assert parse(base + on + ["--background-kmer", "16", "--background-mismatches", "1"]).background_mismatches == 1
        assert parse(base + on + ["--background-mismatches", "0", "--background-kmer", "8"]).background_mismatches == 0
        if designs:           # (the report writes every probe's value and has no histogram option)
            a = parse(base + ["--background", "h.fa", "--write-background-histogram", "h.tsv", "--background-mismatches", "1"])
            assert a.background_mismatches == 1 and a.background_max_hits is None
        for bad, words in ((on + ["--background-mismatches", "3"], ()), (on + ["--background-mismatches", "-1"], ()),
                           (on + ["--background-kmer", "23", "--background-mismatches", "2"], ("23", "24")),
                           (on + ["--background-kmer", "15", "--background-mismatches", "1"], ("15", "16")),
                           (on + ["--background-mismatches", "x"], ()), (["--background-mismatches", "1"], ("--background",))):
            with pytest.raises(SystemExit):
                parse(base + bad)
            err = capsys.readouterr().err
            assert "error:" in err and all(w in err for w in words), (bad, err)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        design.parse_args(["--help"])
    assert "--background-mismatches M" in " ".join(buf.getvalue().split())


def test_judge_and_filter_carry_the_budget(tmp_path):
    from catch_amd import design, probe_report
    from catch_amd.filter import background_filter
    bg = tmp_path / "bg.fasta"
    bg.write_text(">h\n%s\n" % WORKED_BACKGROUND)
    args = design.parse_args(["x.fasta", "--background", str(bg), "--background-kmer", "16", "--background-max-hits", "0",
                              "--background-mismatches", "1"])
    f = background_filter.from_args(args)
    assert (f.kmer, f.max_hits, f.mismatches) == (16, 0, 1) and f.background_seqs == [WORKED_BACKGROUND]
    judge = probe_report.Judge(args)
    assert judge.background.mismatches == 1 and judge.background.kmer == 16
    args = probe_report.parse_args(["-f", "p.fasta", "--background", str(bg), "--background-kmer", "16",
                                    "--background-mismatches", "1"])
    assert probe_report.Judge(args).background.mismatches == 1
    assert probe_report.Judge(probe_report.parse_args(["-f", "p.fasta", "--background", str(bg)])).background.mismatches == 0


def test_symbols_declared_and_bound():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name, nargs in (("catchhip_kmer_index_create_tolerant", 9), ("catchhip_kmer_index_fetch_view", 4)):
        at = re.search(r"\b%s\s*\(" % name, hdr)
        assert at, name
        assert "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1], name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
    assert hasattr(engine.KmerIndex, "fetch_view")
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert re.search(r"background\.o[^\n]*measure\.o[^\n]*: kmer_lookup\.h", mk)


# ------------------------------------------------------------------ GPU: the views against Python integers
def _view_backgrounds(K):
    rng = np.random.default_rng(70 + K)
    big = list(_random_bases(rng, 9000))
    for at, ln in ((100, 1), (3000, K - 1), (6000, 2 * K)):
        big[at:at + ln] = "N" * ln
    big = "".join(big)
    return {"three records": [big[:5000], big[5000:5000 + K - 1], big[5000 + K - 1:]],
            "no valid k-mer": [big[:K - 1], "ACGTN" * 20, ""],
            "k bases": [big[200:200 + K]],
            "one code": ["A" * 300]}


@pytest.mark.gpu
@pytest.mark.parametrize("K,M", KM)
def test_views_equal_python_integers(ctx, K, M):
    from catch_amd import engine
    starts = _starts(K, M)
    for name, records in _view_backgrounds(K).items():
        codes = _canonical_codes(records, K)
        distinct = sorted(set(codes))
        exact = engine.KmerIndex(ctx, records, K)
        index = engine.KmerIndex(ctx, records, K, mismatches=M)
        try:
            assert (index.mismatches, index.k, exact.mismatches) == (M, K, 0)
            assert (index.n_valid, index.n_unique) == (exact.n_valid, exact.n_unique) == (len(codes), len(distinct)), name
            assert index.fetch().tolist() == exact.fetch().tolist() == index.fetch_view(0).tolist() == distinct, name
            for b in range(1, M + 1):
                got = index.fetch_view(b)
                assert got.dtype == np.uint64 and got.tolist() == sorted(_rotl(c, 2 * starts[b], K) for c in distinct), (name, b)
            with pytest.raises(ValueError, match="kmer_index_fetch_view: the index has the views 0 .. %d" % M):
                index.fetch_view(M + 1)
            with pytest.raises(ValueError, match="kmer_index_fetch_view"):
                exact.fetch_view(1)
            assert exact.fetch_view(0).tolist() == distinct
        finally:
            index.close()
            exact.close()
        assert {"no valid k-mer": 0, "k bases": 1, "one code": 1}.get(name, len(distinct)) == len(distinct) and (
            name != "three records" or len(distinct) > 8000)


@pytest.mark.gpu
def test_index_refusals_and_the_c_entry_with_zero_mismatches(ctx):
    from catch_amd import engine
    records = ["ACGT" * 20]
    with pytest.raises(ValueError, match="kmer_index_create: mismatches must lie in 0 .. 2"):
        engine.KmerIndex(ctx, records, 24, mismatches=3)
    with pytest.raises(ValueError, match="kmer_index_create: mismatches must lie in 0 .. 2"):
        engine.KmerIndex(ctx, records, 24, mismatches=-1)
    with pytest.raises(ValueError, match="kmer_index_create: 1 mismatches need k >= 16"):
        engine.KmerIndex(ctx, records, 15, mismatches=1)
    with pytest.raises(ValueError, match="kmer_index_create: 2 mismatches need k >= 24"):
        engine.KmerIndex(ctx, records, 23, mismatches=2)
    with pytest.raises(ValueError, match="kmer_index_create: k must lie in 8 .. 32"):
        engine.KmerIndex(ctx, records, 33, mismatches=1)
    # the new entry with mismatches = 0 (engine goes through the old one then): the exact index
    rng = np.random.default_rng(5)
    records = [_random_bases(rng, 4000, 0.002), _random_bases(rng, 10)]
    buf = np.frombuffer("".join(records).encode(), dtype=np.uint8).copy()
    off = np.array([0, 4000, 4010], dtype=np.int64)
    h, nv, nu = ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0)
    L = ctx._L
    rc = L.catchhip_kmer_index_create_tolerant(
        ctx._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2, 20, 0,
        ctypes.byref(h), ctypes.byref(nv), ctypes.byref(nu))
    assert rc == 0 and h
    try:
        want = sorted(set(_canonical_codes(records, 20)))
        out = np.zeros(nu.value, dtype=np.uint64)
        assert L.catchhip_kmer_index_fetch_view(ctx._h, h, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 0
        assert out.tolist() == want and nv.value == len(_canonical_codes(records, 20))
        assert L.catchhip_kmer_index_fetch_view(ctx._h, h, 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) != 0
    finally:
        L.catchhip_kmer_index_destroy(h)


# ------------------------------------------------------------------ GPU: the kernel against NumPy
def _background(seed, K):
    """Records: random bases with a few Ns, a palindrome of Gs and Cs (K = 32: a canonical code with the top bit set)
    and 150 k-mers that begin with AAAA (long buckets in view 0)."""
    rng = np.random.default_rng(seed)
    gc = "G" * (K // 2) + "C" * (K - K // 2)
    clustered = ["AAAA" + _random_bases(rng, K - 4) for _ in range(150)]
    return [_random_bases(rng, 3000, 0.003), "G" + _random_bases(rng, K + 5) + "C", gc, "N".join(clustered)]


def _planted(rng, n, records, K, every, rate):
    """n characters: random bases with isolated Ns and, about every `every` characters, a piece of a record, K .. K + 16
    long, forward or reverse-complemented, in which each base is substituted with probability `rate`."""
    s = list(_random_bases(rng, n, 0.004))
    at = int(rng.integers(0, every))
    while at + K + 16 < n:
        rec = records[0 if rng.random() < 0.5 else int(rng.integers(0, len(records)))]
        ln = min(K + int(rng.integers(0, 17)), len(rec))
        a = int(rng.integers(0, len(rec) - ln + 1))
        piece = rec[a:a + ln]
        if rng.random() < 0.5:
            piece = _rc(piece)
        piece = "".join("ACGT"[int(rng.integers(0, 4))] if c != "N" and rng.random() < rate else c for c in piece)
        s[at:at + ln] = piece
        at += ln + int(rng.integers(1, 2 * every))
    s = "".join(s)[:n]
    while "NN" in s:
        s = s.replace("NN", "NA")
    return s


def _targets(seed, L, stride, ncand, records, K):
    """Sequences whose windows give about ncand candidates, a good part of them more than once."""
    rng = np.random.default_rng(seed)
    every = max(L, 2 * K) if L - K >= 8 else K // 2
    s = _planted(rng, L + stride * (ncand - 1), records, K, every, 0.04)
    half = L + stride * (ncand // 2 + 3)
    return [s, s[:half], s[stride * (ncand // 3):]]


def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


def _expect(f, strs, mult, L):
    """(keep mask, dropped, histogram, hits) by the NumPy rule, multiplicities counted."""
    hits = np.concatenate([f._hits_equal_length(strs[a:a + 4096], L) for a in range(0, len(strs), 4096)])
    hist = np.zeros(256, dtype=np.int64)
    np.add.at(hist, np.minimum(hits, 255), mult.astype(np.int64))
    if f.max_hits is None:
        return np.ones(len(strs), dtype=bool), 0, hist.tolist(), hits
    keep = hits <= f.max_hits
    return keep, int(mult[~keep].sum()), hist.tolist(), hits


# (K, L, stride) as in tests/test_background_filter.py's KERNEL_CASES for the K that allows a budget: L = K and K + 1, the
# four shapes, the last length of one workgroup size and the first of the next (256 / 128 / 64 rows, then unstaged), and
# the unstaged kernel; M = 1 on all of them, M = 2 on both ends, both staged shapes of 256 and 128 rows, a tier edge and
# the unstaged one.  Other K (odd blocks) at L = 100.
SHAPES = [(64, 32), (100, 50), (130, 50), (300, 100)]
TIER_EDGES = [(225, 40), (226, 40), (465, 97), (466, 97), (961, 200), (962, 200)]
UNSTAGED = [(1000, 500)]
KERNEL_CASES = [(32, L, s, 1) for L, s in [(32, 1), (33, 1)] + SHAPES + TIER_EDGES + UNSTAGED]
KERNEL_CASES += [(32, L, s, 2) for L, s in [(32, 1), (100, 50), (300, 100), (466, 97), (1000, 500)]]
KERNEL_CASES += [(16, 100, 50, 1), (17, 100, 50, 1), (24, 100, 50, 2), (26, 100, 50, 2), (31, 100, 50, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,L,stride,M", KERNEL_CASES)
def test_tolerant_kernel_equals_numpy(ctx, K, L, stride, M):
    """catchhip_candidates_drop_background against a tolerant index, in the three settings: surviving positions,
    multiplicities and groups are the unfiltered list's, masked; `dropped` and all 256 bins equal NumPy's; and the hits
    of Candidates.measure are NumPy's, alone and next to the other families of the rows kernel."""
    from catch_amd import engine
    from catch_amd.filter.tm_filter import TmFilter
    records = _background(300 + K + M, K)
    seqs = _targets(4000 + 37 * K + L + M, L, stride, (1500 if L <= 40 else 500) if L < 400 else 200, records, K)
    concat = "".join(seqs)
    targets = engine.Targets(ctx, [[s] for s in seqs])
    index = engine.KmerIndex(ctx, records, K, mismatches=M)
    try:
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        n = len(strs0)
        assert mult0.max() > 1 and n % 64 != 0 and n > 128 and any("N" in s for s in strs0)
        oracle = BF(records, kmer=K, mismatches=M)
        _, _, _, hits = _expect(oracle, strs0, mult0, L)
        below = _expect(BF(records, kmer=K, mismatches=M - 1), strs0, mult0, L)[3]
        assert (hits >= below).all() and (hits > below).sum() > 0.03 * n, "the budget adds nothing here"
        # measure: the hits family alone, and with composition and Tm in the same kernel
        tm = TmFilter()
        got = base.measure(what="hits", index=index, values=True, histograms=False)
        assert got["hits"].astype(np.int64).tolist() == hits.tolist()
        got = base.measure(what=("composition", "tm", "hits"), tm=(tm._q(L), tm.offset_c), index=index, values=True)
        assert got["hits"].astype(np.int64).tolist() == hits.tolist()
        assert got["gc"].tolist() == [s.count("G") + s.count("C") for s in strs0]
        base.close()
        H = int(np.median(hits))
        assert hits.min() <= H < hits.max()
        for name, kwargs in (("filter + histogram", dict(max_hits=H)), ("filter only", dict(max_hits=H)),
                             ("histogram only", {})):
            f = BF(records, kmer=K, mismatches=M, **kwargs)
            keep, want, hist, _ = _expect(f, strs0, mult0, L)
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
                    print(name, K, L, M, n, "kept", c.n, "dropped", f.dropped, "want", want)
                    assert f.dropped == want, name
                    assert f.histogram == hist and sum(hist) == ncand == int(mult0.sum()), name
                pos, mult, grp, _ = _snapshot(c, concat, L)
                assert c.n == int(keep.sum()) and c.ncandidates == ncand
                assert pos.tolist() == pos0[keep].tolist(), name
                assert mult.tolist() == mult0[keep].tolist(), name
                assert grp.tolist() == grp0[keep].tolist(), name
            finally:
                c.close()
    finally:
        index.close()
        targets.close()


@pytest.mark.gpu
def test_tolerant_kernel_grouped_and_the_filters_own_index(ctx):
    """Three groups, the first and third sharing strings, through BackgroundFilter._apply_to_candidates, which builds
    its own tolerant index of the device; an empty tolerant index; candidates shorter than K."""
    from catch_amd import engine
    K, L, stride, H, M = 24, 64, 16, 2, 2
    records = _background(78, K)
    rng = np.random.default_rng(9)
    mixed = _planted(rng, L + stride * 299, records, K, 70, 0.04)
    other = _planted(rng, 1500, records[3:], K, 40, 0.04)
    genomes = [[mixed], [other], [mixed[:L + stride * 100], mixed[stride * 7:]]]
    concat = "".join(s for g in genomes for s in g)
    targets = engine.Targets(ctx, genomes)
    empty = engine.KmerIndex(ctx, ["ACGTNACGT"], K, mismatches=M)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, stride)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        f = BF(records, kmer=K, max_hits=H, mismatches=M)
        keep, want, hist, hits = _expect(f, strs0, mult0, L)
        exact = _expect(BF(records, kmer=K, max_hits=H), strs0, mult0, L)
        assert 0.05 * len(strs0) <= (~keep).sum() <= 0.95 * len(strs0) and (~keep).sum() > (~exact[0]).sum()
        c = engine.Candidates(ctx, targets, L, stride)
        total = c.ncandidates
        f._apply_to_candidates(c)
        own = f._device_indexes[ctx.device]
        assert own.mismatches == M and own.k == K and f.distinct_kmers() == own.n_unique
        pos, mult, grp, _ = _snapshot(c, concat, L)
        assert f.dropped == want and f.histogram == hist
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (pos0[keep].tolist(), mult0[keep].tolist(), grp0[keep].tolist())
        c.close()
        f.close()
        c = engine.Candidates(ctx, targets, L, stride)
        dropped, h = c.drop_background(empty, 0)
        assert dropped == 0 and h == [total] + [0] * 255
        assert c.measure(what="hits", index=empty, values=True, histograms=False)["hits"].max() == 0
        c.close()
        c = engine.Candidates(ctx, targets, K - 1, 5)
        short = c.n
        assert c.drop_background(empty, 0) == (0, [0] * 256) and c.n == short > 0
        c.close()
    finally:
        empty.close()
        targets.close()


def _hits_on_device(ctx, index, strs, L):
    """hits of every string (all of length L, without two N in a row, distinct) by the flag kernel's histogram-free
    sibling, the measure."""
    from catch_amd import engine
    targets = engine.Targets(ctx, [[s] for s in strs])
    try:
        c = engine.Candidates(ctx, targets, L, L)
        try:
            got = c.measure(what="hits", index=index, values=True, histograms=False)["hits"]
            row = {p // L: k for k, p in enumerate(c.positions().tolist())}
            dropped, hist = c.drop_background(index, 0)
            kept = {p // L for p in c.positions().tolist()}
        finally:
            c.close()
    finally:
        targets.close()
    hits = [int(got[row[i]]) for i in range(len(strs))]
    assert [i in kept for i in range(len(strs))] == [h == 0 for h in hits] and dropped == sum(1 for h in hits if h)
    return hits


def _near(codes, K, M, s):
    """Distinct codes within M mismatches of s or of its reverse complement, by Python integers."""
    out = set()
    for w in (s, _rc(s)):
        x = 0
        for ch in w:
            x = (x << 2) | CODE[ch]
        for c in codes:
            d = x ^ c
            if bin((d | (d >> 1)) & 0x5555555555555555).count("1") <= M:
                out.add(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K,M,view", [(32, 1, 1), (32, 1, 0), (32, 2, 2), (26, 2, 1)])
def test_long_bucket_first_last_and_none(ctx, K, M, view):
    """One bucket of `view` holds at least 300 entries: k-mers that are equal in block `view` and random elsewhere (they
    begin with A and end with C, so each is its own canonical form).  A candidate whose only match is the bucket's first
    entry, one for its last, and one that walks the whole bucket and finds nothing -- each substituted in the first
    character of every other block, so that no other view's bucket holds the match."""
    from catch_amd import engine
    rng = np.random.default_rng(1000 * K + 10 * M + view)
    starts = _starts(K, M)
    s0, s1 = starts[view], starts[view + 1]
    shared = _random_bases(rng, s1 - s0)
    kmers = set()
    while len(kmers) < 320:
        w = list(_random_bases(rng, K))
        w[s0:s1] = shared
        w[0], w[-1] = "A", "C"
        kmers.add("".join(w))
    shared = "".join(sorted(kmers)[0][s0:s1])           # (with the A or the C where the block holds an end)
    records = sorted(kmers) + [_random_bases(rng, 2000)]
    index = engine.KmerIndex(ctx, records, K, mismatches=M)
    try:
        codes = index.fetch().tolist()
        assert codes == sorted(set(_canonical_codes(records, K)))
        rotated = index.fetch_view(view).tolist()
        assert rotated == sorted(_rotl(c, 2 * s0, K) for c in codes)
        n = len(codes)
        P = min(max((n - 1).bit_length(), 8), min(2 * (s1 - s0), 30))
        top = 0
        for ch in shared:
            top = (top << 2) | CODE[ch]
        prefix = top >> (2 * (s1 - s0) - P)
        bucket = [c for c in rotated if c >> (2 * K - P) == prefix]
        assert len(bucket) >= 300, len(bucket)
        others = [starts[b] for b in range(M + 1) if b != view]
        cands = []
        for entry in (bucket[0], bucket[-1]):
            kmer = _decode(_rotl(entry, 2 * K - 2 * s0, K), K)
            cands.append(_substitute(kmer, others))
        none = list(_random_bases(rng, K))
        none[s0:s1] = shared
        cands.append("".join(none))
        L = K + 8
        strs = ["ACCA" + c + "TGGT" for c in cands] + ["GTTG" + _rc(c) + "CAAC" for c in cands]
        want = []
        for s, w in zip(strs, [1, 1, 0, 1, 1, 0]):
            near = _near(codes, K, M, s[4:4 + K])
            assert len(near) == w and not _near(codes, K, M - 1, s[4:4 + K]), "the candidate is not what it should be"
            # (where the entry is a k-mer of the long record, a flank may bring a neighbouring window within the budget)
            want.append(sum(1 for j in range(L - K + 1) if _near(codes, K, M, s[j:j + K])))
            assert want[-1] >= w and (w or want[-1] == 0)
        f = BF(records, kmer=K, mismatches=M)
        assert f._hits_equal_length(strs, L).tolist() == want
        assert _hits_on_device(ctx, index, strs, L) == want
    finally:
        index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K,M", KM)
def test_match_through_one_view_and_through_rc(ctx, K, M):
    """For every view b: a stored k-mer substituted in the first character of every other block (M substitutions: only
    view b's bucket holds it), as it is -- found through the forward word -- and reverse-complemented -- found through
    rc alone; with M + 1 substitutions, one per block, nothing finds it; a palindrome looks up one word."""
    from catch_amd import engine
    rng = np.random.default_rng(50 * K + M)
    records = [_random_bases(rng, 1500), _random_bases(rng, 700, 0.01)]
    if K % 2 == 0:
        half = _random_bases(rng, K // 2)
        records.append(half + _rc(half))
    index = engine.KmerIndex(ctx, records, K, mismatches=M)
    try:
        codes = index.fetch().tolist()
        starts = _starts(K, M)
        strs, want = [], []
        for b in range(M + 1):
            for pick in (17, len(codes) // 2, len(codes) - 9):
                kmer = _decode(codes[pick], K)
                v = _substitute(kmer, [starts[j] for j in range(M + 1) if j != b], 1 + pick % 3)
                miss = _substitute(kmer, [starts[j] + 1 for j in range(M + 1)], 2)
                for w, expect in ((v, 1), (_rc(v), 1), (miss, 0), (_rc(miss), 0)):
                    strs.append("CAC" + w + "GTG")
                    want.append(expect)
        pal = records[-1] if K % 2 == 0 else None
        if pal:
            strs += ["CAC" + pal + "GTG", "CAC" + _substitute(pal, [K // 2]) + "GTG"]
            want += [1, 1]
        L = K + 6
        keep = [i for i, s in enumerate(strs) if strs.index(s) == i]
        strs, want = [strs[i] for i in keep], [want[i] for i in keep]
        # the planted k-mer is window 3; a flank may bring a neighbouring window within the budget too, so every window
        # is counted by Python integers
        for s, w in zip(strs, want):
            if pal is None or sum(a != b for a, b in zip(s[3:3 + K], pal)) > 1:
                assert len(_near(codes, K, M, s[3:3 + K])) == w and not _near(codes, K, M - 1, s[3:3 + K]), s
        brute = [sum(1 for j in range(L - K + 1) if _near(codes, K, M, s[j:j + K])) for s in strs]
        assert all(h >= w for h, w in zip(brute, want)) and sum(want) >= 2 * 3 * (M + 1)
        numpy_hits = BF(records, kmer=K, mismatches=M)._hits_equal_length(strs, L).tolist()
        assert numpy_hits == brute
        assert _hits_on_device(ctx, index, strs, L) == numpy_hits
    finally:
        index.close()


# ------------------------------------------------------------------ GPU: the design commands
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


def _windows(seqs, L, stride):
    from catch_amd.filter import candidate_probes
    return [c for q in seqs for c in candidate_probes.candidate_strings_from_sequences([q], L, stride)]


def _run_design(argv, seed, capsys):
    from catch_amd import design
    random.seed(seed)
    np.random.seed(seed)
    capsys.readouterr()
    pb = design.main(design.parse_args(argv))
    return pb, capsys.readouterr().out


def _ebola5(tmp_path):
    recs = _ebola_records(5)
    fa = _write_records(tmp_path / "ebola5.fasta", recs)
    bg = _write_records(tmp_path / "background.fasta", [("background", _ebola_background(recs[0][1]))])
    return fa, bg, recs


def test_the_end_to_end_inputs_drop_strictly_more_with_one_mismatch():
    """No GPU: what the end-to-end test below relies on, by the NumPy rule."""
    recs = _ebola_records(5)
    background = [_ebola_background(recs[0][1])]
    cands = _windows([s for _, s in recs], 100, 50)
    gone = [len(cands) - len(BF(background, kmer=24, max_hits=0, mismatches=M)._filter_strs(cands)) for M in (0, 1)]
    print("candidates", len(cands), "dropped at M = 0, 1:", gone)
    assert len(cands) == 1888 and 0.02 * len(cands) < gone[0] < gone[1] < 0.6 * len(cands)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"]], ids=["dup", "hamming"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, caplog, extra):
    """--background-kmer 24 --background-mismatches 1 --background-max-hits 0 --write-background-histogram on the first
    5 Ebola genomes: the kernel on the device's candidates and NumPy on the host's strings give the same probes, the
    same histogram file and the same --verbose line; strictly more candidates go than at M = 0; --write-probe-report is
    probe_report -f of the output with the same options."""
    from catch_amd import engine, probe_report
    from catch_amd.filter.background_filter import BackgroundFilter
    fa, bg, recs = _ebola5(tmp_path)
    plain = [fa] + BASE + extra
    options = ["--background", bg, "--background-kmer", "24", "--background-max-hits", "0"]
    tolerant = options + ["--background-mismatches", "1"]
    outs, hists, dropped, lines, calls = {}, {}, {}, {}, []
    real = engine.Candidates.drop_background

    def counted(self, index, *a, **k):
        calls.append((index.mismatches, self.n))
        return real(self, index, *a, **k)
    monkeypatch.setattr(engine.Candidates, "drop_background", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn, hn, rn = (tmp_path / (front + ext) for ext in (".fasta", ".tsv", ".report.tsv"))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="catch_amd.design"):
            pb, printed = _run_design(plain + tolerant + ["--write-background-histogram", str(hn), "--verbose", "-o", str(fn),
                                                          "--write-probe-report", str(rn)], 5, capsys)
        outs[front], hists[front] = fn.read_bytes(), hn.read_bytes()
        lines[front] = [r.getMessage() for r in caplog.records if r.getMessage().startswith("background filter:")]
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        bf = [f for f in pb.filters if type(f) is BackgroundFilter]
        assert len(bf) == 1 and bf[0].mismatches == 1
        dropped[front] = (bf[0].dropped, list(bf[0].histogram))
        if front == "device":
            assert len(calls) == 1 and calls[0][0] == 1, "the device front end did not run the tolerant kernel"
        again = tmp_path / (front + ".again.tsv")
        probe_report.main(probe_report.parse_args(["-f", str(fn), "-o", str(again)] + tolerant))
        capsys.readouterr()
        assert rn.read_bytes() == again.read_bytes() and again.read_text().count("\n") == outs[front].count(b">") + 1
        rows = [line.split("\t") for line in again.read_text().splitlines()]
        assert rows[0][-2:] == ["background_hits", "verdict"] and all(r[-2:] == ["0", "ok"] for r in rows[1:])
    assert len(calls) == 1, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"] and hists["device"] == hists["host"]
    assert dropped["device"] == dropped["host"] and lines["device"] == lines["host"] and len(lines["device"]) == 1
    assert "within 1 mismatches" in lines["device"][0]
    gone, hist = dropped["device"]
    assert sum(hist) == 1888 and gone == sum(hist[1:])
    # the same run with exact k-mers drops strictly fewer
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    pb, _ = _run_design(plain + options + ["-o", str(tmp_path / "exact.fasta")], 5, capsys)
    exact = [f for f in pb.filters if type(f) is BackgroundFilter][0]
    print("dropped at M = 1:", gone, "at M = 0:", exact.dropped)
    assert exact.mismatches == 0 and 0 < exact.dropped < gone and calls[-1][0] == 0
    assert (tmp_path / "exact.fasta").read_bytes() != outs["device"]
