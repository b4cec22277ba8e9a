"""design_naively: the two redundancy predicates, the naive redundant filter and
the dominating set filter (catch_amd/filter/naive_redundant_filter.py,
dominating_set_filter.py, csrc/redundant.hip, catch_amd/design_naively.py).

tests/golden/naive.json.gz holds what the live reference computes
(tests/golden/make_naive_golden.py): k_lcf and mismatches_at_offset of ~400 pairs,
the two filters' outputs with the exact predicate, and bin/design_naively.py's
counts.  The GPU tests compare the device graph with a NumPy restatement of the
two predicates (every diagonal, windows of exactly lcf_thres) that is itself
checked against the golden pairs without a GPU.
"""
import functools
import os
import re

import numpy as np
import pytest

from util import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (0, 1, 2, 3, 5)


@pytest.fixture(scope="module")
def golden():
    return load_golden("naive")


# ------------------------------------------------------------------ restatement
def _encode(strs):
    n = len(strs)
    width = max([len(s) for s in strs] + [1])
    arr = np.zeros((n, width), dtype=np.uint8)
    for i, s in enumerate(strs):
        arr[i, :len(s)] = np.frombuffer(s.encode("ascii"), dtype=np.uint8)
    return arr, np.array([len(s) for s in strs], dtype=np.int64)


_NEVER = 1 << 12          # what a position outside the overlap adds to a window: more than any mismatch budget asked for


def _fewest(A, la, B, lb, kind, p):
    """For every pair of the broadcast of A (..., LA) against B (..., LB).  kind "lcf": the fewest mismatches in a window
    of exactly p >= 1 positions inside the overlap, over every diagonal (>= _NEVER where no diagonal holds such a
    window); kind "shift": the fewest mismatches of the overlap (possibly empty: 0) over the offsets in [-p, p]."""
    LA, LB = A.shape[-1], B.shape[-1]
    shape = np.broadcast_shapes(A.shape[:-1], B.shape[:-1])
    best = np.full(shape, _NEVER * (LA + LB + 1), dtype=np.int64)
    for d in (range(-(LB - 1), LA) if kind == "lcf" else range(-p, p + 1)):
        i0, j0 = max(d, 0), max(-d, 0)
        size = min(LA - i0, LB - j0)
        overlap = np.minimum(la - i0, lb - j0)
        if kind == "shift":
            if size <= 0:
                count = np.zeros(shape, dtype=np.int64)
            else:
                neq = A[..., i0:i0 + size] != B[..., j0:j0 + size]
                count = (neq & (np.arange(size) < overlap[..., None])).sum(axis=-1)
            best = np.minimum(best, count)
            continue
        if size < p:
            continue
        neq = np.where(np.arange(size) < overlap[..., None], A[..., i0:i0 + size] != B[..., j0:j0 + size], _NEVER)
        cs = np.cumsum(neq, axis=-1, dtype=np.int32)             # (a window that leaves the overlap: >= _NEVER)
        win = cs[..., p - 1:].copy()
        win[..., 1:] -= cs[..., :size - p]
        best = np.minimum(best, win.min(axis=-1))
    return best


def _redundant(A, la, B, lb, kind, p0, p1):
    """The predicate for every pair of the broadcast of A (..., LA) against B (..., LB): kind "lcf": on some diagonal
    a window of exactly p1 positions inside the overlap has at most p0 mismatches (everything when p1 <= 0); kind
    "shift": for some offset in [-p0, p0] the overlap (possibly empty) has at most p1 mismatches."""
    assert p0 < _NEVER and p1 < _NEVER
    if kind == "lcf":
        if p1 <= 0:
            return np.ones(np.broadcast_shapes(A.shape[:-1], B.shape[:-1]), dtype=bool)
        return _fewest(A, la, B, lb, "lcf", p1) <= p0
    return _fewest(A, la, B, lb, "shift", p0) <= p1


@functools.lru_cache(maxsize=4)
def _fewest_of_pairs(strs, kind, p):
    """_fewest for the pairs i < j of a probe set: computed once for every mismatch budget a test asks about."""
    arr, lens = _encode(strs)
    i, j = np.triu_indices(len(strs), 1)
    return i, j, _fewest(arr[i], lens[i], arr[j], lens[j], kind, p)


def restate_graph(strs, kind, p0, p1):
    """Adjacency matrix (symmetric, no self loops) of the redundancy graph; pair (i, j), i < j, is (a, b)."""
    n = len(strs)
    adj = np.zeros((n, n), dtype=bool)
    if kind == "lcf" and p1 <= 0:
        adj[np.triu_indices(n, 1)] = True
    else:
        assert p0 < _NEVER and p1 < _NEVER
        i, j, fewest = _fewest_of_pairs(tuple(strs), kind, p1 if kind == "lcf" else p0)
        adj[i, j] = fewest <= (p0 if kind == "lcf" else p1)
    return adj | adj.T


def naive_loop(ptr, idx):
    """The reference's double loop over a CSR graph: the kept vertices."""
    n = len(ptr) - 1
    dropped = np.zeros(n, dtype=bool)
    for i in range(n):
        if not dropped[i]:
            nb = idx[ptr[i]:ptr[i + 1]]
            dropped[nb[nb > i]] = True
    return ~dropped


# ------------------------------------------------------------------ no GPU
def test_host_predicates_and_probe_methods_reproduce_the_golden_pairs(golden):
    from catch_amd import probe
    from catch_amd.filter import naive_redundant_filter as nrf
    from catch_amd.utils import longest_common_substring as lcs
    assert len(golden["pairs"]) >= 380
    unequal = with_n = 0
    for rec in golden["pairs"]:
        a, b = rec["a"], rec["b"]
        pa, pb = probe.Probe.from_str(a), probe.Probe.from_str(b)
        unequal += len(a) != len(b)
        with_n += "N" in a or "N" in b
        for k in KS:
            want = rec["k_lcf"][str(k)]
            length, sa, sb = lcs.k_lcf(a, b, k)
            assert length == want, (a, b, k)
            assert sum(x != y for x, y in zip(a[sa:sa + length], b[sb:sb + length])) <= k
            assert pa.longest_common_substring_length(pb, k) == want
        for k in (0, 2):
            want = rec["k_lcf"][str(k)]
            assert nrf.redundant_longest_common_substring(k, want)(pa, pb) is True
            assert nrf.redundant_longest_common_substring(k, want + 1, prune_with_heuristic_and_anchor=False)(pa, pb) is False
        if "mismatches_at_offset" in rec:
            L = len(a)
            mm = rec["mismatches_at_offset"]
            assert len(mm) == 2 * L - 1
            for o in sorted(o for o in {-(L - 1), -1, 0, 1, L // 2, L - 1} if abs(o) < L):
                assert pa.mismatches_at_offset(pb, o) == mm[o + L - 1], (a, b, o)
            for shift in sorted({0, min(5, L - 1), L - 1}):
                lo = min(mm[L - 1 - shift:L + shift])
                assert pa.min_mismatches_within_shift(pb, shift) == lo
                for thres in (0, 3, 12):       # (12: off the quick path)
                    assert nrf.redundant_shift_and_mismatch_count(shift, thres)(pa, pb) == (lo <= thres)
            with pytest.raises(ValueError):
                pa.mismatches_at_offset(pb, L)
        else:
            with pytest.raises(ValueError):
                pa.mismatches_at_offset(pb, 0)
            with pytest.raises(ValueError):
                nrf.redundant_shift_and_mismatch_count(0, 12)(pa, pb)
            # the quick path takes unequal lengths; beyond the shorter probe the overlap is empty: 0 mismatches
            assert nrf.redundant_shift_and_mismatch_count(max(len(a), len(b)), 0)(pa, pb) is True
    assert unequal >= 60 and with_n >= 100


def test_numpy_restatement_reproduces_the_golden_pairs(golden):
    pairs = golden["pairs"]
    A, la = _encode([r["a"] for r in pairs])
    B, lb = _encode([r["b"] for r in pairs])
    for k in KS:
        lcf = np.array([r["k_lcf"][str(k)] for r in pairs])
        for thres in (0, 1, 2, 3, 5, 8, 13, 20, 31, 40, 50, 63, 64, 65, 80, 100, 127, 128, 129, 130, 131):
            got = _redundant(A, la, B, lb, "lcf", k, thres)
            assert (got == (lcf >= thres)).all(), (k, thres)
    eq = [i for i, r in enumerate(pairs) if "mismatches_at_offset" in r]
    for shift in (0, 1, 5, 40, 129, 130, 200):
        for thres in (0, 1, 3, 10):
            got = _redundant(A[eq], la[eq], B[eq], lb[eq], "shift", shift, thres)
            for g, i in zip(got.tolist(), eq):
                mm, L = pairs[i]["mismatches_at_offset"], len(pairs[i]["a"])
                want = shift >= L or min(mm[L - 1 - shift:L + shift]) <= thres       # (an empty overlap: 0 mismatches)
                assert g == want, (pairs[i], shift, thres)


def test_restatement_is_the_pair_by_pair_predicate_on_a_small_mixed_set():
    """restate_graph (all pairs at once) against the host predicates pair by pair, unequal lengths and N included."""
    from catch_amd import probe
    from catch_amd.filter import naive_redundant_filter as nrf
    rng = np.random.default_rng(5)
    strs = _probe_set(rng, 14, None, n_rate=0.05)
    probes = [probe.Probe.from_str(s) for s in strs]
    for kind, fn, p0, p1 in (("lcf", nrf.redundant_longest_common_substring(1, 12), 1, 12),
                             ("shift", nrf.redundant_shift_and_mismatch_count(4, 2), 4, 2)):
        adj = restate_graph(strs, kind, p0, p1)
        for i in range(len(strs)):
            for j in range(i + 1, len(strs)):
                assert adj[i, j] == fn(probes[i], probes[j]), (kind, strs[i], strs[j])


def _write_fasta(golden, tmp_path):
    path = tmp_path / "naive3.fasta"
    path.write_text(golden["runs"]["fasta"])
    return str(path)


def test_command_argument_errors(golden, tmp_path):
    from catch_amd import design_naively
    fasta = _write_fasta(golden, tmp_path)
    with pytest.raises(Exception, match="Cannot use both"):
        design_naively.main(design_naively.parse_args([fasta, "-nrf", "3", "80", "-dsf", "3", "80"]))
    with pytest.raises(Exception, match="Cannot --limit-target-genomes and"):
        design_naively.main(design_naively.parse_args(
            [fasta, "--limit-target-genomes", "2", "--limit-target-genomes-randomly-with-replacement", "2"]))
    with pytest.raises(ValueError, match="FASTA file"):
        design_naively.main(design_naively.parse_args([str(tmp_path / "absent.fasta")]))
    with pytest.raises(SystemExit):
        design_naively.parse_args([fasta, "-nrf", "3"])
    args = design_naively.parse_args([fasta])
    assert (args.probe_length, args.probe_stride, args.naive_redundant_filter, args.dominating_set_filter) == (100, 50, None, None)
    assert args.write_probe_fasta is None and not args.add_reverse_complements and not args.print_analysis


def test_foreign_callable_long_probe_and_foreign_letter_are_refused():
    from catch_amd import engine, probe
    from catch_amd.filter import naive_redundant_filter as nrf
    from catch_amd.filter.dominating_set_filter import DominatingSetFilter
    for cls in (nrf.NaiveRedundantFilter, DominatingSetFilter):
        with pytest.raises(NotImplementedError):
            cls(lambda a, b: a.seq_str == b.seq_str)
        f = cls(nrf.redundant_longest_common_substring(2, 10))
        with pytest.raises(ValueError, match="ACGTN"):
            f._filter([probe.Probe.from_str("ACGTACGTACGT"), probe.Probe.from_str("ACGTACGUACGT")])
        with pytest.raises(ValueError, match="ACGTN"):
            f._filter_strs(["ACGTACGTACGT", "acgtacgtacgt"])
        with pytest.raises(ValueError, match=str(engine.REDUNDANT_MAX_LENGTH)):
            f._filter_strs(["ACGT", "A" * (engine.REDUNDANT_MAX_LENGTH + 1)])
        assert f._filter([]) == [] and f._filter_strs([]) == []
    assert engine.REDUNDANT_MAX_LENGTH >= 256
    # off the quick path the reference raises for unequal lengths and for a shift of a whole probe
    slow = nrf.NaiveRedundantFilter(nrf.redundant_shift_and_mismatch_count(1, 12))
    with pytest.raises(ValueError, match="same length"):
        slow._filter_strs(["ACGTA", "ACGT"])
    with pytest.raises(ValueError, match="Invalid offset"):
        nrf.NaiveRedundantFilter(nrf.redundant_shift_and_mismatch_count(4, 12))._filter_strs(["ACGT", "ACGA"])
    # the predicates say what they are
    fn = nrf.redundant_longest_common_substring(3, 80)
    assert (fn.redundancy_kind, fn.redundancy_params) == ("lcf", (3, 80))
    fn = nrf.redundant_shift_and_mismatch_count(shift=5, mismatch_thres=3)
    assert (fn.redundancy_kind, fn.redundancy_params) == ("shift", (5, 3, True))


def test_redundancy_symbols_declared_bound_and_built():
    from catch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name in ("catchhip_redundancy_graph", "catchhip_redundancy_fetch", "catchhip_redundancy_destroy",
                 "catchhip_redundancy_naive", "catchhip_redundancy_rows"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
    assert "naive_redundant_filter.py" in hdr and "dominating_set_filter.py" in hdr and "set_cover.py:14-144" in hdr
    assert "redundant.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------ GPU
def _probe_set(rng, n, length, n_rate=0.0, root_length=230, max_length=150):
    """n probes in families: windows of a few roots of root_length bases with 0-3 substitutions; length None: lengths
    1-max_length mixed."""
    roots = ["".join(rng.choice(list("ACGT"), size=root_length)) for _ in range(max(1, n // 6))]
    out = []
    for _ in range(n):
        L = int(rng.integers(1, max_length + 1)) if length is None else length
        root = roots[int(rng.integers(len(roots)))]
        at = int(rng.integers(0, min(12, root_length - L) + 1))
        s = list(root[at:at + L])
        for j in rng.choice(L, size=min(L, int(rng.integers(0, 4))), replace=False):
            s[j] = "ACGT"[int(rng.integers(4))]
        for j in range(L):
            if rng.random() < n_rate:
                s[j] = "N"
        out.append("".join(s))
    return out


def _check_graph(ctx, strs, kind, p0, p1):
    from catch_amd import engine
    code = engine.REDUNDANT_LCF if kind == "lcf" else engine.REDUNDANT_SHIFT
    g = engine.RedundancyGraph(ctx, strs, code, p0, p1)
    try:
        ptr, idx = g.fetch()
        n = len(strs)
        assert ptr[0] == 0 and ptr[-1] == g.nedges == idx.size and (np.diff(ptr) >= 0).all()
        got = np.zeros((n, n), dtype=bool)
        for i in range(n):
            nb = idx[ptr[i]:ptr[i + 1]].astype(np.int64)
            assert (np.diff(nb) > 0).all(), "row %d is not ascending" % i
            assert (nb != i).all() and (nb < n).all()
            got[i, nb] = True
        assert (got == got.T).all()
        want = restate_graph(strs, kind, p0, p1)
        assert (got == want).all(), (kind, p0, p1, np.argwhere(got != want)[:5].tolist())
        keep = g.naive()
        assert (keep == naive_loop(ptr, idx)).all(), (kind, p0, p1)
        return int(g.nedges)
    finally:
        g.close()


# (n, probe length or None = lengths 1-150 mixed or (1, M) = lengths 1-M mixed, share of N): 63 / 64 / 65 and 130 straddle
# the 64-probe pair tile; from 129 bases a plane is four 64-base words, all four in use from 193, full at 256
GRAPH_SETS = [(1, 40, 0.0), (2, 128, 0.0), (63, 65, 0.02), (64, 64, 0.0), (65, 1, 0.1), (65, 40, 0.03), (40, 100, 0.02),
              (130, 40, 0.0), (36, 128, 0.02), (36, 129, 0.0), (40, None, 0.03),
              (40, 192, 0.0), (40, 193, 0.02), (36, 255, 0.02), (36, 256, 0.0), (65, 256, 0.01), (40, (1, 256), 0.03)]
LONG_ROOT = 280           # root length of the sets longer than 150 bases (a window of 256 at offsets 0-12)


def _graph_set(n, length, n_rate):
    """The probes of one GRAPH_SETS entry and the length its thresholds and shifts are taken around."""
    if isinstance(length, tuple):
        rng = np.random.default_rng(1000 + n * 7 + length[1])
        return _probe_set(rng, n, None, n_rate, root_length=LONG_ROOT, max_length=length[1]), 200
    rng = np.random.default_rng(1000 + n * 7 + (length or 0))
    if length is not None and length > 150:
        return _probe_set(rng, n, length, n_rate, root_length=LONG_ROOT), length
    return _probe_set(rng, n, length, n_rate), length if length is not None else 100


def test_long_graph_sets_fill_the_words_they_are_there_for():
    """No GPU: the sets above 128 bases use the plane words claimed -- 192 fills word 2 exactly, 193 puts one base into
    word 3, 255 / 256 leave one bit / nothing of word 3 free -- and the mixed set holds lengths on both sides of every
    word boundary, 256 itself not required."""
    for n, length, n_rate in GRAPH_SETS:
        strs, around = _graph_set(n, length, n_rate)
        assert len(strs) == n and set("".join(strs)) <= set("ACGTN")
        if isinstance(length, tuple):
            lens = sorted(len(s) for s in strs)
            assert around == 200 and lens[0] >= 1 and lens[-1] <= 256
            for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 256)):
                assert sum(lo <= x <= hi for x in lens) >= 4, (lo, hi, lens)
        elif length is not None:
            assert around == length and all(len(s) == length for s in strs)
        if n_rate > 0 and n * (around if length is None or isinstance(length, tuple) else length) >= 1000:
            assert any("N" in s for s in strs)
    # today's sets are the sets of before the generalisation (same seeds, same draws)
    assert _graph_set(36, 129, 0.0)[0] == _probe_set(np.random.default_rng(1000 + 36 * 7 + 129), 36, 129, 0.0)
    assert _graph_set(40, None, 0.03)[0] == _probe_set(np.random.default_rng(1000 + 40 * 7), 40, None, 0.03)


@pytest.mark.gpu
@pytest.mark.parametrize("n,length,n_rate", GRAPH_SETS)
def test_graph_equals_restatement_both_kinds_and_naive_pass_equals_the_loop(ctx, n, length, n_rate):
    strs, L = _graph_set(n, length, n_rate)
    edges = 0
    for lcf_thres in sorted({1, max(L // 2, 1), L, L + 1}):
        for mismatches in (0, 2, 5):
            edges += _check_graph(ctx, strs, "lcf", mismatches, lcf_thres)
    for shift in sorted({0, 5, max(L - 1, 0), L}):
        for thres in (0, 3):
            edges += _check_graph(ctx, strs, "shift", shift, thres)
    assert n < 2 or edges > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,length,n_rate,shift", [(64, 64, 0.0, 70), (63, 65, 0.02, 129), (36, 256, 0.0, 300),
                                                   (36, 256, 0.0, 257), (40, (1, 256), 0.03, 300)])
def test_graph_shift_beyond_the_packed_width(ctx, n, length, n_rate, shift):
    """A shift above the 64 W bases the planes hold (W = 1 up to 64 bases, 2 up to 128, 4 up to 256): the kernel
    clamps the diagonals it walks to 64 W, where every overlap is empty and so without a mismatch -- all pairs, as
    the restatement says, whatever the mismatch threshold."""
    strs, _ = _graph_set(n, length, n_rate)
    for thres in (0, 3):
        assert _check_graph(ctx, strs, "shift", shift, thres) == n * (n - 1)


@pytest.mark.gpu
def test_graph_of_257_probes(ctx):
    strs = _probe_set(np.random.default_rng(257), 257, 40, 0.01)
    assert _check_graph(ctx, strs, "lcf", 2, 20) > 0
    assert _check_graph(ctx, strs, "shift", 5, 3) > 0


@pytest.mark.gpu
def test_graph_refuses_what_it_cannot_pack(ctx):
    from catch_amd import engine
    with pytest.raises(ValueError, match="256"):
        engine.RedundancyGraph(ctx, ["ACGT", "A" * 257], engine.REDUNDANT_LCF, 0, 2)
    with pytest.raises(ValueError, match="ACGTN"):
        engine.RedundancyGraph(ctx, ["ACGT", "ACGU"], engine.REDUNDANT_LCF, 0, 2)
    with pytest.raises(ValueError, match="every pair"):
        engine.RedundancyGraph(ctx, ["ACGT", "ACGA"], engine.REDUNDANT_LCF, 0, 0)
    with pytest.raises(ValueError, match="mismatches must not be negative"):
        engine.RedundancyGraph(ctx, ["ACGT", "ACGA"], engine.REDUNDANT_LCF, -1, 2)
    with pytest.raises(ValueError, match="shift must not be negative"):
        engine.RedundancyGraph(ctx, ["ACGT", "ACGA"], engine.REDUNDANT_SHIFT, -1, 0)
    g = engine.RedundancyGraph(ctx, [], engine.REDUNDANT_SHIFT, 0, 0)
    assert g.nedges == 0 and g.naive().size == 0 and g.fetch()[0].tolist() == [0]
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 2500])
def test_naive_pass_on_a_path_an_empty_and_a_complete_graph(ctx, n):
    """Windows of one random sequence at stride 20: neighbours share 40 bases, second neighbours 20, so under LCF
    (0, 30) the graph is a path -- the longest possible dependency chain (2,500 vertices: more than one chunk of the
    one-workgroup walk).  lcf_thres = L + 1: no edges.  shift = L: complete."""
    from catch_amd import engine
    rng = np.random.default_rng(n)
    seq = "".join(rng.choice(list("ACGT"), size=20 * n + 40))
    strs = [seq[20 * i:20 * i + 60] for i in range(n)]
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, 0, 30)
    ptr, idx = g.fetch()
    assert g.nedges == 2 * (n - 1)
    for i in (0, 1, n // 2, n - 1):
        assert idx[ptr[i]:ptr[i + 1]].tolist() == [j for j in (i - 1, i + 1) if 0 <= j < n]
    keep = g.naive()
    assert (keep == naive_loop(ptr, idx)).all() and keep.tolist() == [i % 2 == 0 for i in range(n)]
    g.close()
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, 0, 61)
    assert g.nedges == 0 and g.naive().all()
    g.close()
    if n <= 300:
        g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_SHIFT, 60, 0)
        assert g.nedges == n * (n - 1)
        assert g.naive().tolist() == [True] + [False] * (n - 1)
        g.close()


@pytest.mark.gpu
def test_naive_pass_on_a_path_of_256_base_probes(ctx):
    """Windows of 256 bases at stride 100: neighbours share 156 bases, second neighbours 56, so under LCF (0, 120) the
    graph is a path of 300 vertices whose every comparison runs over all four words of a plane.  lcf_thres = 257: no
    edges.  shift = 256: complete."""
    from catch_amd import engine
    n = 300
    rng = np.random.default_rng(256)
    seq = "".join(rng.choice(list("ACGT"), size=100 * n + 156))
    strs = [seq[100 * i:100 * i + 256] for i in range(n)]
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, 0, 120)
    ptr, idx = g.fetch()
    assert g.nedges == 2 * (n - 1)
    assert all(idx[ptr[i]:ptr[i + 1]].tolist() == [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n))
    keep = g.naive()
    assert (keep == naive_loop(ptr, idx)).all() and keep.tolist() == [i % 2 == 0 for i in range(n)]
    g.close()
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_LCF, 0, 257)
    assert g.nedges == 0 and g.naive().all()
    g.close()
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_SHIFT, 256, 0)
    assert g.nedges == n * (n - 1)
    assert g.naive().tolist() == [True] + [False] * (n - 1)
    g.close()


# ------------------------------------------------------------------ more than 4,096 probes: a second turn of 64 bitmap words
BIG_N, BIG_FAMILIES, BIG_LENGTH = 4200, 600, 24


@functools.lru_cache(maxsize=1)
def _big_family_set():
    """4,200 probes of 24 bases: member k of family f sits at index f + 600 k and is the family's root with 0-2
    substitutions out of ACGT and, now and then, N.  A family's members lie 600 indices apart, so rows below 4,096
    have neighbours in the bitmap words 64 and 65 (columns 4,096-4,199) and the other way round."""
    rng = np.random.default_rng(4200)
    roots = rng.choice(list("ACGT"), size=(BIG_FAMILIES, BIG_LENGTH))
    out = []
    for i in range(BIG_N):
        s = roots[i % BIG_FAMILIES].copy()
        for j in rng.choice(BIG_LENGTH, size=int(rng.integers(0, 3)), replace=False):
            s[j] = "N" if rng.random() < 0.1 else "ACGT"[int(rng.integers(4))]
        out.append("".join(s))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def _big_mismatches():
    """Hamming distance of every pair of _big_family_set, N a letter of its own: 24 minus the product of the one-hot
    encodings (position x letter).  The product is taken in float32, whose sums of at most 24 ones are exact."""
    strs = _big_family_set()
    arr, lens = _encode(list(strs))
    assert (lens == BIG_LENGTH).all()
    onehot = (arr[:, :, None] == np.frombuffer(b"ACGTN", dtype=np.uint8)[None, None, :])
    assert (onehot.sum(axis=2) == 1).all()
    flat = onehot.reshape(BIG_N, BIG_LENGTH * 5).astype(np.float32)
    same = flat @ flat.T
    assert same.max() == BIG_LENGTH and (same == np.rint(same)).all()
    return BIG_LENGTH - same.astype(np.int64)


def _big_adjacency(thres):
    adj = _big_mismatches() <= thres
    np.fill_diagonal(adj, False)
    return adj


def test_hamming_adjacency_of_the_big_set_is_the_restatement_on_a_slice():
    """No GPU: kind "shift" with shift 0 is the Hamming predicate, so restate_graph(..., "shift", 0, t) of 200 probes
    of the big set -- 29 whole families, members on both sides of column 4,096 among them -- is that block of the
    one-hot adjacency, at both thresholds, with edges at both; and the set is what it claims."""
    strs = _big_family_set()
    assert len(strs) == BIG_N and all(len(s) == BIG_LENGTH for s in strs) and set("".join(strs)) == set("ACGTN")
    assert -(-BIG_N // 64) == 66                             # bitmap words per row: a second turn of the 64-word walk
    pick = np.asarray([f + BIG_FAMILIES * k for f in range(540, 569) for k in range(7)][:200])
    assert (pick < 4096).any() and (pick >= 4096).any() and (pick >= 4160).any()
    sub = [strs[i] for i in pick]
    for thres in (0, 4):
        adj = _big_adjacency(thres)
        want = restate_graph(sub, "shift", 0, thres)
        assert want.any() and (adj[np.ix_(pick, pick)] == want).all(), thres
        assert (adj == adj.T).all() and not adj.diagonal().any()
        # some family has members on both sides of column 4,096, joined by an edge; both ways round, word 65 included
        assert adj[500, 500 + 6 * BIG_FAMILIES] or thres == 0
        assert adj[:4096, 4096:].any() and adj[4096:, :4096].any() and adj[:4096, 4160:].any() and adj[4160:, :4096].any()
        in_family = adj[np.arange(BIG_N)[:, None] % BIG_FAMILIES == np.arange(BIG_N)[None, :] % BIG_FAMILIES].sum()
        assert in_family >= (1000 if thres == 0 else 25000) and (thres == 0 or in_family == BIG_N * 6)
    assert _big_adjacency(4).sum() > _big_adjacency(0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("thres", [0, 4])
def test_graph_naive_pass_and_rows_above_4096_probes(ctx, thres):
    """66 bitmap words per row: rg_degree_kernel and rg_fill_kernel take a second turn (and carry the count of the
    first 64 words into it), rg_pairs_kernel runs on a 66 x 66 tile grid.  The fetched CSR graph is compared whole
    with the one-hot adjacency, the naive pass with the reference's loop, the dominating-set rows with
    {i} + N(i) in order."""
    from catch_amd import engine
    strs = list(_big_family_set())
    adj = _big_adjacency(thres)
    g = engine.RedundancyGraph(ctx, strs, engine.REDUNDANT_SHIFT, 0, thres)
    try:
        ptr, idx = g.fetch()
        want_ptr = np.concatenate(([0], np.cumsum(adj.sum(axis=1))))
        want_row, want_idx = np.nonzero(adj)                             # row-major: every row ascending
        assert want_idx.size > 0 and g.nedges == idx.size
        assert np.array_equal(ptr, want_ptr), np.nonzero(ptr != want_ptr)[0][:5].tolist()
        assert np.array_equal(idx, want_idx), np.nonzero(idx != want_idx)[0][:5].tolist()
        # (said by the equality, and cheap to say on its own:) symmetric, every row ascending, no loops
        got = np.zeros((BIG_N, BIG_N), dtype=bool)
        row = np.repeat(np.arange(BIG_N), np.diff(ptr))
        got[row, idx] = True
        assert (got == got.T).all() and not got.diagonal().any()
        inner = np.ones(idx.size, dtype=bool)
        inner[ptr[:-1][np.diff(ptr) > 0]] = False
        assert (np.diff(idx.astype(np.int64))[inner[1:]] > 0).all()
        keep = g.naive()
        assert np.array_equal(keep, naive_loop(ptr, idx)) and 0 < keep.sum() < BIG_N
        rows = g.rows()
        try:
            assert rows.n == g.nedges + BIG_N
            set_id, univ, start, end = rows.fetch()
            with_self = adj.copy()
            np.fill_diagonal(with_self, True)
            want_set, want_elem = np.nonzero(with_self)
            assert np.array_equal(set_id, want_set) and np.array_equal(start, 2 * want_elem)
            assert np.array_equal(end, start + 1) and not univ.any()
        finally:
            rows.close()
        high = int((want_idx[want_row < 4096] >= 4096).sum()), int((want_idx[want_row >= 4096] < 4096).sum())
        assert high[0] > 0 and high[1] > 0 and (want_idx[want_row < 4096] >= 4160).any()
        print("redundancy graph of %d probes, mismatches <= %d: rowwords %d, %d directed edges, %d from rows below 4096 "
              "to columns from 4096, %d the other way, longest row %d, naive pass keeps %d"
              % (BIG_N, thres, -(-BIG_N // 64), idx.size, high[0], high[1], int(np.diff(ptr).max()), int(keep.sum())))
    finally:
        g.close()


def _predicate(case):
    from catch_amd.filter import naive_redundant_filter as nrf
    if case["kind"] == "default":
        return None
    if case["kind"] == "lcf":
        return nrf.redundant_longest_common_substring(*case["params"])
    return nrf.redundant_shift_and_mismatch_count(*case["params"])


@pytest.mark.gpu
def test_both_classes_reproduce_every_golden_filter_case_in_returned_order(golden):
    from catch_amd import probe
    from catch_amd.filter.dominating_set_filter import DominatingSetFilter
    from catch_amd.filter.naive_redundant_filter import NaiveRedundantFilter
    names = [c["name"] for c in golden["filters"]]
    assert len(names) >= 14 and any("dups" in n for n in names) and "families_shift_5_3" in names
    for case in golden["filters"]:
        probes = [probe.Probe.from_str(s) for s in case["probes"]]
        index = {id(p): i for i, p in enumerate(probes)}
        got = [index[id(p)] for p in NaiveRedundantFilter(_predicate(case))._filter(list(probes))]
        assert got == case["nrf"], case["name"]
        dsf = DominatingSetFilter(_predicate(case))
        got = [index[id(p)] for p in dsf._filter(list(probes))]
        assert got == case["dsf"], case["name"]
        assert sorted(dsf.last_picks) == sorted(case["dsf"])
        assert NaiveRedundantFilter(_predicate(case))._filter_strs(case["probes"]) == [case["probes"][i] for i in case["nrf"]]
        assert dsf._filter_strs(case["probes"]) == [case["probes"][i] for i in case["dsf"]]
    fam = next(c for c in golden["filters"] if c["name"] == "families_shift_5_3")
    assert fam["dsf"] != sorted(fam["dsf"])      # (the interpreter's set order, not an ascending list)


@pytest.mark.gpu
def test_dominating_set_picks_cover_everything_each_with_a_gain(ctx, golden):
    from catch_amd import engine
    for case in golden["filters"]:
        if case["kind"] == "default" or (case["kind"] == "lcf" and case["params"][1] <= 0):
            continue
        uniq = list(dict.fromkeys(case["probes"]))
        code = engine.REDUNDANT_LCF if case["kind"] == "lcf" else engine.REDUNDANT_SHIFT
        g = engine.RedundancyGraph(ctx, uniq, code, case["params"][0], case["params"][1])
        rows = g.rows()
        assert rows.n == g.nedges + len(uniq)
        set_id, univ, start, end = rows.fetch()
        assert (np.diff(set_id) >= 0).all() and (univ == 0).all() and (end == start + 1).all() and (start % 2 == 0).all()
        ptr, idx = g.fetch()
        for i in (0, len(uniq) // 2, len(uniq) - 1):
            members = sorted(idx[ptr[i]:ptr[i + 1]].tolist() + [i])
            assert (start[set_id == i] // 2).tolist() == members
        picks = rows.greedy(len(uniq))
        first = {s: i for i, s in reversed(list(enumerate(case["probes"])))}
        assert sorted(first[uniq[u]] for u in picks) == sorted(case["dsf"]), case["name"]
        chk = rows.cover_check(len(uniq), picks)
        assert chk["picks_without_gain"] == 0 and chk["universes_short"] == 0 and chk["bad_pick_ids"] == 0
        assert chk["covered_bases"] == chk["universe_bases"] == len(uniq)
        rows.close()
        g.close()


@pytest.mark.gpu
def test_command_reproduces_the_reference_counts_writes_its_probes_and_analyses(golden, tmp_path, capsys):
    from catch_amd import design_naively
    from catch_amd.utils import seq_io
    fasta = _write_fasta(golden, tmp_path)
    runs = golden["runs"]["runs"]
    assert {tuple(r["options"]) for r in runs} >= {("-nrf", "3", "80"), ("-dsf", "3", "80"), (), ("--add-reverse-complements",)}
    for run in runs:
        capsys.readouterr()
        design_naively.main(design_naively.parse_args([fasta] + run["options"]))
        assert capsys.readouterr().out == run["stdout"], run["options"]
    out = str(tmp_path / "probes.fasta")
    pb = design_naively.main(design_naively.parse_args([fasta, "-dsf", "3", "80", "-o", out]))
    count = next(r["count"] for r in runs if r["options"] == ["-dsf", "3", "80"])
    assert capsys.readouterr().out == "%d\n" % count
    written = [str(s) for s in seq_io.read_fasta(out).values()]
    assert written == [p.seq_str for p in pb.final_probes] and len(written) == count
    design_naively.main(design_naively.parse_args([fasta, "-nrf", "3", "80", "--print-analysis", "--limit-target-genomes", "2"]))
    text = capsys.readouterr().out
    assert re.search(r"NUMBER OF PROBES: \d+", text) and "Genome" in text
