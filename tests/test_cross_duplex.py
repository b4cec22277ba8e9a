"""Cross-dimer dG (catch_amd/filter/cross_duplex.py, csrc/duplex.hip): the definition, its two properties and the NumPy
host path without a GPU; the four C entries against the NumPy form on the GPU.  Every comparison is of exact integers.
The design commands are in test_cross_duplex_design.py."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RC = str.maketrans("ACGT", "TGCA")

# the worked values of the specification
WORKED = [
    ("ACGT", "ACGT", 144 + 217 + 144 - 206, 299),
    ("AAAA", "TTTT", 300 - 206, 94),
    ("GCGC", "GCGC", 665 - 196, 469),
    ("AAAA", "AAAA", 0, 0),
    ("TA", "TA", 0, 0),                                   # (it would be 58 - 206 = -148)
    ("AT" * 8, "AT" * 8, 8 * 88 + 7 * 58 - 206, 904),
    ("GC" * 5, "GC" * 5, 5 * 224 + 4 * 217 - 196, 1792),
]


def _rc(s):
    return s[::-1].translate(_RC)


def _cx():
    from catch_amd.filter import cross_duplex
    return cross_duplex


def _random(rng, length, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=length)) if length else ""


def _walk(matrix, above):
    """The sequential walk over a duplex matrix: keep[i] iff no kept j < i has duplex > above."""
    keep = []
    for i in range(matrix.shape[0]):
        keep.append(not any(keep[j] and matrix[i, j] > above for j in range(i)))
    return np.array(keep, dtype=bool)


def _of_matrix(matrix):
    """(values, partners) of a square duplex matrix with a zero diagonal, or of a rectangular one."""
    if matrix.shape[0] == 0 or matrix.shape[1] == 0:
        return np.zeros(matrix.shape[0], np.int32), np.full(matrix.shape[0], -1, np.int32)
    values = matrix.max(axis=1)
    return values, np.where(values > 0, matrix.argmax(axis=1), -1)


# ------------------------------------------------------------------ without a GPU
def test_definition_gives_the_worked_values():
    cx = _cx()
    for s, t, by_hand, want in WORKED:
        assert by_hand == want
        assert cx.duplex(s, t) == want == cx.duplex(t, s)
        v, p = cx.dcross_numpy([s, t])
        assert v.tolist() == [want, want] and p.tolist() == ([1, 0] if want else [-1, -1])
    assert cx.stab("ACGT", 0, 4) == 299 and cx.stab("TA", 0, 2) == -148
    # ten GC pairs hold about twice as firmly as sixteen AT pairs: length is the wrong unit
    assert cx.duplex("GC" * 5, "GC" * 5) > 1.9 * cx.duplex("AT" * 8, "AT" * 8)
    assert cx.dcross_list(["ACGT"]) == ([0], [-1]) and cx.dcross_list([]) == ([], [])
    assert cx.cross_duplex_against("ACGT", []) == (0, -1)
    assert cx.cross_duplex_against("GCGC", ["AAAA", "GCGC", "GCGC"]) == (469, 1)
    # the table: 16 dinucleotides, symmetric under reverse complement; the derived bound
    assert len(cx.DG) == 16 and all(cx.DG[d] == cx.DG[_rc(d)] for d in cx.DG)
    assert min(cx.DG.values()) == -224 and max(cx.DG.values()) == -58 and min(cx.TERM.values()) == 98


def _stretches(s, t):
    """Every stretch (a, b, n) of s and t with its stab, and whether it is maximal."""
    cx = _cx()
    pairs = lambda x, y: 0 <= x < len(s) and 0 <= y < len(t) and s[x] in "ACGT" and _rc(s[x]) == t[y]    # noqa: E731
    out = []
    for a in range(len(s)):
        for b in range(len(t)):
            n = 0
            while pairs(a + n, b - n):
                n += 1
                if n >= 2:
                    out.append((cx.stab(s, a, n), not pairs(a - 1, b + 1) and not pairs(a + n, b - n)))
    return out


def test_duplex_is_symmetric_and_reached_by_a_maximal_stretch():
    cx = _cx()
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(400):
        s = _random(rng, int(rng.integers(0, 13)), "ACGTNa")
        t = _random(rng, int(rng.integers(0, 13)), "ACGTNa")
        if rng.integers(0, 2) and len(s) >= 3:            # half of them with something to find
            k = int(rng.integers(2, len(s)))
            t = (t + _rc(s[:k]))[-12:]
        v = cx.duplex(s, t)
        assert v == cx.duplex(t, s)
        all_ = _stretches(s, t)
        assert v == max([x for x, _m in all_] + [0])
        if v > 0:
            assert v == max(x for x, m in all_ if m)
            seen += 1
    assert seen >= 40
    # the bound the kernel aims by: n pairs give at most 224 (n - 1) - 196
    for n in range(2, 12):
        assert cx.stab("GC" * 6, 0, n) <= 224 * (n - 1) - 196


def _forty(rng):
    seqs = [_random(rng, int(rng.integers(0, 31)), "ACGTNa") for _ in range(34)]
    long = _random(rng, 24)
    seqs[3] = long                                        # a record and its reverse complement
    seqs[17] = _rc(long)
    seqs[20] = _rc(long[:12]) + "N" + _rc(long)[13:]      # an N in the middle of a long stretch
    seqs[8] = seqs[25] = _random(rng, 20)                 # duplicates
    return seqs + ["A", "", seqs[3], "GC" * 6, "AT" * 9, ""]


def test_numpy_form_equals_the_definition():
    cx = _cx()
    seqs = _forty(np.random.default_rng(11))
    assert len(seqs) == 40 and "" in seqs and "A" in seqs and max(len(s) for s in seqs) <= 30
    want_v, want_p = cx.dcross_list(seqs)
    got_v, got_p = cx.dcross_numpy(seqs)
    assert got_v.dtype == got_p.dtype == np.int32
    assert got_v.tolist() == want_v and got_p.tolist() == want_p
    assert want_v[3] == cx.stab(seqs[3], 0, 24) and want_p[3] == 17 and want_p[17] == 3 and want_p[36] == 17
    assert 0 < want_v[20] < want_v[3]
    m = cx.duplex_matrix(seqs)
    assert m.tolist() == [[0 if i == j else cx.duplex(s, t) for j, t in enumerate(seqs)] for i, s in enumerate(seqs)]
    assert (m == m.T).all()
    # one list against another, the walk and the flags
    bs = seqs[:7] + ["", "GC" * 6]
    v, p = cx.against_numpy(bs, seqs)
    assert (v.tolist(), p.tolist()) == tuple(map(list, zip(*[cx.cross_duplex_against(b, seqs) for b in bs])))
    assert v[3] == cx.duplex(seqs[3], seqs[17]) and p[3] == 17
    for above in (0, 300, int(m.max()) - 1, int(m.max())):
        assert cx.walk(seqs, above).tolist() == _walk(m, above).tolist()
    assert cx.walk(seqs, int(m.max())).all() and not cx.walk(seqs, 0).all()
    for seqs in ([], ["ACGT"], ["", ""], ["", "ACGT", ""]):
        v, p = cx.dcross_numpy(seqs)
        assert (v.tolist(), p.tolist()) == cx.dcross_list(seqs)
    assert cx.against_numpy(["ACGT"], [])[0].tolist() == [0] and cx.against_numpy([], ["ACGT"])[0].size == 0


def _inserts():
    """A probe that holds (AT)8 and (GC)5; one record pairs with the first, a later one with the second."""
    rng = np.random.default_rng(4)
    probe = "CACACA" + "AT" * 8 + "CACACA" + "GC" * 5 + "CACACA"
    return [probe, "TCTCTC" + "AT" * 8 + "TCTCTC", "TCTCTC" + "GC" * 5 + "TCTCTC", _random(rng, 30, "ACT")]


def test_length_and_energy_name_different_partners():
    cx = _cx()
    from catch_amd.filter import cross_dimer
    seqs = _inserts()
    runs, partners = cross_dimer.cross_dimers(seqs)
    values, dpartners = cx.dcross_list(seqs)
    assert runs[0] == 17 and partners[0] == 1             # the longest stretch is the AT one (and the A in front)
    assert dpartners[0] == 2 and values[0] >= 1792 > cx.duplex(seqs[0], seqs[1]) >= 904      # the firmest is the GC one
    got_v, got_p = cx.dcross_numpy(seqs)
    assert got_v.tolist() == values and got_p.tolist() == dpartners
    # a length threshold of 12 bans the weak pair and lets the firm one through; an energy threshold does the opposite
    assert cross_dimer.walk(seqs, 12).tolist() == [True, False, True, True]
    assert cx.walk(seqs, 1500).tolist() == [True, True, False, True]


def test_ties_go_to_the_smallest_index():
    cx = _cx()
    piece = "GATTACAGGC"
    seqs = ["TTTT" + piece, _rc(piece) + "TTTT", "CCCC" + _rc(piece), _rc(piece)]
    values, partners = cx.dcross_list(seqs)
    assert values[0] == cx.stab(piece, 0, 10) and partners == [1, 0, 0, 0]
    v, p = cx.dcross_numpy(seqs)
    assert v.tolist() == values and p.tolist() == partners
    assert cx.cross_duplex_against(seqs[0], seqs[1:]) == (values[0], 0)
    assert cx.against_numpy([seqs[0]], seqs[:0:-1])[1].tolist() == [0]


@pytest.mark.parametrize("text, want", [("0", 0), ("17.92", 1792), ("17.929", 1792), ("9/2", 450), ("600", 60000), (12, 1200)])
def test_threshold_is_read_exactly(text, want):
    assert _cx().threshold(text) == want


@pytest.mark.parametrize("bad", [-1, "-0.01", "600.01", 2.5, "x", None, True])
def test_threshold_refuses(bad):
    cx = _cx()
    with pytest.raises(ValueError):
        cx.threshold(bad)
    from catch_amd.filter import cross_dimer
    with pytest.raises(ValueError):
        cross_dimer.CrossDimerFilter(max_cross_dimer_dg=bad)
    with pytest.raises(ValueError):
        cross_dimer.CrossDimerFilter(20, max_cross_dimer_dg="10")


def test_filter_on_the_host_path_is_the_sequential_walk(monkeypatch):
    cx = _cx()
    from catch_amd.filter import cross_dimer
    from catch_amd.probe import Probe
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    seqs = _inserts()
    m = cx.duplex_matrix(seqs)
    f = cross_dimer.CrossDimerFilter(max_cross_dimer_dg="15")
    kept = f.filter([Probe.from_str(s) for s in seqs])
    assert [p.seq_str for p in kept] == [seqs[0], seqs[1], seqs[3]]
    assert (f.dropped, f.seen, f.max_cross_dimer) == (1, 4, None)
    assert f.largest_before == int(m.max()) and f.largest_after == int(m[np.ix_([0, 1, 3], [0, 1, 3])].max())
    assert len(cross_dimer.CrossDimerFilter(max_cross_dimer_dg="600").filter([Probe.from_str(s) for s in seqs])) == 4
    v, p = cx.measure(seqs)
    assert (v.tolist(), p.tolist()) == cx.dcross_list(seqs)
    assert cx.measure_against(seqs[:2], seqs)[0].tolist() == [max(cx.duplex(s, t) for t in seqs) for s in seqs[:2]]
    # ((GC)5 is its own reverse complement: against a panel nothing is exempted, record 2 pairs with its equal)
    assert cx.flags_against(seqs, [seqs[2]], 1500).tolist() == [True, False, True, False]


def test_third_header_third_table_library_and_makefile():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "catchhip_duplex.h")).read()
    declared = set(re.findall(r"\b(catchhip_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"catchhip_cross_duplex", "catchhip_cross_duplex_graph", "catchhip_cross_duplex_against",
                        "catchhip_cross_duplex_against_flags"} == set(_lib.DUPLEX_PROTOTYPES)
    assert not declared & (set(_lib.PROTOTYPES) | set(_lib.CROSS_PROTOTYPES) | set(_lib.REDESIGN_PROTOTYPES))
    L = _lib.lib()
    for name, (res, args) in _lib.DUPLEX_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "duplex.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()


# ------------------------------------------------------------------ on the GPU
SIZES = (1, 2, 63, 64, 65, 130)
# (i, j, the piece): pairs on a diagonal tile, in tiles 0 and 1, 0 and 2, 1 and 2; GC-rich, AT-rich and mixed pieces
_PLANTS = ((3, 40, "GC" * 9), (5, 70, "AT" * 14), (66, 100, None), (7, 129, None), (64, 128, "GGGCCC" * 3), (10, 11, None),
           (60, 61, "ATTA" * 5))
_shared = {}


def _planted(rng, lens, plants, alphabet):
    seqs = [_random(rng, n, alphabet) for n in lens]
    for i, j, piece in plants:
        k = len(piece) if piece else int(rng.integers(8, 1 + min(lens[i], lens[j], 40)))
        piece = piece or _random(rng, k)
        assert k <= min(lens[i], lens[j])
        oi, oj = int(rng.integers(0, lens[i] - k + 1)), int(rng.integers(0, lens[j] - k + 1))
        seqs[i] = seqs[i][:oi] + piece + seqs[i][oi + k:]
        seqs[j] = seqs[j][:oj] + _rc(piece) + seqs[j][oj + k:]
    assert [len(s) for s in seqs] == list(lens)
    return seqs


def _master():
    """130 records of at most 64 characters (W = 1) with 5 % N and some lower case, and their duplex matrix."""
    if "m" not in _shared:
        rng = np.random.default_rng(20261021)
        lens = [int(rng.choice((0, 1, 2, 31, 32, 33, 63, 64, 64, 64))) for _ in range(130)]
        for i, j, _piece in _PLANTS:
            lens[i] = lens[j] = 64 if i % 2 else 63
        seqs = _planted(rng, lens, _PLANTS, list("ACGT") * 23 + ["N"] * 5 + ["a", "c", "g"])
        seqs[20] = seqs[3]                                  # a duplicate: the smaller index is the partner
        m = _cx().duplex_matrix(seqs)
        assert m[3, 40] >= 9 * 224 + 8 * 217 - 196 and m[5, 70] >= 14 * 88 + 13 * 58 - 206
        _shared["m"] = (seqs, m)
    return _shared["m"]


def _mixed(longest):
    """About two dozen records of mixed lengths up to `longest` (128: W = 2; 256: W = 4) and their duplex matrix: runs
    that cross a 64-bit word, both signs of the antidiagonal's shift."""
    if longest not in _shared:
        rng = np.random.default_rng(longest)
        pool = [x for x in (0, 1, 2, 63, 64, 65, 100, 128, 129, 255, 256) if x <= longest]
        lens = pool + [int(rng.choice(pool[3:])) for _ in range(22 - len(pool))]
        lens[-1] = lens[-2] = longest
        order = rng.permutation(len(lens))
        lens = [lens[k] for k in order]
        big = [k for k, n in enumerate(lens) if n >= 63]
        plants = [(big[0], big[1], None), (big[2], big[-1], "GC" * 20 + "AT" * 11), (big[3], big[4], None)]
        seqs = _planted(rng, lens, plants, list("ACGT") * 23 + ["N"] * 5 + ["a", "c", "g"])
        # a stretch of 60 pairs from 40 characters in: it crosses the first word edge in one record and sits at the
        # start of the other
        a, b = [k for k, n in enumerate(lens) if n == longest][:2]
        piece = _random(rng, 60)
        seqs[a] = seqs[a][:40] + piece + seqs[a][100:]
        seqs[b] = _rc(piece) + seqs[b][60:]
        _shared[longest] = (seqs, _cx().duplex_matrix(seqs))
    return _shared[longest]


def _check_values(engine, ctx, seqs, m):
    want_v, want_p = _of_matrix(m)
    values, partners = engine.cross_duplex(ctx, seqs)
    assert values.dtype == partners.dtype == np.int32
    wrong = [(i, int(values[i]), int(partners[i]), int(want_v[i]), int(want_p[i])) for i in range(len(seqs))
             if values[i] != want_v[i] or partners[i] != want_p[i]]
    assert not wrong, wrong[:10]
    again = engine.cross_duplex(ctx, seqs)                  # the same call again: the same bytes
    assert again[0].tobytes() == values.tobytes() and again[1].tobytes() == partners.tobytes()


@pytest.mark.gpu
def test_device_gives_the_worked_values(ctx):
    from catch_amd import engine
    for s, t, _hand, want in WORKED:
        values, partners = engine.cross_duplex(ctx, [s, t])
        assert values.tolist() == [want, want] and partners.tolist() == ([1, 0] if want else [-1, -1])
    seqs = _inserts()
    values, partners = engine.cross_duplex(ctx, seqs)
    assert (values.tolist(), partners.tolist()) == _cx().dcross_list(seqs)
    assert partners[0] == 2 and engine.cross_dimer(ctx, seqs)[1][0] == 1
    v, p = engine.cross_duplex(ctx, [])
    assert v.size == p.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_numpy_form_at_tile_edges(ctx, n):
    from catch_amd import engine
    seqs, m = _master()
    _check_values(engine, ctx, seqs[:n], m[:n, :n])


@pytest.mark.gpu
@pytest.mark.parametrize("longest", [128, 256])
def test_device_equals_the_numpy_form_at_mixed_lengths(ctx, longest):
    from catch_amd import engine
    seqs, m = _mixed(longest)
    assert max(len(s) for s in seqs) == longest and m.max() >= 60 * 58 - 206
    _check_values(engine, ctx, seqs, m)
    v, p = _cx().measure(seqs)
    assert (v.tolist(), p.tolist()) == tuple(x.tolist() for x in _of_matrix(m))


def _extremes():
    if "x" not in _shared:
        seqs = ["GC" * 128, "AT" * 128, "A" * 256, "GC" * 128, "T" * 256, "G" * 200, "C" * 256, "AT" * 128, "a" * 50,
                "N" * 256, "acgt" * 10 + "ACGT", "ACGTNACGT" * 20]
        _shared["x"] = (seqs, _cx().duplex_matrix(seqs))
    return _shared["x"]


@pytest.mark.gpu
def test_one_base_repeated_the_gc_and_at_extremes_lower_case_and_n(ctx):
    from catch_amd import engine
    seqs, m = _extremes()
    assert m[0, 3] == 128 * 224 + 127 * 217 - 196 == m.max()         # the largest value 256 characters give
    assert m[1, 7] == 128 * 88 + 127 * 58 - 206 and m[2, 4] == 255 * 100 - 206 and m[5, 6] == 199 * 184 - 196
    assert m[8].max() == 0 == m[9].max() and m[10].max() > 0
    _check_values(engine, ctx, seqs, m)
    for above in (int(m.max()), int(m.max()) - 1, 0):
        g = engine.RedundancyGraph.cross_duplex(ctx, seqs, above)
        try:
            assert _edges(*g.fetch()) == {(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if m[i, j] > above}
        finally:
            g.close()


def _edges(ptr, idx):
    return {(i, int(j)) for i in range(len(ptr) - 1) for j in idx[ptr[i]:ptr[i + 1]]}


def _check_graph(engine, ctx, seqs, m, above):
    n = len(seqs)
    g = engine.RedundancyGraph.cross_duplex(ctx, seqs, above)
    try:
        ptr, idx = g.fetch()
        want = {(i, j) for i in range(n) for j in range(n) if m[i, j] > above}
        assert g.n == n and g.nedges == len(want) == int(ptr[-1]) == idx.size
        assert _edges(ptr, idx) == want
        for i in range(n):
            assert (np.diff(idx[ptr[i]:ptr[i + 1]].astype(np.int64)) > 0).all()
        assert g.naive().tolist() == _walk(m, above).tolist()
        return want, g.naive()
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["master", 128, 256])
def test_graph_equals_the_numpy_form_at_and_below_an_occurring_value(ctx, which):
    from catch_amd import engine
    seqs, m = _master() if which == "master" else _mixed(which)
    i, j = (5, 70) if which == "master" else np.unravel_index(int(m.argmax()), m.shape)
    v = int(m[i, j])
    at, _keep = _check_graph(engine, ctx, seqs, m, v)
    assert (i, j) not in at                                # exactly the value: no conflict
    below, keep = _check_graph(engine, ctx, seqs, m, v - 1)
    assert (i, j) in below and (j, i) in below
    zero, _keep = _check_graph(engine, ctx, seqs, m, 0)
    assert len(zero) == int(np.count_nonzero(m)) > len(below)
    if which == "master":
        assert keep.tolist() == _cx().walk(seqs, v - 1).tolist()
        median = int(np.median(m[m > 0]))
        _check_graph(engine, ctx, seqs, m, median)


@pytest.mark.gpu
def test_graph_of_nothing_and_of_one(ctx):
    from catch_amd import engine
    g = engine.RedundancyGraph.cross_duplex(ctx, [], 0)
    try:
        ptr, idx = g.fetch()
        assert (g.n, g.nedges, ptr.tolist(), idx.size) == (0, 0, [0], 0) and g.naive().tolist() == []
    finally:
        g.close()
    g = engine.RedundancyGraph.cross_duplex(ctx, ["ACGT" * 25], 0)
    try:
        assert (g.n, g.nedges) == (1, 0) and g.naive().tolist() == [True]
    finally:
        g.close()


def _two_lists():
    """B: 200 records, A: the master's 130, and the 200 x 130 matrix duplex(b, a)."""
    if "ba" not in _shared:
        cx = _cx()
        a_seqs, _m = _master()
        rng = np.random.default_rng(77)
        b_seqs = [_random(rng, int(rng.choice((0, 1, 2, 33, 63, 64))), list("ACGT") * 23 + ["N"] * 5 + ["a"]) for _ in range(200)]
        for b, a in ((0, 3), (63, 70), (64, 0), (65, 129), (199, 64), (100, 128)):
            k = min(len(a_seqs[a]), 30)
            b_seqs[b] = (_rc(a_seqs[a][:k]) + _random(rng, 64))[:64]
        b_seqs[150] = a_seqs[5]                             # an equal record is a partner like any other
        from catch_amd.filter import cross_dimer
        m = cx.duplex_rows(cross_dimer._digits(b_seqs), cross_dimer._digits(a_seqs))
        _shared["ba"] = (b_seqs, a_seqs, m)
    return _shared["ba"]


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [0, 1, 64, 65, 200])
def test_two_lists_equal_the_numpy_form(ctx, nb):
    from catch_amd import engine
    b_seqs, a_seqs, m = _two_lists()
    for na in (0, 1, 64, 65, 130):
        sub = m[:nb, :na]
        want_v, want_p = _of_matrix(sub)
        values, partners = engine.cross_duplex_against(ctx, b_seqs[:nb], a_seqs[:na])
        assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist(), (nb, na)
        if nb and na:
            v = int(sub.max())
            for above in sorted({v, max(v - 1, 0), 0, int(np.median(sub.max(axis=1)))}):
                flags = engine.cross_duplex_against_flags(ctx, b_seqs[:nb], a_seqs[:na], above)
                assert flags.dtype == bool and flags.tolist() == (want_v > above).tolist(), (nb, na, above)
        else:
            assert engine.cross_duplex_against_flags(ctx, b_seqs[:nb], a_seqs[:na], 0).tolist() == [False] * nb
    if nb == 200:
        cx = _cx()
        assert int(m[150, 5]) == cx.duplex(a_seqs[5], a_seqs[5])      # an equal record: the record's own pairing
        v, p = cx.measure_against(b_seqs, a_seqs)
        assert (v.tolist(), p.tolist()) == tuple(x.tolist() for x in _of_matrix(m))
        assert cx.flags_against(b_seqs, a_seqs, 900).tolist() == (m.max(axis=1) > 900).tolist()


@pytest.mark.gpu
def test_two_lists_of_long_records(ctx):
    from catch_amd import engine
    cx = _cx()
    from catch_amd.filter import cross_dimer
    seqs, _m = _mixed(256)
    short, _m1 = _master()
    bs, as_ = seqs[:9] + short[:3], seqs[5:]
    m = cx.duplex_rows(cross_dimer._digits(bs), cross_dimer._digits(as_))
    want_v, want_p = _of_matrix(m)
    values, partners = engine.cross_duplex_against(ctx, bs, as_)
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()
    v = int(m.max())
    for above in (v, v - 1, 0):
        assert engine.cross_duplex_against_flags(ctx, bs, as_, above).tolist() == (want_v > above).tolist()


@pytest.mark.gpu
def test_refusals(ctx):
    from catch_amd import engine
    rng = np.random.default_rng(2)
    long = _random(rng, 257)
    seqs = [_random(rng, 40), long, _random(rng, 64)]
    for call in (lambda: engine.cross_duplex(ctx, seqs),
                 lambda: engine.RedundancyGraph.cross_duplex(ctx, seqs, 100),
                 lambda: engine.cross_duplex_against(ctx, seqs, seqs[:1]),
                 lambda: engine.cross_duplex_against(ctx, seqs[:1], seqs),
                 lambda: engine.cross_duplex_against_flags(ctx, seqs, seqs[:1], 100)):
        with pytest.raises(ValueError, match="257 characters.*at most 256"):
            call()
    with pytest.raises(ValueError, match="at least 0"):
        engine.RedundancyGraph.cross_duplex(ctx, seqs[:1], -1)
    with pytest.raises(ValueError, match="at least 0"):
        engine.cross_duplex_against_flags(ctx, seqs[:1], seqs[:1], -1)
    # 256 is taken, 0 is a threshold
    values, partners = engine.cross_duplex(ctx, [long[:256], _rc(long[:256])])
    assert values.tolist() == [_cx().stab(long, 0, 256)] * 2 and partners.tolist() == [1, 0]
    # decreasing offsets, and more records than one call pairs (refused from the sizes alone)
    u8p, i64p, i32p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int64, ctypes.c_int32))
    buf = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8).copy()
    out = np.zeros(4, dtype=np.int32)
    off = np.array([0, 8, 4, 12], dtype=np.int64)
    rc = ctx._L.catchhip_cross_duplex(ctx._h, buf.ctypes.data_as(u8p), off.ctypes.data_as(i64p), 3,
                                      out.ctypes.data_as(i32p), out.ctypes.data_as(i32p))
    assert rc == -1 and b"decrease" in ctx._L.catchhip_last_error()
    n = (1 << 20) + 1
    off = np.zeros(n + 1, dtype=np.int64)
    rc = ctx._L.catchhip_cross_duplex(ctx._h, buf.ctypes.data_as(u8p), off.ctypes.data_as(i64p), n,
                                      out.ctypes.data_as(i32p), out.ctypes.data_as(i32p))
    assert rc == -1 and b"1048576" in ctx._L.catchhip_last_error()
    # a longer record goes to the host path
    v, p = _cx().measure(seqs + [_rc(long[100:140])])
    assert int(v[1]) == _cx().stab(long, 100, 40) and int(p[1]) == 3


@pytest.mark.gpu
def test_all_four_entries_on_poisoned_memory(ctx, monkeypatch):
    from catch_amd import engine
    seqs, m = _master()
    want_v, want_p = _of_matrix(m)
    above = int(m[5, 70]) - 1
    want_edges = {(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if m[i, j] > above}
    b_seqs, a_seqs, ba = _two_lists()
    outs = {}
    for poison in (None, 255, 85):
        # (set before the context is created: its first blocks are poisoned too)
        if poison is None:
            monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
        else:
            monkeypatch.setenv("CATCHHIP_POOL_POISON", str(poison))
        c = engine.Context(ctx.device)
        try:
            values, partners = engine.cross_duplex(c, seqs)
            g = engine.RedundancyGraph.cross_duplex(c, seqs, above)
            try:
                ptr, idx = g.fetch()
                keep = g.naive()
            finally:
                g.close()
            av, ap = engine.cross_duplex_against(c, b_seqs, a_seqs)
            flags = engine.cross_duplex_against_flags(c, b_seqs, a_seqs, above)
        finally:
            c.close()
        outs[poison] = tuple(x.tobytes() for x in (values, partners, ptr, idx, keep, av, ap, flags))
        assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist(), poison
        assert _edges(ptr, idx) == want_edges, poison
        assert (av.tolist(), ap.tolist()) == tuple(x.tolist() for x in _of_matrix(ba)), poison
        assert flags.tolist() == (ba.max(axis=1) > above).tolist(), poison
    monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
    assert outs[None] == outs[255] == outs[85]
