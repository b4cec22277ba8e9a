"""catchhip_rows_union (csrc/union.hip, engine.Rows.union): the union of two row tables, set by set.

The model is plain Python: per (set, universe) the ranges of both tables sorted and merged (overlapping or touching
ranges become one), the result sorted by (set, universe, start) -- _normalise of tests/test_extend_probes.py."""
import os
import re

import numpy as np
import pytest

from test_extend_probes import _from_host, _normalise, _random_ranges, _table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ host model
def _model_union(a, b):
    """(set, universe, start, end) tables in -> the rows of the union as a list of tuples, gain0 per set, the
    longest row."""
    by = {}
    for tab in (a, b):
        for i, u, s, t in zip(*tab):
            by.setdefault((int(i), int(u)), []).append((int(s), int(t)))
    rows = [(i, u, s, t) for (i, u) in sorted(by) for s, t in _normalise(by[(i, u)])]
    nsets = 1 + max((r[0] for r in rows), default=-1)
    gain0 = np.zeros(nsets, dtype=np.int64)
    for i, _u, s, t in rows:
        gain0[i] += t - s
    return rows, gain0, max((t - s for _i, _u, s, t in rows), default=0)


def _instance(rng, max_sets=14, max_len=120):
    """Two tables over 1-4 universes of 1-max_len bases: up to max_sets sets, up to 4 ranges per (set, universe) in
    each table (the manner of test_extend_probes._instance)."""
    nuniv = int(rng.integers(1, 5))
    nsets = int(rng.integers(1, max_sets + 1))
    glen = [int(rng.integers(1, max_len + 1)) for _ in range(nuniv)]
    tabs = []
    for _ in range(2):
        rows = []
        for i in range(nsets):
            for u in range(nuniv):
                if rng.random() < 0.7:
                    rows += [(i, u, s, t) for s, t in _random_ranges(rng, glen[u], 4)]
        tabs.append(_table(rows))
    return glen, tabs[0], tabs[1]


def _check_union(ctx, a, b, glen, tag):
    """The device's union of a and b against the model: rows, gain0, the longest row.  Returns the model's rows."""
    A, B = _from_host(ctx, a, glen), _from_host(ctx, b, glen)
    try:
        U = A.union(B)
        try:
            want, gain0, longest = _model_union(a, b)
            got = U.fetch()
            assert U.n == len(want), (tag, U.n, len(want))
            got_rows = [tuple(int(x[i]) for x in got) for i in range(U.n)]
            assert got_rows == want, tag
            held = U.fetch_gain0(max(gain0.size, 1))
            if a[0].size and b[0].size:
                # both inputs carry gain0: summed again from the result, sized to the larger of the two
                assert held is not None and held.size == gain0.size, tag
                assert np.array_equal(held.astype(np.int64), gain0), tag
            elif U.n:
                assert np.array_equal(held.astype(np.int64), gain0), tag
            assert U.longest() == longest, tag
            return want
        finally:
            U.close()
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ without a GPU
def test_symbol_is_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_union\s*\(", hdr)
    assert "catchhip_rows_union" in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["catchhip_rows_union"] == _lib.PROTOTYPES["catchhip_rows_subtract"]
    assert callable(engine.Rows.union)
    assert re.search(r"\bint catchhip_rows_longest\s*\(", hdr) and len(_lib.PROTOTYPES["catchhip_rows_longest"][1]) == 2
    assert callable(engine.Rows.longest)
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "union.hip" in mk


def test_model_merges_touching_ranges_inside_a_set_and_universe_only():
    a = _table([(0, 0, 0, 5), (0, 1, 0, 3), (2, 0, 1, 2)])
    b = _table([(0, 0, 5, 9), (0, 0, 20, 30), (1, 0, 2, 3)])
    rows, gain0, longest = _model_union(a, b)
    assert rows == [(0, 0, 0, 9), (0, 0, 20, 30), (0, 1, 0, 3), (1, 0, 2, 3), (2, 0, 1, 2)]
    assert gain0.tolist() == [22, 1, 1] and longest == 10


# ------------------------------------------------------------------ on the device
def _directed_cases():
    """name -> (universe lengths, rows of a, rows of b), rows as (set, universe, start, end)."""
    many = [(0, 0, s, s + 3) for s in range(10, 4000, 7)]
    return {
        "a empty": ([300], [], [(0, 0, 10, 50), (3, 0, 20, 30)]),
        "b empty": ([300], [(0, 0, 10, 50), (3, 0, 20, 30)], []),
        "both empty": ([300], [], []),
        "equal tables": ([300, 40], [(0, 0, 10, 50), (0, 0, 60, 61), (1, 1, 0, 40), (4, 0, 299, 300)],
                         [(0, 0, 10, 50), (0, 0, 60, 61), (1, 1, 0, 40), (4, 0, 299, 300)]),
        "sets only in a, only in b, ids with gaps": (
            [300], [(2, 0, 10, 50), (9, 0, 0, 5), (40, 0, 7, 8)], [(5, 0, 20, 30), (9, 0, 3, 9), (77, 0, 100, 200)]),
        "equal starts with different ends, equal ends with different starts": (
            [300], [(0, 0, 10, 50), (0, 0, 100, 150), (1, 0, 10, 20), (1, 0, 100, 150)],
            [(0, 0, 10, 30), (0, 0, 120, 150), (1, 0, 10, 40), (1, 0, 90, 150)]),
        "a ends where b starts": ([300], [(0, 0, 10, 50), (1, 0, 70, 80)], [(0, 0, 50, 60), (1, 0, 60, 70)]),
        "end of universe u, start of u + 1": (
            [100, 100, 28], [(0, 0, 90, 100), (0, 1, 95, 100), (1, 1, 0, 7)], [(0, 1, 0, 10), (0, 2, 0, 28), (1, 0, 50, 100)]),
        "the same, the tables swapped": (
            [100, 100, 28], [(0, 1, 0, 10), (0, 2, 0, 28), (1, 0, 50, 100)], [(0, 0, 90, 100), (0, 1, 95, 100), (1, 1, 0, 7)]),
        "equal ends at a universe's last base, the next universe starts in both": (
            [100, 100], [(0, 0, 90, 100), (0, 1, 0, 5)], [(0, 0, 80, 100), (0, 1, 0, 9)]),
        "a row that ends at the last base of the coordinate space": (
            [64, 64], [(0, 1, 60, 64)], [(0, 1, 10, 61), (1, 1, 63, 64)]),
        "a row of b that spans many rows of a": ([5000], many + [(1, 0, 0, 1)], [(0, 0, 100, 3000), (1, 0, 1, 5000)]),
        "a row of a that spans many rows of b": ([5000], [(0, 0, 100, 3000), (1, 0, 1, 5000)], many + [(1, 0, 0, 1)]),
        "nested and staggered": ([300], [(0, 0, 10, 100), (0, 0, 120, 130), (0, 0, 140, 200)],
                                 [(0, 0, 20, 30), (0, 0, 40, 125), (0, 0, 126, 139), (0, 0, 210, 220)]),
    }


@pytest.mark.gpu
def test_rows_union_directed_cases(ctx):
    expected = {
        "a ends where b starts": [(0, 0, 10, 60), (1, 0, 60, 80)],
        "end of universe u, start of u + 1": [(0, 0, 90, 100), (0, 1, 0, 10), (0, 1, 95, 100), (0, 2, 0, 28),
                                              (1, 0, 50, 100), (1, 1, 0, 7)],
        "equal ends at a universe's last base, the next universe starts in both": [(0, 0, 80, 100), (0, 1, 0, 9)],
        "a row that ends at the last base of the coordinate space": [(0, 1, 10, 64), (1, 1, 63, 64)],
        "nested and staggered": [(0, 0, 10, 139), (0, 0, 140, 200), (0, 0, 210, 220)],     # (139 and 140 do not touch)
        "both empty": [],
    }
    for tag, (glen, a, b) in _directed_cases().items():
        got = _check_union(ctx, _table(a), _table(b), glen, tag)
        if tag in expected:
            assert got == expected[tag], tag
        if tag == "equal tables":
            assert got == sorted(a)
        if tag.startswith("a row of"):
            # (a's rows start at 10 + 7k: [101, 104) is the first one inside the long row, [2999, 3002) ends it)
            assert len(got) < 600 and (0, 0, 100, 3002) in got and (1, 0, 0, 5000) in got
    # two universes that touch, end to start: two rows, whichever table holds which
    for a, b in (([(0, 0, 50, 100)], [(0, 1, 0, 50)]), ([(0, 1, 0, 50)], [(0, 0, 50, 100)])):
        assert len(_check_union(ctx, _table(a), _table(b), [100, 100], "border")) == 2


@pytest.mark.gpu
def test_rows_union_random_tables(ctx):
    rng = np.random.default_rng(431)
    merged = rows_in = 0
    for case in range(200):
        glen, a, b = _instance(rng)
        got = _check_union(ctx, a, b, glen, case)
        rows_in += a[0].size + b[0].size
        merged += a[0].size + b[0].size - len(got)
    assert rows_in > 5000 and merged > 1000


def _chain(broken=()):
    """a = [4i, 4i + 3), b = [4i + 2, 4i + 5) for i < 40,000, one set, one universe of 160,005 bases; for i in
    `broken` b's row is left out, which ends a union interval at 4i + 3 (a's next row starts at 4i + 4).  Whole, the
    chain is ONE row [0, 160,001): the last row of b ends at 4 * 39,999 + 5."""
    i = np.arange(40000, dtype=np.int64)
    z = np.zeros(40000, dtype=np.int32)
    keep = ~np.isin(i, list(broken))
    return (z, z, 4 * i, 4 * i + 3), (z[keep], z[keep], (4 * i + 2)[keep], (4 * i + 5)[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("broken", [(), (63,), (64,), (255,), (256,), (20000,), (63, 64, 255, 256, 20000)])
def test_rows_union_chain_across_every_launch_edge(ctx, broken):
    """80,000 input rows whose head and tail flags are all zero but at the chain's ends: the scans carry one flag
    across every wavefront, workgroup and scan-tile edge; a broken link puts a tail and a head right at an edge."""
    from catch_amd import engine
    a, b = _chain(broken)
    A = engine.Rows.from_host(ctx, *a, [160005])
    B = engine.Rows.from_host(ctx, *b, [160005])
    try:
        for X, Y in ((A, B), (B, A)):
            U = X.union(Y)
            try:
                cuts = sorted(broken)
                want = list(zip([0] + [4 * i + 4 for i in cuts], [4 * i + 3 for i in cuts] + [160001]))
                if not broken:
                    assert want == [(0, 160001)]
                si, un, st, en = U.fetch()
                assert U.n == len(want)
                assert list(zip(st.tolist(), en.tolist())) == want
                assert not si.any() and not un.any()
                assert U.fetch_gain0(1).tolist() == [sum(t - s for s, t in want)]
                assert U.longest() == max(t - s for s, t in want)
            finally:
                U.close()
    finally:
        A.close()
        B.close()


@pytest.mark.gpu
def test_rows_union_refusals(ctx):
    """Refused: another coordinate space (an unmerged range table of a scan over other targets among them -- over the
    SAME targets chip_rows_form_check does not tell unmerged ranges from rows, as catchhip_rows_subtract cannot), and
    rows of a scan with group numbers, on either side."""
    from catch_amd import engine, probe
    R = _from_host(ctx, _table([(0, 0, 10, 50), (0, 1, 0, 5)]), [100, 50])
    held = [R]
    try:
        for glen in ([100, 51], [150], [100, 50, 1], [50, 100]):
            C = _from_host(ctx, _table([(0, 0, 1, 2)]), glen)
            held.append(C)
            for x, y in ((R, C), (C, R)):
                with pytest.raises(ValueError, match="rows_union: the two tables are not over one coordinate space"):
                    x.union(y)
        rng = np.random.default_rng(8)
        genome = "".join(rng.choice(list("ACGT"), size=400))
        strs = [genome[j:j + 60] for j in range(0, 340, 20)]
        k, uniq, owner, ep, eo = probe.anchor_table(strs, 1, 60, min_k=20, k=20)
        targets = engine.Targets(ctx, [[genome], [genome[50:300]]])
        probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
        held += [targets, probes]
        ranges = engine.Rows.scan(ctx, probes, targets, 1, 60, 0, 0, merge=False)
        held.append(ranges)
        assert ranges.n > 0
        with pytest.raises(ValueError, match="coordinate space"):
            R.union(ranges)
        gp, gt = engine.Probes(ctx, uniq, owner, ep, eo, k), engine.Targets(ctx, [[genome], [genome[50:300]]])
        held += [gp, gt]
        gp.set_groups(np.zeros(len(uniq), dtype=np.int32))
        gt.set_groups(np.zeros(2, dtype=np.int32))
        grouped = engine.Rows.scan(ctx, gp, gt, 1, 60, 0, 0)
        plain = engine.Rows.scan(ctx, probes, targets, 1, 60, 0, 0)
        held += [grouped, plain]
        with pytest.raises(ValueError, match="rows_union: the first rows come from a scan with group numbers"):
            grouped.union(plain)
        with pytest.raises(ValueError, match="rows_union: the second rows come from a scan with group numbers"):
            plain.union(grouped)
        # ... and a scan's merged rows united with themselves are themselves
        U = plain.union(plain)
        held.append(U)
        for g, w in zip(U.fetch(), plain.fetch()):
            assert np.array_equal(g, w)
    finally:
        for h in reversed(held):
            h.close()
