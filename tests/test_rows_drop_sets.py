"""engine.Rows.drop_sets (catchhip_rows_drop_sets, csrc/subtract.hip): a row table without the rows of some sets,
against NumPy on the fetched rows -- over a small table of several universes from rows_from_host and over the table of
a real scan."""
from contextlib import closing

import numpy as np
import pytest

from test_extend_probes import _candidates, _genomes

# set, universe, start, end: sets 2 and 6 have no rows; sets 0 and 3 reach into both universes
ROWS = [(0, 0, 0, 10), (0, 0, 20, 30), (0, 1, 5, 9), (1, 0, 5, 25), (3, 0, 90, 100), (3, 1, 0, 50), (4, 1, 10, 11),
        (5, 0, 0, 100), (7, 1, 49, 50)]
GLEN = [100, 50]
NSETS = 8


def _columns(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].copy(), a[:, 3].copy()


def _np_drop(table, drop):
    keep = ~np.asarray(drop, dtype=bool)[table[0]]
    return tuple(x[keep] for x in table)


def _np_gain0(table, num_sets):
    out = np.zeros(num_sets, dtype=np.int64)
    np.add.at(out, table[0], table[3] - table[2])
    return out


def _check(ctx, rows, table, num_sets, drop, greedy=True):
    """rows.drop_sets(drop) against the NumPy filter of the fetched `table`: the rows, gain0 of the surviving sets,
    the longest row, and the greedy picks against those of a rows_from_host table of the same rows."""
    from catch_amd import engine
    want = _np_drop(table, drop)
    with closing(rows.drop_sets(num_sets, drop)) as left:
        assert left.n == want[0].size and left.ngenomes == rows.ngenomes
        got = left.fetch()
        assert all(g.tolist() == w.tolist() for g, w in zip(got, want))
        gain0 = left.fetch_gain0(num_sets)
        if rows.fetch_gain0(num_sets) is not None:
            assert gain0 is not None and gain0.tolist() == _np_gain0(want, num_sets)[:gain0.size].tolist()
        assert left.longest() == (int((want[3] - want[2]).max()) if want[0].size else 0)
        if greedy:
            glen = GLEN if rows.ngenomes == len(GLEN) else None
            picks = left.greedy(num_sets)
            if glen is not None:
                with closing(engine.Rows.from_host(ctx, *want, glen)) as same:
                    assert picks == same.greedy(num_sets)
            return picks, want
    return None, want


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "without_rows"])
def test_small_table_of_two_universes(ctx, pattern):
    from catch_amd import engine
    table = _columns(ROWS)
    drop = {"none": np.zeros(NSETS, bool), "all": np.ones(NSETS, bool), "alternating": np.arange(NSETS) % 2 == 0,
            "without_rows": np.isin(np.arange(NSETS), (2, 6))}[pattern]
    with closing(engine.Rows.from_host(ctx, *table, GLEN)) as rows:
        picks, want = _check(ctx, rows, table, NSETS, drop)
        if pattern in ("none", "without_rows"):
            assert want[0].size == len(ROWS) and picks == rows.greedy(NSETS) == [5, 3]
        if pattern == "all":
            assert want[0].size == 0 and picks == []
        if pattern == "alternating":
            assert sorted(set(want[0].tolist())) == [1, 3, 5, 7] and picks == [5, 3]
        # the table it came from is what it was
        assert all(g.tolist() == w.tolist() for g, w in zip(rows.fetch(), table))


@pytest.mark.gpu
def test_flag_arrays_of_another_length_are_refused(ctx):
    from catch_amd import engine
    table = _columns(ROWS)
    with closing(engine.Rows.from_host(ctx, *table, GLEN)) as rows:
        for n in (NSETS - 1, NSETS + 1, 0):
            with pytest.raises(ValueError, match="flags for %d sets" % NSETS):
                rows.drop_sets(NSETS, np.zeros(n, bool))
        # fewer flags than the set ids of the rows: the library refuses what the binding lets through
        with pytest.raises(ValueError, match="set id is not below the 7 flags"):
            rows.drop_sets(NSETS - 1, np.zeros(NSETS - 1, bool))
        with pytest.raises(ValueError, match="set id is not below the 0 flags"):
            rows.drop_sets(0, np.zeros(0, bool))
        # more flags than sets with rows are flags of sets without rows
        with closing(rows.drop_sets(NSETS + 5, np.zeros(NSETS + 5, bool))) as left:
            assert all(g.tolist() == w.tolist() for g, w in zip(left.fetch(), table))
    with closing(engine.Rows.from_host(ctx, *_columns([]), GLEN)) as empty:
        with closing(empty.drop_sets(0, np.zeros(0, bool))) as left:
            assert left.n == 0 and left.greedy(0) == []


@pytest.mark.gpu
def test_subtract_and_below_depth_take_the_result(ctx):
    from catch_amd import engine
    table = _columns(ROWS)
    drop = np.isin(np.arange(NSETS), (5, 4))
    want = _np_drop(table, drop)
    with closing(engine.Rows.from_host(ctx, *table, GLEN)) as rows, \
            closing(engine.Rows.from_host(ctx, *want, GLEN)) as same, \
            closing(engine.Rows.from_host(ctx, *_columns([(0, 0, 8, 22), (0, 1, 0, 6)]), GLEN)) as covered, \
            closing(rows.drop_sets(NSETS, drop)) as left:
        with closing(left.subtract(covered)) as a, closing(same.subtract(covered)) as b:
            assert a.n == b.n > 0 and all(x.tolist() == y.tolist() for x, y in zip(a.fetch(), b.fetch()))
            assert a.fetch_gain0(NSETS).tolist() == b.fetch_gain0(NSETS).tolist()
            assert a.greedy(NSETS) == b.greedy(NSETS)
        (a, reached_a), (b, reached_b) = left.below_depth(NSETS, [3], 1), same.below_depth(NSETS, [3], 1)
        with closing(a), closing(b):
            assert a.n == b.n > 0 and all(x.tolist() == y.tolist() for x, y in zip(a.fetch(), b.fetch()))
            assert reached_a.tolist() == reached_b.tolist() == [10, 50]
            assert a.greedy(NSETS) == b.greedy(NSETS)
        # dropping twice is dropping the union
        with closing(left.drop_sets(NSETS, np.arange(NSETS) == 0)) as twice:
            assert all(x.tolist() == y.tolist() for x, y in zip(twice.fetch(), _np_drop(table, drop | (np.arange(NSETS) == 0))))


@pytest.mark.gpu
def test_table_of_a_real_scan(ctx):
    """The candidates of two Ebola genomes at 2 mismatches and extension 50: a few hundred sets, rows of several
    universes per set.  What is left solves like the rows_from_host table of the same rows."""
    from catch_amd import engine, probe
    genomes = _genomes(2)
    strs = _candidates(genomes)
    n = len(strs)
    k, uniq, _owner, ep, eo = probe.anchor_table(strs, 2, 100, min_k=20, k=20)
    assert uniq == list(strs) and n > 300
    glen = [sum(len(s) for s in g.seqs) for g in genomes]
    rng = np.random.default_rng(4)
    with closing(engine.Targets(ctx, [g.seqs for g in genomes])) as targets, \
            closing(engine.Probes(ctx, uniq, np.arange(n, dtype=np.int32), ep, eo, k)) as probes, \
            closing(engine.Rows.scan(ctx, probes, targets, 2, 100, 0, 50)) as rows:
        table = rows.fetch()
        assert rows.n >= n and set(table[1].tolist()) == {0, 1}
        plain = rows.greedy(n)
        for drop in (np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 2 == 1, rng.random(n) < 0.1,
                     np.isin(np.arange(n), plain)):
            _picks, want = _check(ctx, rows, table, n, drop, greedy=False)
            with closing(rows.drop_sets(n, drop)) as left, closing(engine.Rows.from_host(ctx, *want, glen)) as same:
                picks = left.greedy(n)
                assert picks == same.greedy(n) and not drop[picks].any()
                if not drop.any():
                    assert picks == plain
        with pytest.raises(ValueError, match="set id is not below"):
            rows.drop_sets(n // 2, np.zeros(n // 2, bool))
