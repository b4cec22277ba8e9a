"""Refused calls hand their device memory back and report their own message.

The constructors of the C library own the object they build until the line that hands it out; a refusal on the way
returns the object and its device blocks to the block cache.  `in_use` = bytes the library holds minus bytes sitting
idle in its cache (engine.pool_stats()) is therefore the same after a refused call as before it, and the ValueError
carries the text of that call, not of the one before."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, THRES, L = 2, 100, 100


def _rand_dna(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _in_use(engine):
    st = engine.pool_stats()
    return st["bytes_held"] - st["bytes_cached_free"]


def _probes(ctx, strs):
    from catch_amd import engine, probe
    k, uniq, owner, ep, eo = probe.anchor_table(strs, M, THRES)
    return engine.Probes(ctx, uniq, owner, ep, eo, k)


def _refused(engine, match, call):
    """`call` raises ValueError with `match` and leaves in_use as it was."""
    before = _in_use(engine)
    with pytest.raises(ValueError, match=match):
        call()
    assert _in_use(engine) == before, match


def test_refusals_return_their_memory(ctx):
    from catch_amd import engine
    gc.collect()   # (device objects of earlier tests that only a collection frees go now, not between two readings)
    seq = _rand_dna(4100, 300)
    strs = [seq[0:100], seq[100:200], seq[200:300]]

    def solve():
        p, t = _probes(ctx, strs), engine.Targets(ctx, [[seq]])
        rows = engine.Rows.scan(ctx, p, t, M, THRES, 0, 0)
        picks = rows.greedy(len(strs))
        rows.close(); t.close(); p.close()
        return picks

    warm = solve()   # the caches are warm
    assert sorted(warm) == [0, 1, 2]

    # 1. groups on one side only: refused inside the scan, after the rows object took its first block
    p, t = _probes(ctx, strs), engine.Targets(ctx, [[seq]])
    p.set_groups([0, 0, 0])
    _refused(engine, "groups must be set on both", lambda: engine.Rows.scan(ctx, p, t, M, THRES, 0, 0))
    p.close(); t.close()

    # 2. too many cover ranges: one poly-A probe covers 8,301 offsets of 8,400 A's (more than the 8,192 a bucket
    # takes); the scan has run and its scratch is live when the refusal fires
    p, t = _probes(ctx, ["A" * 100]), engine.Targets(ctx, [["A" * 8400]])
    _refused(engine, "cover ranges", lambda: engine.Rows.scan(ctx, p, t, M, THRES, 0, 0, merge=False))
    p.close(); t.close()

    # 3. rows too long for a shard: the probe at offset 100, extended by 80 on both sides, is one row of 260 bases
    p, t = _probes(ctx, [seq[100:200]]), engine.Targets(ctx, [[seq]])
    rows = engine.Rows.scan(ctx, p, t, M, THRES, 0, 80)
    _, _, st, en = rows.fetch()
    assert (en - st).tolist() == [260]
    _refused(engine, "solved unsharded", lambda: engine.Shard(rows, 1))
    rows.close(); p.close(); t.close()

    # 4. host rows out of order
    _refused(engine, "out of order",
             lambda: engine.Rows.from_host(ctx, [1, 0], [0, 0], [0, 50], [10, 60], [300]))

    assert solve() == warm


def test_rows_refusals_keep_their_text(ctx):
    """The refusals that the entries deriving a table from a table share (csrc/rows_host.h), each by its whole
    message: tables, a mask and targets over another coordinate space, depth 0, a pick out of range or given twice.
    Argument refusals on the host or after one tiny launch; nothing is computed.  Not reachable at test size, and
    checked by reading: 2^32 - 1 bases and more, 2^31 rows and more, deferred and direct rows."""
    from catch_amd import engine
    table = ([0, 1, 2], [0, 0, 1], [0, 5, 0], [10, 20, 30])            # set, universe, start, end: sorted by set
    R = engine.Rows.from_host(ctx, *table, [100, 50])
    other = engine.Rows.from_host(ctx, [0], [0], [1], [2], [100, 51])
    mask = engine.BaseMask(ctx, [100, 51], [0], [1], [2])
    targets = engine.Targets(ctx, [[_rand_dna(7, 151)]])
    spaces = "(151 bases in 2 universes against 150 in 2)"
    picks = {"a pick lies outside the set ids": ([3], [-1], [0, 3]), "a pick is given twice": ([0, 0], [2, 1, 2])}
    cases = [
        ("rows_subtract: the covered rows are not over the coordinate space of the rows " + spaces, lambda: R.subtract(other)),
        ("rows_subtract: the covered rows are not over the coordinate space of the rows "
         "(150 bases in 2 universes against 151 in 2)", lambda: other.subtract(R)),
        ("rows_restrict: the mask is not over the coordinate space of the rows " + spaces, lambda: R.restrict(mask)),
        ("rows_union: the two tables are not over one coordinate space (150 bases in 2 universes against 151 in 2)",
         lambda: R.union(other)),
        ("rows_union: the two tables are not over one coordinate space " + spaces, lambda: other.union(R)),
        ("rows_uncovered: the mask is not over the coordinate space of the rows " + spaces, lambda: R.uncovered(mask=mask)),
        ("rows_uncovered: the targets (151 bases, 1 sequences in 1 genomes) are not one genome per sequence over the "
         "coordinate space of the rows (150 bases in 2 universes)", lambda: R.uncovered(targets)),
        ("rows_prune: the fixed rows are not over the coordinate space of the rows " + spaces,
         lambda: R.prune(3, [0, 1], 1, fixed=other)),
        ("rows_below_depth: depth 0; the smallest depth is 1", lambda: R.below_depth(3, [0], 0)),
        ("rows_prune: depth 0; the smallest depth is 1", lambda: R.prune(3, [0], 0)),
        ("rows_prune: depth 0; the smallest depth is 1", lambda: R.prune(3, [0], 0, fixed=other)),      # (before the space)
        ("rows_below_depth: 4 picks of 3 sets (an id is repeated or out of range)", lambda: R.below_depth(3, [0, 1, 2, 1], 1)),
    ]
    for what, lists in picks.items():
        for pk in lists:
            cases += [("rows_below_depth: " + what, lambda pk=pk: R.below_depth(3, pk, 1)),
                      ("rows_prune: " + what, lambda pk=pk: R.prune(3, pk, 1)),
                      ("rows_pick_gains: " + what, lambda pk=pk: R.pick_gains(3, pk))]
    try:
        for text, call in cases:
            with pytest.raises(ValueError) as err:
                call()
            assert str(err.value) == "catchhip: " + text
        # and the same calls are taken when nothing is wrong with them
        assert R.below_depth(3, [2, 0], 1)[0].n == 1 and R.pick_gains(3, [2, 0])[0].tolist() == [30, 10]
    finally:
        for obj in (R, other, mask, targets):
            obj.close()
