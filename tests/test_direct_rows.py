"""catchhip_setcover_filter solving from the row build's bucketed records ("direct rows")
against the same instance solved through the SoA row table (Rows.scan + greedy) and against the CPU oracle.
Small instances: the no-defer hook sends them through the synchronous branch, CATCHHIP_FLAT_MIN_ROWS=0 to the
row-parallel solver.  The oracle's set_cover_filter takes ONE coverage fraction and no ranks: the runs with a mixed
universe_p or with ranks are compared with the SoA path only (which test_gpu_parity.py holds against the oracle's
lazy_greedy under both)."""
import numpy as np
import pytest

from util import candidates, small_species

pytestmark = pytest.mark.gpu

M, THRES, L, STRIDE = 2, 100, 100, 50


def _engine():
    from catch_amd import engine
    return engine


def _probe_mod():
    from catch_amd import probe
    return probe


@pytest.fixture
def sync_flat(monkeypatch):
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    return monkeypatch


def _rand_dna(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _with_tandem_repeats(genomes):
    """A copy of `genomes` with two short chromosomes in which a 100-mer stands twice, 30 bases apart, so that at
    extension 50 the probe's two cover ranges merge -- into a row of at most 257 bases, because the chromosome's
    ends clip it.  One is the FIRST sequence of the first genome, and the probe is its first window (bucket 0,
    slot 0 of the records); one is the LAST sequence of the last genome: 245 bases, the 100-mer at 15 and at 145,
    so that only the closing window holds it (15 is off the stride grid) and the probe is the last unique
    candidate (the last bucket, at the very end of the records)."""
    w0, w1 = _rand_dna(901, 100), _rand_dna(902, 100)
    out = [list(g) for g in genomes]
    out[0] = [w0 + _rand_dna(903, 30) + w0] + out[0]
    out[-1] = out[-1] + [_rand_dna(904, 15) + w1 + _rand_dna(905, 30) + w1]
    return out


def _device_probes(ctx, genomes, groups=None):
    """Targets, Candidates and the pigeonhole Probes of the device front end (identity buckets)."""
    engine, probe = _engine(), _probe_mod()
    t = engine.Targets(ctx, genomes)
    if groups is not None:
        t.set_groups(groups)
    c = engine.Candidates(ctx, t, L, STRIDE)
    k = probe.anchor_table([_rand_dna(1, L)], M, THRES, assume_unique=True)[0]
    return t, c, c.probes(k)


def _string_probes(ctx, genomes, strs):
    """Targets and Probes from candidate strings (a bucket -> set table, duplicates allowed)."""
    engine, probe = _engine(), _probe_mod()
    k, uniq, owner, ep, eo = probe.anchor_table(strs, M, THRES)
    return engine.Targets(ctx, genomes), engine.Probes(ctx, uniq, owner, ep, eo, k)


def _solve_both(ctx, p, t, nsets, ext=50, ranks=None, up=None):
    """(picks in order, rows) through the SoA table and through the fused filter, the filter's rows_direct and
    raw hits."""
    engine = _engine()
    rows = engine.Rows.scan(ctx, p, t, M, THRES, 0, ext)
    want = (rows.greedy(nsets, ranks, up), rows.n)
    rows.close()
    got = engine.setcover_filter(ctx, p, t, M, THRES, 0, ext, nsets, ranks, up)
    c = ctx.counters()
    assert got == want, (len(got[0]), len(want[0]), got[1], want[1])
    assert len(got[0]) > 0
    return got, c["rows_direct"], c["raw_hits"]


_ORACLE = {}


def _oracle_ids(oracle, key, strs, genomes, coverage, ext=50):
    if (key, coverage, ext) not in _ORACLE:
        _ORACLE[(key, coverage, ext)] = sorted(oracle.set_cover_filter(
            [strs], [genomes], M, THRES, coverage=coverage, cover_extension=ext)[0])
    return _ORACLE[(key, coverage, ext)]


def _plain_genomes():
    return small_species(seed=301, n=48, length=4000, d1=0.04, d2=0.01)


@pytest.mark.parametrize("tiles", ["shift12", "striped", "forced-soa"])
def test_nothing_merged_identity_buckets(ctx, oracle, sync_flat, tiles):
    """Device candidates (identity buckets), nothing merges, more than three partition blocks of
    4,096 rows; tiles of 4 kbases (sets cross tile borders, 47 tiles), the 8 striped tiles, and the same through
    the forced SoA form.  Full coverage, -c 0.9, mixed universe_p, and with ranks."""
    if tiles != "striped":
        sync_flat.setenv("CATCHHIP_FLAT_TILE_SHIFT", "12")
    if tiles == "forced-soa":
        sync_flat.setenv("CATCHHIP_ROWS_SOA", "1")
    genomes = _plain_genomes()
    strs = candidates(genomes, L, STRIDE)
    t, c, p = _device_probes(ctx, genomes)
    assert c.n == len(strs)
    expect_direct = 0 if tiles == "forced-soa" else 1
    rng = np.random.Generator(np.random.PCG64(5))
    mixed = [float(x) for x in rng.choice([1.0, 0.9, 0.5], size=len(genomes))]
    ranks = [int(x) for x in rng.integers(0, 3, size=c.n)]
    for up, rk, cov in [(None, None, 1.0), ([0.9] * len(genomes), None, 0.9), (mixed, None, None),
                        (None, ranks, None), (mixed, ranks, None)]:
        (ids, nrows), direct, hits = _solve_both(ctx, p, t, c.n, 50, rk, up)
        assert direct == expect_direct, (tiles, up is not None, rk is not None)
        assert nrows > 3 * 4096 and hits == nrows           # three partition blocks and more; nothing merged
        assert ctx.counters()["flat_rows_streamed"] > 0     # the row-parallel solver
        if cov is not None:
            assert sorted(ids) == _oracle_ids(oracle, "plain", strs, genomes, cov)
    p.close(); c.close(); t.close()


def test_merged_rows_leave_gaps_in_the_records(ctx, oracle, sync_flat):
    """Buckets whose ranges merged keep stale records behind their rows; the first and the last bucket of
    the table are such buckets."""
    engine = _engine()
    sync_flat.setenv("CATCHHIP_FLAT_TILE_SHIFT", "12")
    genomes = _with_tandem_repeats(small_species(seed=302, n=8, length=2500, d1=0.04, d2=0.01))
    strs = candidates(genomes, L, STRIDE)
    t, c, p = _device_probes(ctx, genomes)
    assert c.n == len(strs)
    rows = engine.Rows.scan(ctx, p, t, M, THRES, 0, 50)
    sid, _, st, en = rows.fetch()
    rows.close()
    # the merged rows are where the case wants them: in set 0 and in the last set (230 and 245 bases)
    assert int((en - st)[sid == 0].max()) == 230 and int((en - st)[sid == c.n - 1].max()) == 245
    assert int((en - st).max()) <= 257
    mixed = [1.0, 0.9, 0.5, 1.0, 0.9, 0.5, 1.0, 0.9]
    for up, cov in [(None, 1.0), ([0.9] * len(genomes), 0.9), (mixed, None)]:
        (ids, nrows), direct, hits = _solve_both(ctx, p, t, c.n, 50, None, up)
        assert hits > nrows          # something merged: the table has gaps
        assert direct == 1           # identity buckets
        if cov is not None:
            assert sorted(ids) == _oracle_ids(oracle, "tandem", strs, genomes, cov)
    p.close(); c.close(); t.close()


def test_bucket_to_set_table(ctx, oracle, sync_flat):
    """Probes from strings with duplicates (a set id is the LAST index of its string: the buckets are not
    the sets).  Nothing merged: direct; with the tandem repeats: the SoA form is made.  The picks are the same."""
    sync_flat.setenv("CATCHHIP_FLAT_TILE_SHIFT", "12")
    base = small_species(seed=303, n=8, length=2500, d1=0.04, d2=0.01)
    for key, genomes, want_direct in [("dups", base, 1), ("dups-tandem", _with_tandem_repeats(base), 0)]:
        strs = candidates(genomes, L, STRIDE, dedup=False)
        strs = strs + strs[::7]                                # and more duplicates, far from their first copy
        assert len(set(strs)) < len(strs)
        t, p = _string_probes(ctx, genomes, strs)
        for up, cov in [(None, 1.0), ([0.9] * len(genomes), 0.9)]:
            (ids, nrows), direct, hits = _solve_both(ctx, p, t, len(strs), 50, None, up)
            assert direct == want_direct, key
            assert (hits > nrows) == (want_direct == 0)
            assert sorted(ids) == _oracle_ids(oracle, key, strs, genomes, cov)
        p.close(); t.close()


def test_union_of_three_unlike_groups(ctx, oracle, sync_flat):
    """Three groups as one instance (group numbers on the targets, candidates that carry them): direct, every
    group's picks, in order, are the picks of the group solved alone, and as a set the oracle's for that group."""
    sync_flat.setenv("CATCHHIP_FLAT_TILE_SHIFT", "12")
    groups = [small_species(seed=304, n=9, length=2600, d1=0.04, d2=0.01),
              small_species(seed=305, n=3, length=1500, d1=0.03, d2=0.01, with_n=False),
              small_species(seed=306, n=14, length=2000, d1=0.05, d2=0.02)]
    genomes = [g for grp in groups for g in grp]
    gof = np.repeat(np.arange(3), [len(g) for g in groups])
    t, c, p = _device_probes(ctx, genomes, gof)
    cg = c.groups()
    strs = [candidates(grp, L, STRIDE) for grp in groups]
    for up in (None, [0.9] * len(genomes)):
        want = oracle.set_cover_filter(strs, groups, M, THRES, coverage=1.0 if up is None else 0.9, cover_extension=50)
        (ids, _), direct, _ = _solve_both(ctx, p, t, c.n, 50, None, up)
        assert direct == 1
        ids = np.asarray(ids, dtype=np.int64)
        for j, grp in enumerate(groups):
            members = np.nonzero(cg == j)[0]                   # the group's candidates, in candidate order
            tj, cj, pj = _device_probes(ctx, grp)
            assert cj.n == members.size == len(strs[j])
            (alone, _), _, _ = _solve_both(ctx, pj, tj, cj.n, 50, None, None if up is None else [0.9] * len(grp))
            mine = ids[cg[ids] == j]
            assert [int(x) for x in np.searchsorted(members, mine)] == [int(x) for x in alone], j
            assert sorted(int(x) for x in alone) == sorted(want[j]), j
            pj.close(); cj.close(); tj.close()
    p.close(); c.close(); t.close()


def test_solvers_that_need_the_soa_table(ctx, oracle, monkeypatch):
    """Rows longer than 257 bases (extension 100), and an instance below the row-parallel solver's size:
    the SoA table is made from the records and the other solvers run; same picks."""
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    genomes = small_species(seed=307, n=6, length=2500, d1=0.04, d2=0.01)
    strs = candidates(genomes, L, STRIDE)
    t, c, p = _device_probes(ctx, genomes)
    assert c.n == len(strs)
    # without the min-rows hook: the set-parallel solver
    (ids, _), direct, _ = _solve_both(ctx, p, t, c.n, 50)
    assert direct == 0 and ctx.counters()["flat_rows_streamed"] == 0
    assert sorted(ids) == _oracle_ids(oracle, "small", strs, genomes, 1.0)
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    (ids, _), direct, _ = _solve_both(ctx, p, t, c.n, 50)
    assert direct == 1
    assert sorted(ids) == _oracle_ids(oracle, "small", strs, genomes, 1.0)
    # long rows, full and partial coverage
    for up, cov in [(None, 1.0), ([0.9] * len(genomes), 0.9)]:
        (ids, _), direct, _ = _solve_both(ctx, p, t, c.n, 100, None, up)
        assert direct == 0
        assert sorted(ids) == _oracle_ids(oracle, "small", strs, genomes, cov, 100)
    p.close(); c.close(); t.close()
