"""Gain bands of the row-parallel set-cover solver (setcover_flat.inc): the sets are cut
into bands by their round-0 gain, a round streams only the rows of the bands that are awake and lets a set claim
only when its gain reaches the level's boundary.  Whatever the bands, the picks -- and their ORDER -- are those of
the oracle's sequential greedy, and those of the same solve with one band (the rounds without bands).

Every instance is a few hundred to a few thousand rows, forced into the row-parallel solver, and solved with 1, 2
and as many bands as the set-up allows, on striped tiles and on contiguous tiles (several coordinate tiles, so that
a set's rows lie in several sub-tiles).  The boundaries are ratio^(b + 1) x the largest round-0 gain, integer
arithmetic, ratio 1/2 here unless said otherwise: a largest gain of 1000 gives 500, 250, 125, 62, 31, ..."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 1200            # bases per universe
MAX_BANDS = 64      # more than any set-up allows: clamped to its maximum


def _engine():
    from catch_amd import engine
    return engine


def _rows(sets):
    """sets: per set id a list of (universe, start, length) -> sorted int64 rows (set, universe, start, end)."""
    out = []
    for s, rows in enumerate(sets):
        for u, x, ln in rows:
            assert 0 < ln <= 257 and 0 <= x and x + ln <= G
            out.append((s, u, x, x + ln))
    return np.array(sorted(set(out)), dtype=np.int64)


def _span(us, x, ln):
    return [(u, x, ln) for u in us]


# ---- the instances: (sets, number of universes) -------------------------------------------------------------------
def inst_all_equal(rng):
    """All gains equal (two rows of 100 bases each): one occupied band, ties by id everywhere."""
    U = 24
    sets = []
    for _ in range(400):
        u0, u1 = (int(v) for v in rng.choice(U, size=2, replace=False))
        sets.append([(u0, 50 * int(rng.integers(0, 20)), 100), (u1, 50 * int(rng.integers(0, 20)), 100)])
    return sets, U


def inst_octaves(rng):
    """Gains from 100 to 6400 (six octaves, more than the two-band and more than a four-band cut resolve)."""
    U = 64
    sets = []
    for i in range(300):
        nu = 1 << int(rng.integers(0, 7))
        us = sorted(int(v) for v in rng.choice(U, size=nu, replace=False))
        sets.append(_span(us, 50 * int(rng.integers(0, 22)), 100))
    return sets, U


def inst_empty_band(rng):
    """Gains of 1000 (band 0) and of 100 (band 3 of 500 / 250 / 125 / 62): two empty bands in between, whose levels
    pass without a claimant."""
    U = 30
    sets = []
    for i in range(60):
        us = sorted(int(v) for v in rng.choice(20, size=10, replace=False))
        sets.append(_span(us, 100 * int(rng.integers(0, 11)), 100))
    for i in range(300):
        sets.append([(int(rng.integers(0, U)), 25 * int(rng.integers(0, 44)), 100)])
    return sets, U


def inst_boundary(rng):
    """The largest gain is 1000, so the first boundary is 500: sets of exactly 500 (band 0) and of 499 (band 1)
    compete for the same bases."""
    U = 12
    sets = [_span(range(0, 10), 0, 100)]                                     # 1000
    for i in range(40):
        x = 100 + 20 * i
        us = sorted(int(v) for v in rng.choice(U, size=5, replace=False))
        sets.append(_span(us, x, 100))                                       # 500
        sets.append(_span(us[:4], x + 10, 100) + [(us[4], x + 10, 99)])      # 499
    return sets, U


def inst_tie_by_id(rng):
    """Pairs of sets with equal gain that share bases, the lower id now the left and now the right one, in the top
    band and in a lower one: the lower id goes first and the other's gain falls."""
    U = 16
    sets = []
    for i in range(40):
        us = [2 * (i % 8), 2 * (i % 8) + 1]
        x = 120 * (i // 8) + 10
        big = i % 2 == 0
        left = _span(us, x, 100) + (_span(range(0, 8), 900 + i, 100) if big else [])
        right = _span(us, x + 40, 100) + (_span(range(8, 16), 900 + i, 100) if big else [])
        sets += [left, right] if i % 4 < 2 else [right, left]
    return sets, U


def inst_sleeping_only_cover(rng):
    """Low-gain sets (30 bases, asleep until the last levels) that are the only cover of their bases: they must
    wake and be picked."""
    U = 20
    sets = []
    for i in range(80):
        us = sorted(int(v) for v in rng.choice(U, size=10, replace=False))
        sets.append(_span(us, 100 * int(rng.integers(0, 10)), 100))
    for u in range(U):
        sets.append([(u, 1100 + 2 * u, 30)])
    return sets, U


def inst_falls_below(rng):
    """Sets of the top band (900 of a largest 1000) that lose all but 100 bases to the first pick: recounted below
    the level's boundary they must not claim at level 0, and are picked later, as in the sequential order."""
    U = 10
    sets = [_span(range(U), 0, 100)]                                         # 1000
    for i in range(9):
        rows = [(u, 0, 100) for u in range(U) if u != i][:8] + [(i, 150 + 110 * i, 100)]
        sets.append(sorted(rows))                                            # 900, of which 100 its own
    for i in range(60):
        sets.append([(int(rng.integers(0, U)), 120 + 10 * int(rng.integers(0, 98)), 60)])
    return sets, U


def inst_covered_at_level0(rng):
    """The top band covers every base; the lower bands hold only parts of it: the solve ends with nothing picked
    from them."""
    U = 16
    sets = []
    for x in range(0, G, 100):
        sets.append(_span(range(0, 8), x, 100))
        sets.append(_span(range(8, 16), x, 100))
    top = len(sets)
    for i in range(300):
        nu = int(rng.integers(1, 4))
        us = sorted(int(v) for v in rng.choice(U, size=nu, replace=False))
        sets.append(_span(us, int(rng.integers(0, G - 60)), int(rng.integers(20, 60))))
    return sets, U, top


def inst_union_tenfold(rng):
    """A union of two independent groups: sets of group A gain about 2000, those of group B (its own universes)
    about 200."""
    U = 44
    sets = []
    for i in range(150):
        us = sorted(int(v) for v in rng.choice(40, size=int(rng.integers(15, 21)), replace=False))
        sets.append(_span(us, 25 * int(rng.integers(0, 44)), 100))
    for i in range(250):
        us = sorted(40 + int(v) for v in rng.choice(4, size=int(rng.integers(1, 3)), replace=False))
        sets.append(_span(us, 10 * int(rng.integers(0, 110)), 100))
    return sets, U


def inst_random(rng):
    """Rows of any length up to 257 bases, several per set and universe; the default ratio."""
    U = 14
    sets = []
    for s in range(500):
        rows = []
        for u in range(U):
            if rng.random() < 0.4:
                pos = int(rng.integers(0, G - 600))
                for _ in range(int(rng.integers(1, 3))):
                    ln = int(rng.integers(1, 258))
                    rows.append((u, pos, ln))
                    pos += ln + int(rng.integers(1, 60))
        sets.append(rows)
    return sets, U


INSTANCES = {
    "all gains equal": inst_all_equal,
    "more octaves than bands": inst_octaves,
    "empty band in the middle": inst_empty_band,
    "gain on a boundary": inst_boundary,
    "ties by id": inst_tie_by_id,
    "sleeping set is the only cover": inst_sleeping_only_cover,
    "recounted below the boundary": inst_falls_below,
    "covered at level 0": inst_covered_at_level0,
    "union of unlike groups": inst_union_tenfold,
    "random": inst_random,
}
_cache = {}


def _instance(name, oracle):
    """rows, sets, universes, expected picks (the oracle's sequential greedy): built once, shared, never changed."""
    if name not in _cache:
        made = INSTANCES[name](np.random.Generator(np.random.PCG64(20261019)))
        sets, U = made[0], made[1]
        r = _rows(sets)
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], len(sets), U, None, None, None)
        _cache[name] = (r, len(sets), U, list(exp), made[2:] and made[2])
    return _cache[name]


def _tiles(monkeypatch, tiles, U):
    """Forces the row-parallel solver and the tile form; returns the bands the set-up allows."""
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    if tiles == "striped":
        return 32                       # 8 tiles, one per XCD, of up to 32 sub-tiles
    monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "13")
    ntiles = ((U * G) >> 13) + 1
    assert 2 <= ntiles < 256
    return 32 // ((ntiles + 7) // 8)


def _solve(ctx, r, P, glen, ranks=None):
    dev = _engine().Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
    got = dev.greedy(P, ranks, None)
    cn = ctx.counters()
    dev.close()
    assert cn["flat_rows_streamed"] > 0          # the row-parallel kernels ran
    return got, cn


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
@pytest.mark.parametrize("name", list(INSTANCES))
def test_banded_rounds_pick_in_sequential_order(ctx, oracle, monkeypatch, name, tiles):
    r, P, U, exp, extra = _instance(name, oracle)
    glen = np.full(U, G, dtype=np.int64)
    allowed = _tiles(monkeypatch, tiles, U)
    if name != "random":
        monkeypatch.setenv("CATCHHIP_FLAT_BAND_RATIO", "500")
    monkeypatch.setenv("CATCHHIP_FLAT_BANDS", "1")
    one, cn1 = _solve(ctx, r, P, glen)
    assert cn1["flat_bands"] == 1 and cn1["flat_levels"] == 1
    assert one == exp
    streamed = {1: cn1["flat_rows_streamed"]}
    for bands in (2, MAX_BANDS):
        monkeypatch.setenv("CATCHHIP_FLAT_BANDS", str(bands))
        got, cn = _solve(ctx, r, P, glen)
        assert cn["flat_bands"] == min(bands, allowed), (name, tiles, bands)
        assert cn["flat_levels"] == cn["flat_bands"]         # a solve ends at the last level
        assert got == exp, (name, tiles, bands)
        assert got == one, (name, tiles, bands)
        streamed[bands] = cn["flat_rows_streamed"]
    if name == "covered at level 0":
        assert all(s < extra for s in exp)                   # nothing of the lower bands is picked
    if name == "sleeping set is the only cover":
        assert set(range(P - U, P)) <= set(exp)              # every low-gain only-cover set is
    print(name, tiles, "rows streamed by bands:", streamed)


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
def test_ranks_given_keep_one_band(ctx, oracle, monkeypatch, tiles):
    """With ranks the bands are off, whatever is asked for, and the picks are the oracle's."""
    r, P, U, _, _ = _instance("more octaves than bands", oracle)
    glen = np.full(U, G, dtype=np.int64)
    _tiles(monkeypatch, tiles, U)
    ranks = np.random.Generator(np.random.PCG64(5)).integers(0, 3, size=P)
    exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, U, None, None, ranks)
    for bands in (1, 2, MAX_BANDS):
        monkeypatch.setenv("CATCHHIP_FLAT_BANDS", str(bands))
        got, cn = _solve(ctx, r, P, glen, ranks)
        assert cn["flat_bands"] == 1
        assert got == exp, bands


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
def test_default_bands_on_direct_rows(ctx, oracle, monkeypatch, tiles):
    """The default band count and ratio on the rows of a scan, solved where the row build leaves them (direct rows,
    round-0 gains summed by the row build): the picks of one band, and the oracle's probe set."""
    from catch_amd import probe
    from util import candidates, small_species
    engine = _engine()
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    if tiles == "contiguous":
        monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "14")
    genomes = small_species(seed=77, n=24, length=3000, d1=0.04, d2=0.015)
    strs = candidates(genomes, 100, 50)
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, 100, 50)
    k = probe.anchor_table([strs[0]], 2, 100, assume_unique=True)[0]
    p = c.probes(k)
    res = {}
    for bands in ("1", None):
        if bands is not None:
            monkeypatch.setenv("CATCHHIP_FLAT_BANDS", bands)
        else:
            monkeypatch.delenv("CATCHHIP_FLAT_BANDS")
        res[bands] = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n, None, None)
        cn = ctx.counters()
        assert cn["rows_direct"] == 1 and cn["flat_rows_streamed"] > 0
        assert cn["flat_bands"] == (1 if bands else min(2, 32 if tiles == "striped" else 32 // (((24 * 3000 >> 14) + 8) // 8)))
    p.close(); c.close(); t.close()
    assert res[None] == res["1"] and len(res["1"][0]) > 0
    exp = oracle.set_cover_filter([strs], [genomes], 2, 100, coverage=1.0, cover_extension=50)[0]
    assert sorted(res[None][0]) == sorted(exp)


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
def test_union_with_group_numbers_tenfold_gain_scale(ctx, oracle, monkeypatch, tiles):
    """Rows with group numbers (a scan of grouped targets, solved as one instance): a group of 30 genomes beside one
    of 3, so the sets' gains differ tenfold.  Such an instance keeps one band unless asked; with 2 bands and with as
    many as the set-up allows every group's picks, in order, are those of one band, and as a set the oracle's."""
    from catch_amd import probe
    from util import candidates, small_species
    engine = _engine()
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    monkeypatch.setenv("CATCHHIP_FLAT_BAND_RATIO", "500")
    allowed = 32
    groups = [small_species(seed=81, n=30, length=2500, d1=0.04, d2=0.015),
              small_species(seed=82, n=3, length=2500, d1=0.04, d2=0.015)]
    genomes = [g for grp in groups for g in grp]
    if tiles == "contiguous":
        monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "14")
        ntiles = (sum(len(s) for g in genomes for s in g) >> 14) + 1
        assert 2 <= ntiles < 256
        allowed = 32 // ((ntiles + 7) // 8)
    t = engine.Targets(ctx, genomes)
    t.set_groups(np.repeat(np.arange(2), [len(g) for g in groups]))
    c = engine.Candidates(ctx, t, 100, 50)
    cg = c.groups()
    strs = [candidates(grp, 100, 50) for grp in groups]
    k = probe.anchor_table([strs[0][0]], 2, 100, assume_unique=True)[0]
    p = c.probes(k)
    res = {}
    for bands in (None, 1, 2, MAX_BANDS):
        if bands is not None:
            monkeypatch.setenv("CATCHHIP_FLAT_BANDS_GROUPED", str(bands))
        res[bands] = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n, None, None)
        cn = ctx.counters()
        assert cn["rows_direct"] == 1 and cn["flat_rows_streamed"] > 0
        assert cn["flat_bands"] == (1 if bands is None else min(bands, allowed)), (tiles, bands)
    p.close(); c.close(); t.close()
    for bands in (None, 2, MAX_BANDS):
        assert res[bands] == res[1], (tiles, bands)
    ids = np.asarray(res[1][0], dtype=np.int64)
    want = oracle.set_cover_filter(strs, groups, 2, 100, coverage=1.0, cover_extension=50)
    for j in range(2):
        members = np.nonzero(cg == j)[0]
        assert members.size == len(strs[j])
        mine = np.searchsorted(members, ids[cg[ids] == j])
        assert sorted(int(x) for x in mine) == sorted(want[j]), j
        assert len(mine) > 0
