"""Gain bands on a UNION of independent groups (rows of a scan with group numbers, solved as one instance by the
row-parallel solver; setcover_flat.inc): every group's sets are cut into bands by that
group's own largest round-0 gain, the level stays one number for the instance, and a set claims when its gain reaches
its own group's boundary of the level.

Whatever the bands, every group's picks -- in pick order -- are those of the same union with one band, and as a set
those of the oracle's filter run on that group alone.  Every input is a few thousand bases per genome, forced into the
row-parallel solver through the synchronous filter (CATCHHIP_FILTER_NO_DEFER, CATCHHIP_FLAT_MIN_ROWS=0), on striped
and on contiguous tiles, with 1, 2 and as many bands as the set-up allows, at ratio 1/2 and at the default ratio."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_BANDS = 64      # more than any set-up allows: clamped to its maximum
HERE = os.path.dirname(os.path.abspath(__file__))


def _species(seed, n, length):
    from util import small_species
    return small_species(seed=seed, n=n, length=length, d1=0.04, d2=0.015)


# ---- the inputs: (groups of genomes in genome order, group number of every group) ----------------------------------
def case_tenfold():
    """Two groups of 30 and 3 genomes: the sets' gains differ tenfold."""
    return [_species(81, 30, 2500), _species(82, 3, 2500)], [0, 1]


def case_flat_middle():
    """12 / 1 / 12 genomes: every gain of the middle group is about one probe's reach, all in its band 0."""
    return [_species(83, 12, 2600), _species(84, 1, 3000), _species(85, 12, 2700)], [0, 1, 2]


def case_sparse_numbers():
    """Group numbers that are neither dense nor ascending."""
    return [_species(86, 9, 2500), _species(87, 2, 2800), _species(88, 5, 2600)], [7, 2, 40]


def case_borders_in_words():
    """Five groups whose lengths are no multiples of 64: group borders fall inside bitmap words."""
    return [_species(89 + i, n, ln) for i, (n, ln) in enumerate([(7, 2501), (2, 2613), (11, 2750), (1, 2999), (4, 2837)])], [0, 1, 2, 3, 4]


def case_identical_genomes():
    """A group of identical genomes beside an ordinary one: after the first round all but a handful of the identical
    group's sets gain nothing."""
    one = _species(95, 1, 2900)[0]
    return [[list(one) for _ in range(10)], _species(96, 8, 2500)], [0, 1]


CASES = {
    "tenfold": case_tenfold,
    "flat middle group": case_flat_middle,
    "sparse group numbers": case_sparse_numbers,
    "borders inside words": case_borders_in_words,
    "identical genomes": case_identical_genomes,
}
_cache = {}


def _case(name, oracle):
    """groups, numbers, candidate strings per group, the oracle's picks per group: built once, shared, never changed."""
    if name not in _cache:
        from util import candidates
        groups, numbers = CASES[name]()
        strs = [candidates(grp, 100, 50) for grp in groups]
        want = oracle.set_cover_filter(strs, groups, 2, 100, coverage=1.0, cover_extension=50)
        _cache[name] = (groups, numbers, strs, [sorted(w) for w in want])
    return _cache[name]


def _allowed(monkeypatch, tiles, total):
    """Sets the tile form; returns the bands the set-up allows (an XCD lists at most 32 sub-tiles)."""
    if tiles == "striped":
        return 32
    monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "14")
    ntiles = (total >> 14) + 1
    assert 2 <= ntiles < 256
    return 32 // ((ntiles + 7) // 8)


def _forced(monkeypatch):
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")


def _solve_all(ctx, monkeypatch, engine, p, t, n, ngroups, allowed, label):
    """The union with 1, 2 and MAX_BANDS bands at ratio 1/2 and at the default ratio -> the picks with one band.  Checks
    the counters of every solve and that all of them pick the same sets in the same order."""
    one = None
    for ratio in ("500", None):
        if ratio is None:
            monkeypatch.delenv("CATCHHIP_FLAT_BAND_RATIO")
        else:
            monkeypatch.setenv("CATCHHIP_FLAT_BAND_RATIO", ratio)
        for bands in (1, 2, MAX_BANDS):
            monkeypatch.setenv("CATCHHIP_FLAT_BANDS_GROUPED", str(bands))
            got = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, n, None, None)
            cn = ctx.counters()
            assert cn["rows_direct"] == 1 and cn["flat_rows_streamed"] > 0, (label, ratio, bands)
            assert cn["flat_bands"] == min(bands, allowed), (label, ratio, bands)
            assert cn["flat_band_groups"] == (ngroups if min(bands, allowed) > 1 else 1), (label, ratio, bands)
            print(label, "ratio", ratio, "bands", bands, "levels", cn["flat_levels"], "rounds", cn["greedy_iters"],
                  "rows streamed", cn["flat_rows_streamed"])
            if one is None:
                one = got
            assert list(got[0]) == list(one[0]), (label, ratio, bands)       # every group's picks, in pick order
    return one


def _union(ctx, engine, groups, numbers):
    from catch_amd import probe
    genomes = [g for grp in groups for g in grp]
    t = engine.Targets(ctx, genomes)
    t.set_groups(np.repeat(np.asarray(numbers, dtype=np.int32), [len(g) for g in groups]))
    c = engine.Candidates(ctx, t, 100, 50)
    first = next(s for g in genomes for s in g)[:100]
    k = probe.anchor_table([first], 2, 100, assume_unique=True)[0]
    return t, c, c.probes(k)


def _per_group(ids, cg, numbers, sizes):
    """Union ids -> per group, in pick order, the index among the group's own unique candidates."""
    ids = np.asarray(ids, dtype=np.int64)
    out = []
    for j, num in enumerate(numbers):
        members = np.nonzero(cg == num)[0]
        assert members.size == sizes[j], j
        out.append([int(x) for x in np.searchsorted(members, ids[cg[ids] == num])])
    return out


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
@pytest.mark.parametrize("name", list(CASES))
def test_union_bands_pick_what_one_band_picks(ctx, oracle, monkeypatch, name, tiles):
    from catch_amd import engine
    groups, numbers, strs, want = _case(name, oracle)
    _forced(monkeypatch)
    total = sum(len(s) for grp in groups for g in grp for s in g)
    if name == "borders inside words":
        ends = np.cumsum([sum(len(s) for g in grp for s in g) for grp in groups])[:-1]
        assert all(int(e) % 64 for e in ends)
    allowed = _allowed(monkeypatch, tiles, total)
    t, c, p = _union(ctx, engine, groups, numbers)
    cg = c.groups()
    one = _solve_all(ctx, monkeypatch, engine, p, t, c.n, len(groups), allowed, (name, tiles))
    p.close(); c.close(); t.close()
    mine = _per_group(one[0], cg, numbers, [len(s) for s in strs])
    for j in range(len(groups)):
        assert sorted(mine[j]) == want[j], (name, tiles, j)
        assert len(mine[j]) > 0


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
def test_union_with_interleaved_group_numbers(ctx, oracle, monkeypatch, tiles):
    """Group numbers interleaved over the genomes (0, 1, 0, 1, ...): the scan accepts groups that are not contiguous
    in the coordinate space, so group borders are everywhere -- the picks per group are the oracle's all the same."""
    from catch_amd import engine, probe
    from util import candidates
    key = "interleaved"
    if key not in _cache:
        a, b = _species(97, 8, 2500), _species(98, 3, 2700)
        genomes, numbers = [], []
        for i in range(8):
            genomes.append(a[i]); numbers.append(0)
            if i < 3:
                genomes.append(b[i]); numbers.append(1)
        strs = [candidates(a, 100, 50), candidates(b, 100, 50)]
        want = oracle.set_cover_filter(strs, [a, b], 2, 100, coverage=1.0, cover_extension=50)
        _cache[key] = (genomes, numbers, strs, [sorted(w) for w in want])
    genomes, numbers, strs, want = _cache[key]
    _forced(monkeypatch)
    allowed = _allowed(monkeypatch, tiles, sum(len(s) for g in genomes for s in g))
    t = engine.Targets(ctx, genomes)
    t.set_groups(np.asarray(numbers, dtype=np.int32))
    c = engine.Candidates(ctx, t, 100, 50)
    k = probe.anchor_table([genomes[0][0][:100]], 2, 100, assume_unique=True)[0]
    p = c.probes(k)
    cg = c.groups()
    one = _solve_all(ctx, monkeypatch, engine, p, t, c.n, 2, allowed, (key, tiles))
    p.close(); c.close(); t.close()
    mine = _per_group(one[0], cg, [0, 1], [len(s) for s in strs])
    for j in range(2):
        assert sorted(mine[j]) == want[j], (tiles, j)


def _s4_union(ctx, engine, scale):
    from catch_amd.utils import synthetic
    groups = synthetic.dataset("S4", scale=scale)
    t, c, p = _union(ctx, engine, groups, list(range(len(groups))))
    return groups, t, c, p


def test_s4_small_union_of_twenty_groups(ctx, monkeypatch):
    """synthetic.dataset("S4", scale=0.004): 99 genomes in 20 groups, 2.6 Mbases, about 53 k candidates, solved as one
    union with 2 bands: every group's picks, in order, are those of the union with one band and those of the filter
    run on that group alone, and the selection is the one the live reference made (tests/golden/reference_runs.json)."""
    from catch_amd import engine, probe
    from catch_amd.filter import candidate_probes
    _forced(monkeypatch)
    groups, t, c, p = _s4_union(ctx, engine, 0.004)
    assert len(groups) == 20 and sum(len(g) for g in groups) == 99
    cg = c.groups()
    res = {}
    for bands in (1, 2):
        monkeypatch.setenv("CATCHHIP_FLAT_BANDS_GROUPED", str(bands))
        res[bands] = list(engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n, None, None)[0])
        cn = ctx.counters()
        assert cn["flat_bands"] == bands and cn["flat_band_groups"] == (20 if bands > 1 else 1)
        print("S4 x 0.004 union, bands", bands, "rounds", cn["greedy_iters"], "rows streamed", cn["flat_rows_streamed"])
    p.close(); c.close(); t.close()
    assert res[2] == res[1]
    cands = [list(dict.fromkeys(candidate_probes.candidate_strings_from_sequences([s for g in grp for s in g], 100, 50)))
             for grp in groups]
    mine = _per_group(res[2], cg, list(range(20)), [len(x) for x in cands])
    monkeypatch.delenv("CATCHHIP_FLAT_BANDS_GROUPED")
    for j, grp in enumerate(groups):
        tj = engine.Targets(ctx, grp)
        cj = engine.Candidates(ctx, tj, 100, 50)
        pj = cj.probes(probe.anchor_table([cands[j][0]], 2, 100, assume_unique=True)[0])
        alone = list(engine.setcover_filter(ctx, pj, tj, 2, 100, 0, 50, cj.n, None, None)[0])
        pj.close(); cj.close(); tj.close()
        assert mine[j] == [int(x) for x in alone], j
    with open(os.path.join(HERE, "golden", "reference_runs.json")) as f:
        rec = [r for r in json.load(f)["runs"] if r["input"] == "S4" and r["scale"] == 0.004]
    assert len(rec) == 1 and sum(map(len, cands)) == rec[0]["P"]
    sel = [sorted(cd[i] for i in g) for cd, g in zip(cands, mine)]
    assert sum(map(len, sel)) == rec[0]["probes_out"]
    assert hashlib.sha256("\n".join(",".join(g) for g in sel).encode()).hexdigest() == rec[0]["picks_sha256"]


DEFAULT_SCALE = 0.021


def test_large_union_takes_two_bands_by_default(ctx, monkeypatch):
    """Nothing forced: a union that reaches the row-parallel solver by its own size (2^18 rows or more) is cut into
    GR_BANDS = 2 bands, group by group, and picks what it picks with the hook at 1.

    S4 x 0.02 (10.9 Mbases, 427,410 rows) has the rows but not the bases: below 2^26 / 6 = 11.2 Mbases of targets the
    filter queues scan and solve without a synchronisation and the fused solver takes the rows.  S4 x 0.021 (11.9
    Mbases, 456 genomes in 20 groups, 484,012 rows) is the smallest scale in steps of 0.001 that the filter scans
    synchronously.
    A second filter call with the same probes sizes its work list by the seeds the first one saw and may then fall
    below that limit, so the solve with the hook at 1 gets probes of its own."""
    from catch_amd import engine, probe
    for v in ("CATCHHIP_FLAT_BANDS_GROUPED", "CATCHHIP_FLAT_MIN_ROWS", "CATCHHIP_FLAT_BAND_RATIO", "CATCHHIP_FILTER_NO_DEFER"):
        monkeypatch.delenv(v, raising=False)
    groups, t, c, p = _s4_union(ctx, engine, DEFAULT_SCALE)
    got, nrows = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n, None, None)
    cn = ctx.counters()
    print("S4 x", DEFAULT_SCALE, "union: rows", nrows, "bands", cn["flat_bands"], "groups", cn["flat_band_groups"],
          "rounds", cn["greedy_iters"], "rows streamed", cn["flat_rows_streamed"])
    assert nrows >= 1 << 18
    assert cn["flat_rows_streamed"] > 0 and cn["flat_bands"] == 2 and cn["flat_band_groups"] == len(groups)
    monkeypatch.setenv("CATCHHIP_FLAT_BANDS_GROUPED", "1")
    p.close()
    p = c.probes(probe.anchor_table([groups[0][0][0][:100]], 2, 100, assume_unique=True)[0])
    one, _ = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n, None, None)
    cn = ctx.counters()
    assert cn["flat_rows_streamed"] > 0 and cn["flat_bands"] == 1 and cn["flat_band_groups"] == 1
    p.close(); c.close(); t.close()
    assert list(got) == list(one) and len(got) > 0
