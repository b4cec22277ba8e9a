"""The count launch of the row-parallel set-cover solver (gr_count_kernel in setcover_flat.inc; DESIGN.md section 4
K2) has one instance per form of a launch -- partial coverage, the changed-word statistics and round 0, and for the
rounds of a full-coverage solve one per tile form with and without gain bands -- and counts a row's uncovered
positions from its <= 5 bitmap words with masks made once per row.  These instances are built around what that
code can get wrong: where a row starts and ends inside a word, which of its words are still flagged, where it lies
in its tile, how many records a tile holds, and where a set's run of records falls in a wavefront.

Every solve goes through engine.Rows.from_host -> greedy, forced into the row-parallel solver, and is held against
two things: the oracle's sequential greedy (the picks, in order), and the solver's work counters as recorded from
the library before the instances existed (test_count_word_loop_counters.json): the counters are deterministic, and
they are what keeps a rewrite of the kernel from changing what is counted.

Coordinates: universes of G = 2112 bases (33 words: a universe starts on a word border, and the 4-kbase stripe
borders and the 8-kbase tile borders fall INSIDE universes, so rows can cross them)."""
import json
import os

import numpy as np
import pytest

G = 2112
SHIFT = 13                      # contiguous tiles of 8,192 bases
STARTS = (0, 1, 31, 32, 63)     # first bit of a row in its word
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 193, 256, 257)
TILE_FILL = (63, 64, 65, 256, 257, 2048, 2049)      # records: chunk, wavefront step, workgroup step, and one more
COUNTERS = ("flat_rows_streamed", "flat_rows_recounted", "flat_bitmap_words", "flat_owner_words")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_count_word_loop_counters.json")


def _row(gx, ln):
    """A row by its global start -> (universe, start in the universe, length); it may not leave its universe."""
    u, x = divmod(int(gx), G)
    assert 0 < ln <= 257 and x + ln <= G, (gx, ln)
    return (u, x, int(ln))


def _table(sets):
    out = []
    for s, rows in enumerate(sets):
        rows = sorted(rows)
        for (u0, x0, l0), (u1, x1, _) in zip(rows, rows[1:]):
            assert u0 != u1 or x0 + l0 < x1, ("rows of a set touch", s)      # normalised per (set, universe)
        out += [(s, u, x, x + ln) for u, x, ln in rows]
    return np.array(sorted(out), dtype=np.int64)


def _soup(rng, sets, U, per_universe, lo=0):
    """Random rows of 1 to 257 bases over the universes lo..U-1, in sets of one to three rows: they overlap the
    placed rows, so those are covered piece by piece over several rounds."""
    rows = []
    for u in range(lo, U):
        for _ in range(per_universe):
            ln = int(rng.integers(1, 258))
            rows.append((u, int(rng.integers(0, G - ln + 1)), ln))
    rng.shuffle(rows)
    i = 0
    while i < len(rows):
        n = int(rng.integers(1, 4))
        mine, seen = [], set()
        for r in rows[i:i + n]:
            if r[0] not in seen:                 # (one row per universe: never two rows of a set that touch)
                mine.append(r)
                seen.add(r[0])
        sets.append(mine)
        i += n


def inst_edges(rng):
    """Universe 0-3: the borders of the coordinate space, of a stripe (4,096) and of a tile (8,192).  Universes
    4-16: a slot of 512 bases per (first bit, length), the row from word 1 of the slot, a competitor on its middle
    third (with a row of 120 bases of its own, so that it goes first for lengths up to 129 and second above), and
    neighbours that end and start where the row starts and ends -- in the same words, outside the row.  Two more
    slots: rows of five words whose words 1 and 3 / 0, 2 and 4 are covered first by a set with a higher gain, and
    which lose one more round to a neighbour in word 4 / word 1 (flags 0b10101 and 0b01010 are counted twice).
    Universe 17: sets 0 and 1 hold 60 and 10 rows of one tile, so the records of set 1 cross lanes 63 | 64."""
    U = 18
    total = U * G
    sets = []
    tail = 17 * G
    sets.append([_row(tail + 12 * i, 5) for i in range(60)])                 # set 0: records 0-59 of its tile
    sets.append([_row(tail + 720 + 12 * i, 5) for i in range(10)])           # set 1: records 60-69
    # the borders
    for gx, ln in ((0, 30), (0, 1), (total - 30, 30), (total - 1, 1),
                   (4095, 1), (4096, 50), (4090, 20), (4000, 96), (4096 - 257, 257), (4096 - 256, 257),
                   (8191, 1), (8192, 50), (8150, 100), (8192 - 64, 64), (8192 - 64, 65), (8192, 200)):
        sets.append([_row(gx, ln)])                                          # single-row sets
    slot = 4 * G
    def next_slot():
        nonlocal slot
        s = slot
        slot += 512
        if slot % G > G - 512:                                               # four slots per universe
            slot += G - slot % G
        return s
    for b in STARTS:
        for ln in LENGTHS:
            s = next_slot()
            x = s + 64 + b
            sets.append([_row(x, ln)])
            third = max(1, ln // 3)
            sets.append([_row(x + ln // 3, third), _row(s + 390, 120)])
            sets.append([_row(x - 10, 10)])
            sets.append([_row(x + ln, 7)])
    # flags 0b10101: words 1 and 3 go first (64 + 64 + 200 > 257), then word 4's neighbour (63 + 100 > 129)
    s = next_slot()
    sets.append([_row(s, 257)])
    sets.append([_row(s + 64, 64), _row(s + 192, 64), _row(17 * G + 900, 200)])
    sets.append([_row(s + 257, 63), _row(s + 400, 100)])
    # flags 0b01010: words 0, 2 and 4 go first (64 + 64 + 1 + 200 > 257), then word 1's neighbour
    s = next_slot()
    sets.append([_row(s + 64, 257)])                                         # (words 1-5 of the slot)
    sets.append([_row(s + 64, 64), _row(s + 192, 64), _row(s + 320, 1), _row(17 * G + 1200, 200)])
    sets.append([_row(s + 148, 30), _row(s + 400, 100)])
    assert slot <= 17 * G
    _soup(rng, sets, U, 6)
    return sets, U


def inst_tile_fill(rng):
    """Contiguous tile t holds TILE_FILL[t] records, every one a set of its own: rows of 20 to 59 bases, three bases
    apart, so a pick leaves its neighbours alive with parts of their words covered."""
    U = (len(TILE_FILL) << SHIFT) // G + 1
    sets = []
    for t, n in enumerate(TILE_FILL):
        gx = t << SHIFT
        for _ in range(n):
            ln = int(rng.integers(20, 60))
            if gx % G + ln > G:
                gx += G - gx % G
            assert gx >> SHIFT == t
            sets.append([_row(gx, ln)])
            gx += 3
    return sets, U


def inst_partial(rng):
    """Partial coverage: sets with a row in several universes at about the same place, as in a design."""
    U = 12
    sets = []
    for _ in range(260):
        centre = int(rng.integers(0, G - 300))
        us = np.nonzero(rng.random(U) < 0.5)[0]
        sets.append([(int(u), centre + int(rng.integers(0, 30)), int(rng.integers(1, 258))) for u in us])
    return [s for s in sets if s], U


INSTANCES = {"edges": inst_edges, "tile fill": inst_tile_fill, "partial": inst_partial}
# (instance, tiles, CATCHHIP_FLAT_BANDS, universe_p, changed-word statistics)
CASES = [(name, tiles, bands, None, False)
         for name in ("edges", "tile fill") for tiles in ("striped", "contiguous") for bands in (1, 2)]
CASES += [("partial", "striped", 1, 0.9, False), ("partial", "contiguous", 1, 0.9, False),
          ("edges", "contiguous", 1, None, True), ("edges", "striped", 1, None, True)]     # (the statistics keep one band)
_cache = {}


def case_id(case):
    name, tiles, bands, p, stats = case
    return "%s-%s-%d band%s%s%s" % (name, tiles, bands, "s" if bands > 1 else "", "-p%g" % p if p else "",
                                    "-statistics" if stats else "")


def instance(name, p, oracle):
    """rows, sets, universes, universe_p, the oracle's picks: built once, shared, never changed."""
    key = (name, p)
    if key not in _cache:
        sets, U = INSTANCES[name](np.random.Generator(np.random.PCG64(20261020)))
        r = _table(sets)
        up = None if p is None else [p] * U
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], len(sets), U, None, up, None)
        _cache[key] = (r, len(sets), U, up, list(exp))
    return _cache[key]


def solve_case(ctx, oracle, setenv, case):
    """Solves the case on the device; setenv(name, value) sets a switch of the library.  -> picks, expected picks,
    the four work counters."""
    from catch_amd import engine
    name, tiles, bands, p, stats = case
    r, P, U, up, exp = instance(name, p, oracle)
    setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    setenv("CATCHHIP_FLAT_BANDS", str(bands))
    if tiles == "contiguous":
        setenv("CATCHHIP_FLAT_TILE_SHIFT", str(SHIFT))
    if stats:
        setenv("CATCHHIP_FLAT_COUNT_DIRTY", "1")
    dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], np.full(U, G, dtype=np.int64))
    got = dev.greedy(P, None, up)
    cn = ctx.counters()
    dev.close()
    if p is None:
        assert cn["flat_bands"] == bands, case_id(case)
    return got, exp, {k: cn[k] for k in COUNTERS}


def test_instances_are_what_they_claim_and_the_oracle_solves_them(oracle):
    """No device: the rows sit where the docstrings say, and the oracle's picks cover what the rows cover."""
    for name, p in (("edges", None), ("tile fill", None), ("partial", 0.9)):
        r, P, U, up, exp = instance(name, p, oracle)
        assert 0 < len(exp) <= P and len(set(exp)) == len(exp), name
        assert r.shape[0] <= 6000 and (r[:, 3] - r[:, 2]).max() <= 257
        gx = r[:, 1] * G + r[:, 2]
        ln = r[:, 3] - r[:, 2]
        want = np.zeros(U * G, dtype=bool)
        have = np.zeros(U * G, dtype=bool)
        chosen = np.isin(r[:, 0], exp)
        for x, n, c in zip(gx, ln, chosen):
            want[x:x + n] = True
            if c:
                have[x:x + n] = True
        if p is None:
            assert (want == have).all(), name
        else:
            for u in range(U):
                w, h = want[u * G:(u + 1) * G].sum(), have[u * G:(u + 1) * G].sum()
                assert h + 1 > p * w, (name, u)
        if name == "edges":
            rows = set(zip(gx.tolist(), ln.tolist()))
            lone = [(int(x) & 63, int(n)) for x, n in rows]
            for b in STARTS:
                for n in LENGTHS:
                    assert (b, n) in lone, (b, n)
            assert {(0, 1), (U * G - 1, 1), (4095, 1), (4096, 50), (8191, 1), (8192, 50)} <= rows
            assert any(x < 4096 < x + n for x, n in rows) and any(x < 8192 < x + n for x, n in rows)
            assert (r[:, 0] == 0).sum() == 60 and (r[:, 0] == 1).sum() == 10      # set 1: records 60-69 of its tile
            assert len({int(x) >> SHIFT for x in gx[r[:, 0] <= 1]}) == 1
            assert len({(int(x) >> 12) & 7 for x in gx[r[:, 0] <= 1]}) == 1
            assert (np.bincount(r[:, 0]) == 1).sum() > 100                          # single-row sets
        if name == "tile fill":
            assert tuple(np.bincount(gx >> SHIFT)[:len(TILE_FILL)]) == TILE_FILL
            assert (np.bincount(r[:, 0]) == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_count_launch_picks_and_counters(ctx, oracle, monkeypatch, case):
    got, exp, cn = solve_case(ctx, oracle, monkeypatch.setenv, case)
    print(case_id(case), len(got), "picks", cn)
    assert got == exp
    assert cn["flat_rows_streamed"] > 0                      # the row-parallel kernels ran
    with open(FIXTURE) as f:
        assert cn == json.load(f)[case_id(case)]
