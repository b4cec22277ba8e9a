"""The key-grouped join's wave-wide runs at the edges of their loops.

csrc/scan_join.inc verifies a run -- the W target positions that hold one anchor k-mer against the Q table entries
listed under it -- 64 windows (a chunk) by 64 entries (a block) at a time, per block anchor by anchor, and skips an
anchor that has no entry in the block or no window inside a sequence in the chunk.  These are the cases a change to
those loops can get wrong (written for round 12's software pipeline, which issued the next window's loads ahead of the
tests, passed them and was not kept: DESIGN.md section 4 K1d).  Every case here PLANTS such runs: a master sequence
with a k-mer K that occurs nowhere else, W
copies of it as targets (each a genome of one sequence, a few substitutions outside K, cut at the left or right
where the case says so) and Q probes cut from the master so that K is their anchor a_j (substitutions outside K
again).  The run of K is then exactly W windows by Q entries with the anchors the case names; the k-mers of the
probes' other anchors give further, smaller runs.

Each case is scanned through engine.Rows.scan and compared with a brute-force Hamming scan in NumPy (every probe
against every window of every sequence: <= m mismatches, extended by `ext`, clipped to the sequence, touching ranges
of one set in one genome merged), scanned again with CATCHHIP_SEED_LIST=1 (the seed-list scan: no join) for identical
rows, and its join counters (hit positions, pairs, lane slots of the wave-wide runs, tasks of cut runs) must equal
tests/test_join_pipeline_counters.json, recorded from the commit before round 12.
"""
import contextlib
import functools
import json
import os
import random

import numpy as np
import pytest

from util import rows_as_tuples

KJ_LANES_W, KJ_GIANT_PAIRS = 48, 1 << 15     # csrc/scan_join.inc
COUNTERS = ("join_hit_positions", "join_pairs", "join_lane_slots", "join_cut_tasks")
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_join_pipeline_counters.json")


@contextlib.contextmanager
def _env(**hooks):
    old = {k: os.environ.get(k) for k in hooks}
    try:
        for k, v in hooks.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rs(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s, n, keep):
    """n substitutions of s outside the half-open range `keep`."""
    s = list(s)
    if keep[0] <= 0 and keep[1] >= len(s):
        return "".join(s)
    for _ in range(n):
        while True:
            i = rng.randrange(len(s))
            if not keep[0] <= i < keep[1]:
                break
        s[i] = rng.choice([b for b in "ACGT" if b != s[i]])
    return "".join(s)


class Case:
    """L, m: probe length and mismatches (the pigeonhole k follows); plants: (W, anchors, cut) -- W copies of a
    master, one probe per element of `anchors` with K at that anchor, cut: which copies are cut short ('none';
    'left': all of them, K at their first bases, so that only anchor 0 has a window inside the sequence;
    'left_but_last': all but the last copy; 'left64': the first 64 copies; 'mix': a third at the left, a third at
    the right, where the window of anchor 0 no longer fits); species: also 20 diverged copies of a 1,500-base
    sequence with probes at stride k from the first (short runs, a lane per window); groups / buckets: the two sinks."""

    def __init__(self, name, L, m, plants=(), species=False, groups=False, buckets=False, ext=10, seed=1):
        from catch_amd import probe
        self.name, self.L, self.m, self.ext = name, L, m, ext
        self.k = k = probe.pigeonhole_kmer_length(L, m)
        assert k >= 20 and L % k == 0
        self.nanch, self.ntab = L // k, min(L // k, m + 1)
        rng = random.Random(seed)
        probes, genomes = [], []
        self.runs = []                                   # (W, Q) of the planted k-mers
        for W, anchors, cut in plants:
            assert all(0 <= a < self.ntab for a in anchors)
            kpos = (self.ntab - 1) * k + 3
            master = _rs(rng, kpos + L + 4)
            keep = (kpos, kpos + k)
            mine = []
            while len(mine) < len(anchors):              # distinct probes, K at anchor a
                a = anchors[len(mine)]
                at = kpos - a * k
                p = _mutate(rng, master[at:at + L], rng.randrange(0, m + 2), (a * k, a * k + k))
                if p not in mine and p not in probes:
                    mine.append(p)
            probes += mine
            for w in range(W):
                c = _mutate(rng, master, rng.randrange(0, 3), keep)
                how = {"none": 0, "left": 1, "left_but_last": int(w + 1 < W), "left64": int(w < 64),
                       "mix": (0, 1, 2)[w % 3]}[cut]
                if how == 1:
                    c = c[kpos - rng.randrange(0, min(k, 4)):]
                elif how == 2:
                    c = c[:kpos + L - 1 - rng.randrange(0, 3)]
                genomes.append([c])
            self.runs.append((W, len(anchors)))
        if species:
            base = _rs(rng, 1500)
            for g in range(20):
                genomes.append([_mutate(rng, base, 30 if g else 0, (0, 0))])
            for at in range(0, 1500 - L + 1, k):
                if base[at:at + L] not in probes:
                    probes.append(base[at:at + L])
        self.probes, self.genomes = probes, genomes
        n = len(probes)
        self.owner = np.arange(n, dtype=np.int32) // 2 if buckets else np.arange(n, dtype=np.int32)
        self.pgroup = self.ggroup = None
        if groups:
            self.pgroup = np.array([3 if i % 3 else 7 for i in range(n)], dtype=np.int32)
            self.ggroup = np.array([3 if g % 2 else 7 for g in range(len(genomes))], dtype=np.int32)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """The brute-force rows: (set, genome, start, end), merged."""
        L, m, ext = self.L, self.m, self.ext
        seqs = [g[0] for g in self.genomes]
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(lens)))
        flat = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        win = np.lib.stride_tricks.sliding_window_view(flat, L)
        start = np.arange(win.shape[0], dtype=np.int64)
        sq = np.searchsorted(off, start, side="right") - 1
        inside = start + L <= off[sq + 1]                # the window lies in one sequence
        per = {}
        for p, s in enumerate(self.probes):
            hit = inside & ((win != np.frombuffer(s.encode(), dtype=np.uint8)).sum(axis=1) <= m)
            if self.pgroup is not None:
                hit &= self.ggroup[sq] == self.pgroup[p]
            for i in np.nonzero(hit)[0]:
                g, at = int(sq[i]), int(start[i] - off[sq[i]])
                per.setdefault((int(self.owner[p]), g), []).append((max(0, at - ext), min(int(lens[g]), at + L + ext)))
        rows = []
        for (s, g), iv in per.items():
            iv.sort()
            cs, ce = iv[0]
            for a, b in iv[1:]:
                if a <= ce:
                    ce = max(ce, b)
                else:
                    rows.append((s, g, cs, ce))
                    cs, ce = a, b
            rows.append((s, g, cs, ce))
        return sorted(rows)

    def scan(self, ctx):
        """-> (rows, counters) of one scan of the case."""
        from catch_amd import engine
        n = len(self.probes)
        ep = np.repeat(np.arange(n, dtype=np.int32), self.nanch)
        eo = np.tile(np.arange(self.nanch, dtype=np.int32) * self.k, n)
        t = engine.Targets(ctx, self.genomes)
        p = engine.Probes(ctx, self.probes, self.owner, ep, eo, self.k)
        try:
            if self.pgroup is not None:
                t.set_groups(self.ggroup)
                p.set_groups(self.pgroup)
            rows = engine.Rows.scan(ctx, p, t, self.m, self.L, 0, self.ext, engine.SCAN_SEED)
            cn = ctx.counters()
            sid, un, st, en = rows.fetch()
            rows.close()
        finally:
            p.close(); t.close()
        return rows_as_tuples(sid, un, st, en), cn


def _mixed(q, ntab):
    return [(j * 7 + j // 5) % ntab for j in range(q)]


def _make(name):
    kind, _, arg = name.partition("_")
    if kind == "W":          # window counts: the kj_lanes border, chunk borders
        return Case(name, 100, 2, [(int(arg), [0, 1, 2, 1, 0], "none")], seed=10 + int(arg))
    if kind == "Q":          # entry counts: block borders, a last block of one entry
        return Case(name, 100, 2, [(70, _mixed(int(arg), 3), "none")], seed=200 + int(arg))
    if name == "one_anchor":
        return Case(name, 100, 2, [(70, [1] * 64, "none")], seed=31)
    if name == "no_middle_anchor":
        return Case(name, 100, 2, [(70, [0, 2] * 32, "none")], seed=32)
    if name == "no_valid_lane":          # anchors 1 and 2 have no window inside a sequence, in every chunk
        return Case(name, 100, 2, [(70, _mixed(6, 3), "left")], seed=33)
    if name == "no_valid_lane_first_chunk":   # ... in the first chunk only: the second must not see its windows
        return Case(name, 100, 2, [(70, _mixed(6, 3), "left64")], seed=34)
    if name == "last_lane_only":
        return Case(name, 100, 2, [(64, _mixed(6, 3), "left_but_last")], seed=35)
    if name == "cut_mix":
        return Case(name, 100, 2, [(130, _mixed(66, 3), "mix")], seed=36)
    if name == "giant":                  # 600 x 64 pairs > KJ_GIANT_PAIRS: tasks in both passes
        return Case(name, 100, 2, [(600, _mixed(64, 3), "none")], seed=37)
    if name == "short_runs":             # a lane per window; runs that cross a 64-record chunk of the hit list
        return Case(name, 100, 2, species=True, seed=38)
    if name == "L32_m0":                 # NW = 1
        return Case(name, 32, 0, [(70, [0], "none")], species=True, seed=39)
    if name == "L100_m0":
        return Case(name, 100, 0, [(130, [0], "none")], species=True, seed=40)
    if name == "L250_m2":                # NW = 8
        return Case(name, 250, 2, [(70, _mixed(66, 3), "mix")], seed=41)
    if name == "L126_m4":                # five anchors in the table
        return Case(name, 126, 4, [(70, _mixed(66, 5), "mix")], seed=42)
    if name == "L250_m4":
        return Case(name, 250, 4, [(65, _mixed(65, 5), "none")], seed=43)
    if name == "union":                  # group numbers on probes and targets
        return Case(name, 100, 2, [(70, _mixed(66, 3), "mix"), (50, _mixed(5, 3), "none")], species=True, groups=True, seed=44)
    if name == "buckets":                # two probes per set id
        return Case(name, 100, 2, [(70, _mixed(66, 3), "mix"), (50, _mixed(5, 3), "none")], species=True, buckets=True, seed=45)
    if name == "union_buckets_giant":
        return Case(name, 100, 2, [(600, _mixed(64, 3), "mix")], groups=True, buckets=True, seed=46)
    if name == "mask_store":             # several wave-wide runs and a cut one: with CATCHHIP_MASK_CAP some or all find the store full
        return Case(name, 100, 2, [(129, _mixed(65, 3), "mix"), (70, _mixed(66, 3), "none"), (600, _mixed(64, 3), "none")], seed=47)
    raise KeyError(name)


CASES = (["W_%d" % w for w in (47, 48, 63, 64, 65, 128, 129)] + ["Q_%d" % q for q in (1, 63, 64, 65, 129)] +
         ["one_anchor", "no_middle_anchor", "no_valid_lane", "no_valid_lane_first_chunk", "last_lane_only", "cut_mix",
          "giant", "short_runs", "L32_m0", "L100_m0", "L250_m2", "L126_m4", "L250_m4", "union", "buckets",
          "union_buckets_giant", "mask_store"])


@functools.lru_cache(maxsize=None)
def case(name):
    return _make(name)


def test_cases_plant_what_they_claim():
    """The planted runs have the sizes the cases are named for, on the sides of the borders they are meant to
    straddle, and every case has hits and windows that are not hits."""
    for w in (47, 48, 63, 64, 65, 128, 129):
        assert case("W_%d" % w).runs == [(w, 5)]
    assert 47 < KJ_LANES_W <= 48
    for q in (1, 63, 64, 65, 129):
        assert case("Q_%d" % q).runs == [(70, q)]
    assert set(_mixed(64, 3)) == {0, 1, 2} and set(_mixed(66, 5)) == {0, 1, 2, 3, 4}
    g = case("giant")
    assert g.runs[0][0] * g.runs[0][1] > KJ_GIANT_PAIRS
    assert (case("L32_m0").L + 31) // 32 == 1 and (case("L100_m0").L + 31) // 32 == 4 and (case("L250_m2").L + 31) // 32 == 8
    assert case("L126_m4").ntab == 5 and case("L126_m4").nanch == 6 and case("L100_m0").nanch == 1
    for name in ("W_65", "Q_65", "no_valid_lane", "cut_mix", "L126_m4", "union"):
        c = case(name)
        exp = c.expected()
        assert 0 < len(exp) < len(c.probes) * len(c.genomes)
    assert sorted(json.load(open(RECORD))) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_join_rows_and_counters(ctx, name):
    c = case(name)
    exp = c.expected()
    rows, cn = c.scan(ctx)
    got = [cn[k] for k in COUNTERS]
    print(name, "rows", len(rows), "expected", len(exp), "counters", got)
    assert rows == exp
    assert cn["join_hit_positions"] > 0                  # the join took it
    assert got == json.load(open(RECORD))[name]
    with _env(CATCHHIP_SEED_LIST=1):
        rows1, cn1 = c.scan(ctx)
    assert cn1["join_hit_positions"] == 0 and rows1 == exp
    if name == "giant":
        assert cn["join_cut_tasks"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 64 * 128, 64 * 1024])
def test_mask_store_too_small(ctx, cap):
    """The counting pass keeps its ballots for the writing pass in a store of fixed size; a run that finds its part
    (one of 64) full is verified again by the writing pass, through kj_big's own tests instead of the replay.
    cap = 1: no run fits; 64 x 128 words: a part holds two blocks of one chunk, so the small runs fit and the large
    do not; 64 x 1024: all fit.  Same rows and counters every time."""
    c = case("mask_store")
    exp = c.expected()
    with _env(CATCHHIP_MASK_CAP=cap):
        rows, cn = c.scan(ctx)
    assert rows == exp
    assert [cn[k] for k in COUNTERS] == json.load(open(RECORD))["mask_store"]
    assert all(v == 0 for v in ctx.capacity_events().values())
