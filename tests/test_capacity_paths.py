"""Every capacity re-run and beyond-the-cap fallback, at test size.

Many device lists of the library are sized by an estimate: a kernel counts past the capacity without writing past it,
the host reads the count and runs again at the exact size, or takes a slower exact path.  The floors of those
capacities are 2^14 .. 2^28, which no test input reaches, so each has a test hook that replaces the FIRST capacity
(csrc/internal.h: chip_test_env_int; README.md lists them) and `Context.capacity_events()` says whether the host took
the recovery path.  Every GPU test here runs one input with the hook unset and set and asserts

  1. the same result, equal to the CPU oracle's where the neighbouring tests compare that operation with the oracle;
  2. the path's entry of capacity_events() is >= 1 with the hook and 0 without it (a forced path that is not taken
     fails the test), and no other entry moved;
  3. nothing else changed: the device memory in use (engine.pool_stats(): held minus idle in the cache) is what it
     was before the pair of calls, as tests/test_error_paths.py checks it.

The CPU tests (unmarked) keep the inputs honest: they restate on the host the quantity each forced capacity is
compared with and assert that it exceeds the cap, or brackets it for the "exact" / "one below" cases.

The fixed in-kernel limits of the solvers (GW_MAXWSEG, GR_USEL_CAP) have no hook: their tests build tables that
cross them and check through the solver counters that the kernel in question ran.
"""
import contextlib
import functools
import gc
import os
import random

import numpy as np
import pytest

from util import candidates, rows_as_tuples, small_species

EVENTS = ("seed_list_rerun", "general_seed_rerun", "byte_join_rerun", "fast_hit_rerun", "cut_list_fallback",
          "giant_task_fallback", "ndf_edge_rerun", "_")
ES_SHARDS = 64              # csrc/ndf.hip: shards of the edge list and of the queue of deferred walks
KJ_GIANT_PAIRS = 1 << 15    # csrc/scan_join.inc: pairs of one run a single wavefront takes; beyond: tasks of fewer entries

SEED_CAP, BYTE_JOIN_CAP, FAST_HIT_CAP, CUT_CAP, GIANT_CAP, NDF_EDGE_CAP = 100, 50, 64, 8, 1, 4


def _oracle():
    from oracle import oracle as o
    o.build()
    return o


@contextlib.contextmanager
def _env(**hooks):
    """The hooks set for the duration of the block (the library reads a hook at every decision, never caches it)."""
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


def _in_use(engine):
    st = engine.pool_stats()
    return st["bytes_held"] - st["bytes_cached_free"]


@contextlib.contextmanager
def _nothing_else_changed():
    """Device memory in use after the block is what it was before it."""
    from catch_amd import engine
    gc.collect()
    before = _in_use(engine)
    yield
    gc.collect()
    assert _in_use(engine) == before


def _only(events, name, forced):
    """The event `name` happened (forced) or did not, and no other one did."""
    assert set(events) == set(EVENTS)
    for k, v in events.items():
        if k == name and forced:
            assert v >= 1, events
        else:
            assert v == 0, events


# ====================================================================== the record of capacity events
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("CATCHHIP_SEED_CAP", "CATCHHIP_BYTE_JOIN_CAP", "CATCHHIP_FAST_HIT_CAP", "CATCHHIP_CUT_CAP",
         "CATCHHIP_GIANT_CAP", "CATCHHIP_NDF_EDGE_CAP", "CATCHHIP_NDF_QUEUE_SEGCAP")


def test_capacity_events_symbol_is_declared_bound_exported_and_wrapped():
    """catchhip_ctx_last_capacity_events: in the header (under the bumped ABI version), in the bindings, exported by
    the built library, wrapped by Context.capacity_events() under the names this file uses; the hooks are read in
    the sources as integer hooks and README.md lists them."""
    import re
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib, engine
    name = "catchhip_ctx_last_capacity_events"
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint %s\s*\(catchhip_ctx \*ctx, int64_t \*out8\)" % name, hdr)
    assert "#define CATCHHIP_ABI_VERSION 2\n" in hdr
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 2
    L = _lib.lib()
    assert hasattr(L, name) and L.catchhip_abi_version() == 2
    assert engine.Context.CAPACITY_EVENTS == EVENTS and callable(engine.Context.capacity_events)
    src = "".join(open(os.path.join(REPO, "catch_amd", "csrc", f)).read() for f in ("scan.hip", "ndf.hip"))
    readme = open(os.path.join(REPO, "README.md")).read()
    for hook in HOOKS:
        assert '"%s"' % hook in src and "`%s" % hook in readme, hook
    # one index per kind, as the header documents them
    ih = open(os.path.join(REPO, "catch_amd", "csrc", "internal.h")).read()
    kinds = re.findall(r"\bCAPEV_[A-Z_]+ = (\d)", ih)
    assert kinds == [str(i) for i in range(7)] and "i64 capacity_events[8]" in ih


# ====================================================================== the scan inputs
class ScanCase:
    """Probes with their anchor table, targets, scan parameters and the oracle's rows."""

    def __init__(self, genomes, strs, m, thres, island, ext, min_k=20, np_seed=None):
        o = _oracle()
        if np_seed is not None:
            np.random.seed(np_seed)       # (random anchor tables: the reference draws them from np.random)
        self.k, self.entries = o.anchor_table(strs, m, thres, min_k=min_k, k=min_k)
        self.uniq, owner = o._unique_last(strs)
        self.owner = np.array(owner, dtype=np.int32)
        self.genomes, self.m, self.thres, self.island, self.ext = genomes, m, thres, island, ext
        pr, un, st, en = o.make_sets(self.uniq, self.entries, self.k, genomes, m, thres, island, ext)
        self.exp = rows_as_tuples(self.owner[pr] if pr.size else pr, un, st, en)
        self.seqs = [s for g in genomes for s in g]

    def kmer_matches(self, pos_limit=None):
        """(sequence, position, entry) of every exact match of an anchor k-mer inside one sequence: the seeds of a
        scan whose table holds the anchors below pos_limit (None: all of them)."""
        table = {}
        for e, (p, a) in enumerate(self.entries):
            if pos_limit is None or a < pos_limit:
                table.setdefault(self.uniq[p][a:a + self.k], []).append(e)
        out = []
        for si, s in enumerate(self.seqs):
            for i in range(len(s) - self.k + 1):
                for e in table.get(s[i:i + self.k], ()):
                    out.append((si, i, e))
        return out

    def cut_windows(self):
        """Of kmer_matches(): the seeds whose probe-long window (the probe laid on the sequence so that the anchor
        lies on its match) crosses an end of the sequence -- what extend_planes_one defers to the cut list."""
        L = len(self.uniq[0])
        n = 0
        for si, i, e in self.kmer_matches():
            a = self.entries[e][1]
            n += i < a or i - a + L > len(self.seqs[si])
        return n

    def device(self, ctx):
        from catch_amd import engine
        ep = np.array([e[0] for e in self.entries], dtype=np.int32)
        eo = np.array([e[1] for e in self.entries], dtype=np.int32)
        return engine.Targets(ctx, self.genomes), engine.Probes(ctx, self.uniq, self.owner, ep, eo, self.k)

    def scan(self, ctx, mode, first_seen=False):
        """-> (rows, first-seen keys or None, work counters, capacity events) of one scan."""
        from catch_amd import engine
        t, p = self.device(ctx)
        try:
            if first_seen:
                rows = engine.Rows.scan_first_seen(ctx, p, t, self.m, self.thres, self.island, self.ext, mode,
                                                   np.arange(len(self.entries), dtype=np.uint32))
            else:
                rows = engine.Rows.scan(ctx, p, t, self.m, self.thres, self.island, self.ext, mode)
            counters, events = ctx.counters(), ctx.capacity_events()
            sid, un, st, en = rows.fetch()
            keys = None
            if first_seen:
                order = np.lexsort((st, un, sid))
                keys = rows.fetch_first_seen()[order].tolist()
            rows.close()
        finally:
            p.close(); t.close()
        return rows_as_tuples(sid, un, st, en), keys, counters, events


@functools.lru_cache(maxsize=None)
def seed_case():
    genomes = small_species(seed=8)
    return ScanCase(genomes, candidates(genomes, 100, 50), 2, 100, 0, 50)


@functools.lru_cache(maxsize=None)
def general_case():
    genomes = small_species(seed=8)
    return ScanCase(genomes, candidates(genomes, 100, 50), 5, 100, 0, 50, np_seed=12)    # -m 5: random anchors of 20


@functools.lru_cache(maxsize=None)
def alphabet_case():
    rng = random.Random(9)
    alpha = "ABCDEFGHIJKLMNOPQRSTUVWXYZacgt"
    seq = "".join(rng.choice(alpha) for _ in range(600))
    genomes = [[seq], [seq[100:400].lower() + seq[400:]]]
    return ScanCase(genomes, [seq[i:i + 20] for i in range(0, 580, 7)], 1, 20, 0, 2, min_k=5)


@functools.lru_cache(maxsize=None)
def cut_case():
    """Genomes in pieces of 60 .. 210 bases (no N: the k-mer matches are the device's seeds exactly), probes of 100
    from the whole genomes, a cover threshold of 60: every seed near the end of a piece has its window cut."""
    whole = small_species(seed=23, n=3, length=2500, with_n=False)
    lengths = [130, 70, 210, 95, 160, 60, 185]
    genomes = []
    for g in whole:
        s, at, i, pieces = g[0], 0, 0, []
        while at < len(s):
            pieces.append(s[at:at + lengths[i % len(lengths)]])
            at += lengths[i % len(lengths)]
            i += 1
        genomes.append(pieces)
    return ScanCase(genomes, candidates(whole, 100, 25), 2, 60, 0, 10, np_seed=5)


@functools.lru_cache(maxsize=None)
def giant_case():
    """The 700-copy input of test_scan_repeats_fill_large_buckets plus 60 probes one mismatch (in the last anchor,
    which -m 2 keeps out of the table) from the unit's first 100 bases: the k-mers of the unit's first three anchors
    are then found at 700 positions and belong to more than 60 table entries each -- more than KJ_GIANT_PAIRS
    (position, entry) pairs in one run, which the join cuts into tasks."""
    rng = random.Random(700)

    def rs(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    unit = rs(150)
    g0 = "".join(unit + rs(30) for _ in range(700))
    genomes = [[g0], [rs(400) + unit + rs(300)]]
    strs = candidates([[unit + rs(50)], [g0[:2000]]], 100, 25)
    for j in range(60):
        q = 75 + j % 25
        b = "ACGT"[("ACGT".index(unit[q]) + 1 + j // 25) % 4]
        strs.append(unit[:q] + b + unit[q + 1:100])
    strs = list(dict.fromkeys(strs))
    return ScanCase(genomes, strs, 2, 100, 0, 20)


def giant_tasks(case):
    """Tasks the join cuts its runs into: a run = the W positions of one k-mer, Q = the table entries of that k-mer
    (anchors below (m + 1) k); beyond KJ_GIANT_PAIRS pairs it becomes ceil(Q / (KJ_GIANT_PAIRS // W)) tasks."""
    W, Q = {}, {}
    for si, i, e in case.kmer_matches((case.m + 1) * case.k):
        km = case.seqs[si][i:i + case.k]
        W.setdefault(km, set()).add((si, i))
        Q.setdefault(km, set()).add(e)
    tasks = 0
    for km in W:
        w, q = len(W[km]), len(Q[km])
        if w * q > KJ_GIANT_PAIRS:
            tasks += -(-q // max(1, KJ_GIANT_PAIRS // w))
    return tasks


def tiled_hits(case):
    """Hits of the tiled scan: every (probe, window) within m mismatches = the oracle's unmerged cover ranges."""
    o = _oracle()
    return sum(len(v) for s in case.seqs
               for v in o.scan_sequence(s, case.uniq, case.entries, case.k, case.m, case.thres, case.island,
                                        merge=False).values())


# ---------------------------------------------------------------------- CPU: the scan inputs are not vacuous
def test_scan_inputs_cross_their_forced_capacities():
    """The quantity each forced capacity is compared with, restated on the host.  The seed lists hold at least the
    exact k-mer matches (the packed keys ignore N, and the seed-list scan's filtered look-up pads every tile's
    share to 64 entries), so the host's count is a lower bound there and the GPU tests take the exact figure from
    the unforced run's work counter; the cut windows of the N-free cut case are restated exactly."""
    c = seed_case()
    assert c.k == 25 and len(c.kmer_matches((c.m + 1) * c.k)) > SEED_CAP
    g = general_case()
    assert g.k == 20 and len(g.kmer_matches()) > SEED_CAP
    assert any(a % 20 for _, a in g.entries)             # (random anchors, not the pigeonhole ones)
    a = alphabet_case()
    assert len(a.kmer_matches()) > BYTE_JOIN_CAP
    assert tiled_hits(c) > FAST_HIT_CAP
    cut = cut_case()
    ncut = cut.cut_windows()
    assert 200 <= ncut < len(cut.kmer_matches()) and ncut > CUT_CAP
    assert len(cut.exp) > 100
    gi = giant_case()
    assert giant_tasks(gi) >= 2 > GIANT_CAP
    assert all(len(x.exp) > 30 for x in (c, g, a, gi))


# ---------------------------------------------------------------------- GPU: the scans
def _scan_pair(ctx, case, mode, event, hooks, first_seen=False, base_hooks=None):
    """One scan with `hooks` unset and one with them set (base_hooks: set in both): same rows as the oracle, the
    event only in the forced run, the memory in use as before.  -> the two runs' work counters."""
    base_hooks = base_hooks or {}
    with _nothing_else_changed():
        with _env(**base_hooks):
            rows0, keys0, c0, e0 = case.scan(ctx, mode, first_seen)
            with _env(**hooks):
                rows1, keys1, c1, e1 = case.scan(ctx, mode, first_seen)
    assert rows0 == case.exp
    assert rows1 == case.exp
    assert keys1 == keys0
    _only(e0, event, False)
    _only(e1, event, True)
    return c0, c1, e1


@pytest.mark.gpu
@pytest.mark.parametrize("first_seen", [False, True])
def test_seed_list_rerun(ctx, first_seen):
    """The seed-list scan's work list (scan.hip: scan_and_group): too small at 100 entries, and exactly at / one
    below the count of the unforced run, with the compact records of a cover scan and with the one-record-per-seed
    form of a first-seen scan.  (CATCHHIP_SEED_LIST: the key-grouped join would take these pigeonhole probes
    otherwise, and it has no work list.)  The list's length is not restated on the host -- the filtered look-up pads
    every tile's share to 64 entries and its keys ignore N; the host's exact k-mer matches are a lower bound -- so
    the exact figure is the unforced run's work counter and the event count is the guard: one below it must re-run,
    the figure itself must not."""
    from catch_amd import engine
    case = seed_case()
    base = {"CATCHHIP_SEED_LIST": 1}
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_SEED, "seed_list_rerun", {"CATCHHIP_SEED_CAP": SEED_CAP}, first_seen, base)
    n = c0["seed_hits"]                                   # entries of the work list: what the capacity is compared with
    assert n == c1["seed_hits"] > SEED_CAP and n >= len(case.kmer_matches((case.m + 1) * case.k))
    assert c0["join_hit_positions"] == 0 and e1["seed_list_rerun"] == 1
    with _nothing_else_changed(), _env(**base):
        for cap, rerun in ((n, 0), (n - 1, 1)):
            with _env(CATCHHIP_SEED_CAP=cap):
                rows, _, c, e = case.scan(ctx, engine.SCAN_SEED, first_seen)
            assert rows == case.exp and c["seed_hits"] == n
            assert e["seed_list_rerun"] == rerun, (cap, n, e)


@pytest.mark.gpu
def test_general_scan_seed_rerun(ctx):
    """The work list of the general scan's table look-up (run_general), random anchors, -m 5."""
    from catch_amd import engine
    case = general_case()
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_GENERAL, "general_seed_rerun", {"CATCHHIP_SEED_CAP": SEED_CAP})
    assert c0["seed_hits"] == c1["seed_hits"] >= len(case.kmer_matches()) > SEED_CAP
    assert e1["general_seed_rerun"] == 1


@pytest.mark.gpu
def test_byte_hash_join_rerun(ctx):
    """The match list of the general scan's join of byte hashes (any alphabet)."""
    from catch_amd import engine
    case = alphabet_case()
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_AUTO, "byte_join_rerun", {"CATCHHIP_BYTE_JOIN_CAP": BYTE_JOIN_CAP})
    assert c0["seed_hits"] == c1["seed_hits"] >= len(case.kmer_matches()) > BYTE_JOIN_CAP
    assert e1["byte_join_rerun"] == 1


@pytest.mark.gpu
def test_tiled_scan_hit_rerun(ctx):
    """The hit list of the tiled cross-check scan (run_fast)."""
    from catch_amd import engine
    case = seed_case()
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_FAST, "fast_hit_rerun", {"CATCHHIP_FAST_HIT_CAP": FAST_HIT_CAP})
    assert c0["raw_hits"] == c1["raw_hits"] > FAST_HIT_CAP          # (the hits: what the capacity is compared with)
    assert e1["fast_hit_rerun"] == 1
    with _env(CATCHHIP_FAST_HIT_CAP=c0["raw_hits"]):      # exactly enough: no re-run
        rows, _, _, e = case.scan(ctx, engine.SCAN_FAST)
    assert rows == case.exp
    _only(e, "fast_hit_rerun", False)


@pytest.mark.gpu
def test_cut_list_fallback(ctx):
    """The general scan's list of windows cut by a sequence end (extend_planes_one files them, extend_cut_kernel
    extends them by bytes): with room for 8 of the few hundred the host resets the hit count and extends EVERY seed
    by bytes (extend_kernel); with room for exactly the host's count of cut windows it does not, with one fewer it
    does -- so that count is the device's."""
    from catch_amd import engine
    case = cut_case()
    ncut = case.cut_windows()
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_GENERAL, "cut_list_fallback", {"CATCHHIP_CUT_CAP": CUT_CAP})
    assert c0["seed_hits"] == c1["seed_hits"] == len(case.kmer_matches())
    assert c0["raw_hits"] == c1["raw_hits"]
    with _nothing_else_changed():
        for cap, fallback in ((ncut, 0), (ncut - 1, 1)):
            with _env(CATCHHIP_CUT_CAP=cap):
                rows, _, c, e = case.scan(ctx, engine.SCAN_GENERAL)
            assert rows == case.exp and c["raw_hits"] == c0["raw_hits"]
            assert e["cut_list_fallback"] == fallback, (cap, e)
    # ... and under a first-seen scan, whose hits carry their seed
    _scan_pair(ctx, case, engine.SCAN_GENERAL, "cut_list_fallback", {"CATCHHIP_CUT_CAP": CUT_CAP}, first_seen=True)


@pytest.mark.gpu
def test_giant_task_fallback(ctx):
    """The key-grouped join's list of tasks of cut runs (run_join): with room for one task the join is abandoned
    after its counting pass has written bucket counts, and the seed-list scan runs in its place -- the oracle's rows,
    no join counters, the event.  Then the same through the fused filter, which takes over the bucket state."""
    from catch_amd import engine
    case = giant_case()
    c0, c1, e1 = _scan_pair(ctx, case, engine.SCAN_SEED, "giant_task_fallback", {"CATCHHIP_GIANT_CAP": GIANT_CAP})
    assert c0["join_cut_tasks"] >= 2 and c0["join_hit_positions"] > 0, c0      # (otherwise the input proves nothing)
    assert [c1[k] for k in ("join_hit_positions", "join_pairs", "join_lane_slots", "join_cut_tasks")] == [0, 0, 0, 0]
    assert c1["seed_hits"] > 0 and e1["giant_task_fallback"] == 1
    with _env(CATCHHIP_GIANT_CAP=c0["join_cut_tasks"]):   # exactly enough: the join goes through
        rows, _, c, e = case.scan(ctx, engine.SCAN_SEED)
    assert rows == case.exp and c["join_cut_tasks"] == c0["join_cut_tasks"]
    _only(e, "giant_task_fallback", False)
    # the fused filter (its synchronous branch: the queued one of small instances never joins), full and partial cover
    nsets, o, r = len(case.uniq), _oracle(), np.array(case.exp)
    glen = [sum(map(len, g)) for g in case.genomes]
    with _nothing_else_changed():
        t, p = case.device(ctx)
        for up in (None, [0.95] * len(case.genomes)):
            rows = engine.Rows.scan(ctx, p, t, case.m, case.thres, case.island, case.ext)
            want = (rows.greedy(nsets, None, up), rows.n)
            rows.close()
            assert want[1] == len(case.exp) and want[0] == o.lazy_greedy(r[:, 0], r[:, 1], r[:, 2], r[:, 3], nsets, glen, up)
            with _env(CATCHHIP_FILTER_NO_DEFER=1):
                got0 = engine.setcover_filter(ctx, p, t, case.m, case.thres, case.island, case.ext, nsets, None, up)
                ev0, cn0 = ctx.capacity_events(), ctx.counters()
                with _env(CATCHHIP_GIANT_CAP=GIANT_CAP):
                    got1 = engine.setcover_filter(ctx, p, t, case.m, case.thres, case.island, case.ext, nsets, None, up)
                    ev1, cn1 = ctx.capacity_events(), ctx.counters()
            assert got0 == want and got1 == want
            assert cn0["join_cut_tasks"] >= 2 and cn1["join_cut_tasks"] == 0 and cn1["join_hit_positions"] == 0
            _only(ev0, "giant_task_fallback", False)
            _only(ev1, "giant_task_fallback", True)
        p.close(); t.close()


# ====================================================================== the near-duplicate filters
HAM_D, HAM_L, MH_D, MH_KMER = 2, 100, 0.5, 10


@functools.lru_cache(maxsize=None)
def ndf_species():
    """52 strains in 2 clades (windows of one clade are a few mismatches apart: near-duplicates)."""
    return small_species(seed=31, n=52, length=3000, d1=0.05, d2=0.008)


@functools.lru_cache(maxsize=None)
def ndf_strs():
    return tuple(candidates(ndf_species(), HAM_L, 50))           # about 2,000 distinct candidates


@functools.lru_cache(maxsize=None)
def ndf_small():
    """64 candidates: the distinct ones among the first 8 windows of the strains of one clade.  The edge kernels shard by sorted slot / 64, so
    ALL edges of so few probes are in shard 0 and the fullest shard's count is the total, which the host restates."""
    sp = ndf_species()
    out = list(dict.fromkeys(s for g in sp[0::2] for s in candidates([g], HAM_L, 50)[:8]))
    return tuple(out[:64])


def ndf_groups3():
    sp = ndf_species()
    return [sp[0:18], sp[18:35], sp[35:52]]


def hamming_positions(seed=99, groups=None):
    o = _oracle()
    random.seed(seed)
    nt = o.lsh_num_tables(HAM_D, HAM_L, 20)
    if groups is None:
        return o.lsh_draw_positions(nt, 20, HAM_L)
    return [o.lsh_draw_positions(nt, 20, HAM_L) for _ in range(groups)]


def minhash_params(seed=77, groups=None):
    o = _oracle()
    random.seed(seed)
    nt = o.minhash_num_tables(MH_D)
    if groups is None:
        return o.minhash_draw_params(nt, 3)
    return [o.minhash_draw_params(nt, 3) for _ in range(groups)]


def _near_pairs(keys_per_table, near):
    """Per table, the pairs that share a bucket and are near: [set of (i, j), i < j]."""
    out = []
    for keys in keys_per_table:
        buckets = {}
        for i, key in enumerate(keys):
            buckets.setdefault(key, []).append(i)
        pairs = set()
        for b in buckets.values():
            for x in range(len(b)):
                for y in range(x + 1, len(b)):
                    if near(b[x], b[y]):
                        pairs.add((b[x], b[y]))
        out.append(pairs)
    return out


def hamming_edges(strs, positions):
    """Edges the Hamming edge kernel lists: per table, the pairs that agree at the table's positions and differ in at
    most HAM_D characters (with fewer than four tables a pair is listed once per table it meets in)."""
    arr = np.frombuffer("".join(strs).encode("latin-1"), dtype=np.uint8).reshape(len(strs), -1)
    assert len(positions) < 4
    keys = [[arr[i, pos].tobytes() for i in range(len(strs))] for pos in positions]
    return sum(len(p) for p in _near_pairs(keys, lambda i, j: int(np.count_nonzero(arr[i] != arr[j])) <= HAM_D))


def minhash_edges(strs, params):
    """Edges the MinHash edge kernel lists: the distinct pairs with the same signature in some table whose k-mer sets
    are within MH_D (a pair that met in an earlier table is not compared again)."""
    o = _oracle()
    L = o.lib()

    def sig(s, fns):
        b = o._bytes_arr(s)
        return tuple(int(L.orc_minhash(o._p(b, o._u8p), len(s), MH_KMER, a_, b_)) for a_, b_ in fns)
    keys = [[sig(s, fns) for s in strs] for fns in params]
    kmers = [set(s[i:i + MH_KMER] for i in range(len(s) - MH_KMER + 1)) for s in strs]

    def near(i, j):
        return 1.0 - float(len(kmers[i] & kmers[j])) / len(kmers[i] | kmers[j]) <= MH_D
    return len(set().union(*_near_pairs(keys, near)))


def test_ndf_inputs_cross_their_forced_capacities():
    """More edges than 64 shards of 4 hold, whatever the sharding (the large input; in three groups too: a pair of one
    group is a pair of the whole), and enough edges among the 64 probes of the small input to bracket a capacity."""
    strs = list(ndf_strs())
    assert 1800 <= len(strs) <= 2200
    assert hamming_edges(strs, hamming_positions()) > NDF_EDGE_CAP * ES_SHARDS
    assert minhash_edges(strs, minhash_params()) > NDF_EDGE_CAP * ES_SHARDS
    small = list(ndf_small())
    assert len(small) == 64
    assert hamming_edges(small, hamming_positions()) > NDF_EDGE_CAP + 1
    assert minhash_edges(small, minhash_params()) > NDF_EDGE_CAP + 1
    groups = [candidates(g, HAM_L, 50) for g in ndf_groups3()]
    for g, pos, par in zip(groups, hamming_positions(groups=3), minhash_params(groups=3)):
        assert hamming_edges(g, pos) > NDF_EDGE_CAP * ES_SHARDS
        assert minhash_edges(g, par) > NDF_EDGE_CAP * ES_SHARDS


def _ndf_pair(ctx, call, hooks):
    """`call()` -> the kept probes, in the edge-list form with the cap unset and set: the same, the event only in the
    forced run, the memory in use as before.  -> (kept, edges the unforced run listed)."""
    with _nothing_else_changed():
        with _env(CATCHHIP_NDF_ALL_PAIRS=1, CATCHHIP_MH_ALL_PAIRS=1):
            kept0 = call()
            e0, edges = ctx.capacity_events(), ctx.ndf_counters()["edges"]
            with _env(**hooks):
                kept1 = call()
                e1 = ctx.capacity_events()
                assert ctx.ndf_counters()["edges"] == edges
    assert kept1 == kept0
    _only(e0, "ndf_edge_rerun", False)
    _only(e1, "ndf_edge_rerun", True)
    assert e1["ndf_edge_rerun"] == 1
    return kept0, edges


@pytest.mark.gpu
def test_ndf_hamming_edge_rerun(ctx):
    """The Hamming filter's edge list (the form CATCHHIP_NDF_ALL_PAIRS selects; the lazy resolution has no list):
    4 edges per shard, one group.  Which shard an edge falls into follows the device's sort of hashed keys and is not
    restated on the host: the host's total (equal to the device's) exceeds what all 64 shards hold, and the event
    count is the guard; test_ndf_edge_capacity_exact_and_one_below brackets a capacity where one shard takes all."""
    o = _oracle()
    strs, pos = list(ndf_strs()), hamming_positions()
    kept, edges = _ndf_pair(ctx, lambda: ctx.ndf_hamming(strs, HAM_L, pos, HAM_D).tolist(), {"CATCHHIP_NDF_EDGE_CAP": NDF_EDGE_CAP})
    assert edges == hamming_edges(strs, pos)
    assert [s for s, kp in zip(strs, kept) if kp] == o.ndf_hamming(strs, HAM_D, pos, inclusion_order=True)
    assert 0 < sum(kept) < len(strs)
    assert ctx.ndf_hamming(strs, HAM_L, pos, HAM_D).tolist() == kept       # the lazy resolution
    _only(ctx.capacity_events(), "ndf_edge_rerun", False)


@pytest.mark.gpu
def test_ndf_hamming_edge_rerun_three_groups(ctx):
    """... and three groups in one call (candidates of grouped targets, positions drawn per group)."""
    from catch_amd import engine
    o = _oracle()
    groups = ndf_groups3()
    genomes = [g for grp in groups for g in grp]
    flat = "".join(s for g in genomes for s in g)
    pos = hamming_positions(groups=3)
    t = engine.Targets(ctx, genomes)
    t.set_groups(np.repeat(np.arange(3), [len(g) for g in groups]))

    def call():
        c = engine.Candidates(ctx, t, HAM_L, 50)
        c.ndf_hamming_many(pos, HAM_D)
        out = list(zip(c.groups().tolist(), (flat[p:p + HAM_L] for p in c.positions().tolist())))
        c.close()
        return out
    kept, _ = _ndf_pair(ctx, call, {"CATCHHIP_NDF_EDGE_CAP": NDF_EDGE_CAP})
    for gi, grp in enumerate(groups):
        want = o.ndf_hamming(candidates(grp, HAM_L, 50, dedup=False), HAM_D, pos[gi], inclusion_order=True)
        assert sorted(s for g, s in kept if g == gi) == sorted(want)
    assert call() == kept                                                    # the lazy resolution
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ngroups", [1, 3])
def test_ndf_minhash_edge_rerun(ctx, ngroups):
    """The MinHash filter's edge list (CATCHHIP_MH_ALL_PAIRS), one group and three."""
    o = _oracle()
    if ngroups == 1:
        strs, par = list(ndf_strs()), minhash_params()
        kept, edges = _ndf_pair(ctx, lambda: ctx.ndf_minhash(strs, MH_KMER, par, MH_D).tolist(), {"CATCHHIP_NDF_EDGE_CAP": NDF_EDGE_CAP})
        assert edges == minhash_edges(strs, par)
        assert [s for s, kp in zip(strs, kept) if kp] == o.ndf_minhash(strs, MH_D, par, MH_KMER, inclusion_order=True)
        assert 0 < sum(kept) < len(strs)
        assert ctx.ndf_minhash(strs, MH_KMER, par, MH_D).tolist() == kept   # the lazy resolution
    else:
        groups = [candidates(g, HAM_L, 50) for g in ndf_groups3()]
        par = minhash_params(groups=3)
        kept, _ = _ndf_pair(ctx, lambda: [k.tolist() for k in ctx.ndf_minhash_many(groups, MH_KMER, par, MH_D)],
                            {"CATCHHIP_NDF_EDGE_CAP": NDF_EDGE_CAP})
        for g, kp, pr in zip(groups, kept, par):
            assert [s for s, x in zip(g, kp) if x] == o.ndf_minhash(g, MH_D, pr, MH_KMER, inclusion_order=True)
        assert [k.tolist() for k in ctx.ndf_minhash_many(groups, MH_KMER, par, MH_D)] == kept
    _only(ctx.capacity_events(), "ndf_edge_rerun", False)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["hamming", "minhash"])
def test_ndf_edge_capacity_exact_and_one_below(ctx, family):
    """64 probes, whose edges all fall into shard 0: a capacity of exactly the host's edge count does not re-run, one
    below it does, and both keep what the oracle keeps."""
    o = _oracle()
    strs = list(ndf_small())
    if family == "hamming":
        pos = hamming_positions()
        n = hamming_edges(strs, pos)
        want = o.ndf_hamming(strs, HAM_D, pos, inclusion_order=True)
        call = lambda: ctx.ndf_hamming(strs, HAM_L, pos, HAM_D).tolist()
    else:
        par = minhash_params()
        n = minhash_edges(strs, par)
        want = o.ndf_minhash(strs, MH_D, par, MH_KMER, inclusion_order=True)
        call = lambda: ctx.ndf_minhash(strs, MH_KMER, par, MH_D).tolist()
    assert 0 < len(want) < len(strs)
    with _nothing_else_changed(), _env(CATCHHIP_NDF_ALL_PAIRS=1, CATCHHIP_MH_ALL_PAIRS=1):
        for cap, rerun in ((None, 0), (n, 0), (n - 1, 1), (NDF_EDGE_CAP, 1)):
            with _env(**({} if cap is None else {"CATCHHIP_NDF_EDGE_CAP": cap})):
                kept = call()
            assert [s for s, kp in zip(strs, kept) if kp] == want
            assert ctx.ndf_counters()["edges"] == n
            assert ctx.capacity_events()["ndf_edge_rerun"] == rerun, (cap, n)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["hamming", "minhash"])
def test_ndf_queue_overflow_is_an_error_and_leaves_nothing_behind(ctx, family):
    """The queue of deferred walks of the lazy resolution: a segment of one entry per shard is too small for the
    walks these near-duplicates defer; the guarded write drops them and the call fails with its own message (there
    is no re-run: the segment's real size cannot be exceeded).  The next call on the same context is right."""
    from catch_amd import engine
    o = _oracle()
    strs = list(ndf_strs())
    if family == "hamming":
        pos = hamming_positions()
        want = o.ndf_hamming(strs, HAM_D, pos, inclusion_order=True)
        call = lambda: ctx.ndf_hamming(strs, HAM_L, pos, HAM_D).tolist()
    else:
        par = minhash_params()
        want = o.ndf_minhash(strs, MH_D, par, MH_KMER, inclusion_order=True)
        call = lambda: ctx.ndf_minhash(strs, MH_KMER, par, MH_D).tolist()
    with _nothing_else_changed():
        assert [s for s, kp in zip(strs, call()) if kp] == want
        with _env(CATCHHIP_NDF_QUEUE_SEGCAP=1):
            with pytest.raises(ValueError, match="queue of deferred walks overflowed"):
                call()
        ctx.sync()
        assert [s for s, kp in zip(strs, call()) if kp] == want
        assert all(v == 0 for v in ctx.capacity_events().values())


# ====================================================================== fixed in-kernel limits of the solvers
GW_MAXWSEG = 4096      # csrc/setcover.hip: (set, universe) segments of a winner with an LDS counter of cleared bits
GR_USEL_CAP = 3072     # csrc/setcover_flat.inc: words with uncovered bits that gr_usel_kernel lists in LDS

# the solver forms the suite switches between: hooks, and whether the one-workgroup solver (greedy_wg_kernel) takes a
# full-coverage / a partial-coverage instance under them
SOLVER_FORMS = {
    "default": ({}, False, False),
    "eager": ({"CATCHHIP_PARTIAL_SEQUENTIAL": 1}, False, True),
    "sequential": ({"CATCHHIP_GREEDY_SEQUENTIAL": 1}, True, True),
    "flat": ({"CATCHHIP_FLAT_MIN_ROWS": 0}, False, False),
}


def _solve(ctx, r, glen, nsets, up, hooks):
    from catch_amd import engine
    dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
    try:
        with _env(**hooks):
            got = dev.greedy(nsets, None, up)
            cn = ctx.counters()
    finally:
        dev.close()
    return got, cn


def _ran_one_workgroup_solver(cn, r, picks):
    """greedy_wg_kernel counts the rows of every winner it applies; the frontier solver reports 0 there and the
    row-parallel one its streamed records (and its own counters)."""
    per_set = np.bincount(r[:, 0])
    return cn["flat_rows_streamed"] == 0 and cn["winner_rows"] == int(per_set[picks].sum())


@functools.lru_cache(maxsize=None)
def wseg_table(nuniv):
    """nuniv universes of 128 bases; set 0 has one 100-base row in every universe (its segments are the universes,
    in order: those from GW_MAXWSEG on have no LDS counter); 300 further sets of 1 - 3 rows in random universes,
    every third of them with a row among the last universes, sets 1 and 2 in the very last one."""
    rng = np.random.Generator(np.random.PCG64(5))
    rows = [(0, u, 10, 110) for u in range(nuniv)]
    rows += [(1, nuniv - 1, 60, 128), (2, nuniv - 1, 0, 40)]
    for s in range(1, 301):
        us = set(int(x) for x in rng.integers(0, nuniv, size=int(rng.integers(1, 4))))
        if s % 3 == 0:
            us.add(int(rng.integers(nuniv - 100, nuniv)))
        for u in sorted(us - {nuniv - 1} if s in (1, 2) else us):
            a = int(rng.integers(0, 100))
            rows.append((s, u, a, a + int(rng.integers(5, 128 - a + 1))))
    return np.array(sorted(set(rows)), dtype=np.int64), np.full(nuniv, 128, dtype=np.int64), 301


@functools.lru_cache(maxsize=None)
def usel_table(nwords):
    """Universe 0 of nwords bitmap words (64 nwords bases) and universe 1 of 500 bases; nwords sets of one 40-base
    row, each inside another word of universe 0 (the first ten also in universe 1); 40 wide sets of 1,000 bases of
    universe 0 -- four rows of 250, the row-parallel solver takes rows of at most 257 -- each over the small rows of
    16 words.  Every word of universe 0 has uncovered bits in round 0; a word dies when a wide set is picked."""
    rows = []
    for s in range(nwords):
        rows.append((s, 0, 64 * s + 12, 64 * s + 52))
        if s < 10:
            rows.append((s, 1, 40 * s, 40 * s + 60))
    for t in range(40):
        for j in range(4):
            a = 64 * (76 * t) + 256 * j
            rows.append((nwords + t, 0, a, a + 250))
    return np.array(sorted(rows), dtype=np.int64), np.array([64 * nwords, 500], dtype=np.int64), nwords + 40


def _live_words(r, picked, nwords):
    """Words of universe 0 that hold a coverable base no picked set covers."""
    cover = np.zeros(64 * nwords, dtype=bool)
    done = np.zeros(64 * nwords, dtype=bool)
    for s, u, a, b in r.tolist():
        if u == 0:
            cover[a:b] = True
            if s in picked:
                done[a:b] = True
    return int((cover & ~done).reshape(nwords, 64).any(axis=1).sum())


def test_solver_tables_cross_their_kernel_limits():
    """Segments of the winner against GW_MAXWSEG; words with uncovered bits in round 0 against GR_USEL_CAP, and below
    it once the wide sets are picked (which the oracle picks first, long before the need is met)."""
    o = _oracle()
    for nuniv, beyond in ((4096, 0), (4097, 1), (4200, 104)):
        r, glen, nsets = wseg_table(nuniv)
        seg0 = len({u for s, u, _, _ in r.tolist() if s == 0})
        assert seg0 == nuniv and max(0, seg0 - GW_MAXWSEG) == beyond
        others_beyond = {s for s, u, _, _ in r.tolist() if s != 0 and u >= GW_MAXWSEG}
        assert (len(others_beyond) >= 2) == (beyond > 0)
        assert np.bincount(r[:, 0], minlength=nsets).min() >= 1
    for nwords in (3072, 3073, 3200):
        r, glen, nsets = usel_table(nwords)
        assert int((r[:, 3] - r[:, 2]).max()) <= 257
        assert _live_words(r, set(), nwords) == nwords
        picks = o.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], nsets, 2, None, [0.5, 0.5], None)
        assert sorted(picks[:40]) == list(range(nwords, nwords + 40)) and len(picks) > 400
        assert _live_words(r, set(picks[:40]), nwords) == nwords - 640 < GR_USEL_CAP
    assert not 3072 > GR_USEL_CAP and 3073 > GR_USEL_CAP and 3200 > GR_USEL_CAP


@pytest.mark.gpu
@pytest.mark.parametrize("nuniv", [4096, 4097, 4200])
def test_winner_segments_at_and_beyond_the_lds_counters(ctx, nuniv):
    """greedy_wg_kernel's apply step keeps the bits a winner clears per segment in GW_MAXWSEG LDS counters and
    updates `usize` of the segments beyond them with global atomics; `left` and `can` of those universes then decide
    when they stop counting under partial cover.  A winner of exactly 4,096 segments, of 4,097 and of 4,200, at full
    coverage and at 0.6 and 0.9, pick for pick the oracle's -- in every solver form, and with the check that the
    forms meant to reach that kernel did."""
    o = _oracle()
    r, glen, nsets = wseg_table(nuniv)
    with _nothing_else_changed():
        for cov in (None, 0.6, 0.9):
            up = None if cov is None else [cov] * nuniv
            exp = o.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], nsets, nuniv, None, up, None)
            assert exp[0] == 0 and (len(exp) > 50 or cov == 0.6)
            for form, (hooks, wg_full, wg_partial) in SOLVER_FORMS.items():
                got, cn = _solve(ctx, r, glen, nsets, up, hooks)
                assert got == exp, (form, cov)
                assert _ran_one_workgroup_solver(cn, r, got) == (wg_full if cov is None else wg_partial), (form, cov, cn)


@pytest.mark.gpu
@pytest.mark.parametrize("nwords", [3072, 3073, 3200])
def test_universe_select_at_and_beyond_its_word_list(ctx, nwords):
    """gr_usel_kernel (the row-parallel solver's rounds under partial cover) lists up to GR_USEL_CAP words with
    uncovered bits in LDS; with more, the later passes of its radix select read the bitmap and the owner words
    again.  Round 0 of these solves has exactly 3,072 / 3,073 / 3,200 such words, the rounds after the wide sets'
    picks 640 fewer, so the 3,073- and 3,200-word solves run both branches.  The kernel keeps no counter of its
    branches: that it ran is the row-parallel solver's counters, which branch is the host's count of the words
    (test_solver_tables_cross_their_kernel_limits).  The other solver forms must agree."""
    o = _oracle()
    r, glen, nsets = usel_table(nwords)
    up = [0.5, 0.5]
    exp = o.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], nsets, 2, None, up, None)
    with _nothing_else_changed():
        for form, (hooks, _, wg_partial) in SOLVER_FORMS.items():
            got, cn = _solve(ctx, r, glen, nsets, up, hooks)
            assert got == exp, form
            assert _ran_one_workgroup_solver(cn, r, got) == wg_partial, (form, cn)
            if not wg_partial:
                assert cn["flat_rows_streamed"] > 0 and cn["greedy_iters"] > 1, (form, cn)
