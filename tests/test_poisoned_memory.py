"""Every entry point on poisoned device memory.

Every scratch buffer of the library comes from the caching pool of csrc/core.hip.  A block the driver has just supplied
reads as zeros in practice and a block taken from the cache holds what the previous call left -- in a test that repeats
a call, usually the very values the kernel would have written.  A kernel that ORs into a bitmap nobody cleared, reads a
flag one element past what its producer wrote, or masks the slack words behind a bitmap wrongly therefore passes every
other test of the suite.  The test hook CATCHHIP_POOL_POISON=<byte> (honoured under CATCHHIP_TEST_HOOKS=1) fills the
whole size class of every block the pool hands out, and of the index's own hipMalloc blocks, with that byte.

Every case below is one small call into one entry family.  It runs three times, each in a context of its own that is
closed afterwards: hook unset, 255 (zero is no longer the identity; every stale bitmap looks full) and 85 (all ones is
no longer the identity of min; every stale bitmap looks half full).  Every defined output of the two poisoned runs must
equal the plain run's byte for byte, and the plain run must equal the family's own model, imported from the family's
test module or from the oracle.  Outputs the library documents as undefined (the order of a seed table's entries under
one key, lanes a wave helper promises nothing for) are compared in their defined form only.

Shapes: a coordinate space of 4,837 bases (75 bitmap words and 37 bases: the last word is partial, the `+ 2` words
behind it pure slack) in three universes whose borders lie inside words; 257 sets and 1,025 rows (one above a multiple
of the wavefront and of the workgroup: the last wave is partial and the size class has a tail), a row of 257 bases
(five words) and, where the entry takes it, one of 258 (six), and a row that ends at the last base.

The last test needs no GPU: every entry catchhip.h declares is named by a case or listed with its reason in EXEMPT."""
import contextlib
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "catchhip.h")
HOOK = "CATCHHIP_POOL_POISON"
POISONS = (None, 255, 85)

GLEN = (1500, 2000, 1337)          # 4,837 bases = 75 * 64 + 37; the universes end at bits 28 and 44 of their words
NSETS, NROWS = 257, 1025


# ------------------------------------------------------------------ the table of cases
class Case:
    def __init__(self, name, entries, hooks, fn):
        self.name, self.entries, self.hooks, self.fn = name, tuple(entries), dict(hooks), fn


CASES = []


def case(name, entries, **hooks):
    """fn(c, oracle) -> (outputs of the device calls on context c, the model's outputs or None per key).  The model
    half is evaluated for the plain run only; a key the model leaves out is compared between the runs alone."""
    def deco(fn):
        CASES.append(Case(name, entries, hooks, fn))
        return fn
    return deco


@contextlib.contextmanager
def closing(*objs):
    try:
        yield objs if len(objs) != 1 else objs[0]
    finally:
        for o in reversed(objs):
            o.close()


def _canon(x):
    """An output as bytes and plain Python values: equal canons = equal byte for byte."""
    if isinstance(x, np.ndarray):
        return ("array", str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return {k: _canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x).hex()
    if isinstance(x, float):
        return x.hex()
    return x


def _values(x):
    """An output as values, whatever the integer type: what the models are compared by."""
    if isinstance(x, np.ndarray):
        return _values(x.tolist())
    if isinstance(x, dict):
        return {k: _values(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_values(v) for v in x]
    if isinstance(x, (np.integer, np.bool_, bool)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    return x


def _differing(a, b):
    ca, cb = _canon(a), _canon(b)
    return sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))


# ------------------------------------------------------------------ shared inputs: built once, never changed
_cache = {}


def cached(fn):
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]
    wrapper.__name__ = fn.__name__
    return wrapper


def _free(rows_of, u, a, b):
    """[a, b) neither overlaps nor touches a row the (set, universe) holds already."""
    return all(b < s or a > e for s, e in rows_of.get(u, ()))


@cached
def table(long_rows, seed):
    """(set, universe, start, end) arrays of NROWS rows in NSETS sets over GLEN, sorted by (set, universe, start), the
    rows of a (set, universe) disjoint and non-touching.  Set 0 holds a row of 257 bases from bit 63 of a word (five
    words), set 1 a row that ends at the last base of the space, and with long_rows set 2 one of 258 bases from bit
    63 (six words)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate(([0], np.cumsum(GLEN)))
    by_set = [dict() for _ in range(NSETS)]
    by_set[0][0] = [(63, 320)]
    by_set[1][2] = [(GLEN[2] - 100, GLEN[2])]
    if long_rows:
        x = int(-(off[1] + 1) % 64)                      # off[1] + x = 63 (mod 64)
        by_set[2][1] = [(x, x + 258)]
    n = sum(len(v) for d in by_set for v in d.values())
    s = 0
    while n < NROWS:
        u = int(rng.integers(0, len(GLEN)))
        ln = int(rng.integers(1, 257))
        a = int(rng.integers(0, GLEN[u] - ln + 1))
        if _free(by_set[s], u, a, a + ln):
            by_set[s].setdefault(u, []).append((a, a + ln))
            n += 1
        s = (s + 1) % NSETS
    rows = sorted((i, u, a, b) for i, d in enumerate(by_set) for u, v in d.items() for a, b in v)
    arr = np.array(rows, dtype=np.int64)
    assert arr.shape == (NROWS, 4) and int(off[-1]) % 64 == 37 and int(off[1]) % 64 and int(off[2]) % 64
    assert (arr[:, 3] - arr[:, 2]).max() == (258 if long_rows else 257) and (off[arr[:, 1]] + arr[:, 3]).max() == off[-1]
    return arr[:, 0].astype(np.int32), arr[:, 1].astype(np.int32), arr[:, 2].copy(), arr[:, 3].copy()


def from_host(c, tab, glen=GLEN):
    from catch_amd import engine
    return engine.Rows.from_host(c, tab[0], tab[1], tab[2], tab[3], glen)


def fetched(rows):
    si, un, st, en = rows.fetch()
    return {"set": si, "universe": un, "start": st, "end": en}


def as_table(d):
    return d["set"], d["universe"], d["start"], d["end"]


def table_dict(tab):
    return {"set": np.asarray(tab[0]), "universe": np.asarray(tab[1]), "start": np.asarray(tab[2]), "end": np.asarray(tab[3])}


@cached
def picks65():
    """65 distinct sets in no order: a pick list (one above a wavefront)."""
    return [int(x) for x in np.random.default_rng(65).permutation(NSETS)[:65]]


# ------------------------------------------------------------------ row tables
@case("rows_from_host", ["catchhip_rows_from_host", "catchhip_rows_fetch", "catchhip_rows_fetch_gain0",
                         "catchhip_rows_longest", "catchhip_rows_destroy"])
def _rows_from_host(c, oracle):
    tab = table(True, 1)
    with closing(from_host(c, tab)) as r:
        got = dict(fetched(r), gain0=r.fetch_gain0(NSETS), longest=r.longest())
    gain0 = np.bincount(tab[0], weights=tab[3] - tab[2], minlength=NSETS).astype(np.int64)
    return got, dict(table_dict(tab), gain0=gain0, longest=258)


@case("rows_subtract", ["catchhip_rows_subtract"])
def _rows_subtract(c, oracle):
    from test_extend_probes import _np_subtract
    tab, cov = table(True, 1), table(False, 2)
    cov = tuple(a[:65] for a in cov)                     # the rows of the first sets: they overlap one another
    with closing(from_host(c, tab), from_host(c, cov)) as (r, k):
        with closing(r.subtract(k)) as d:
            got = dict(fetched(d), gain0=d.fetch_gain0(NSETS), longest=d.longest())
    want = _np_subtract(tab, cov, GLEN)
    return got, dict(table_dict(want), longest=int((want[3] - want[2]).max()),
                     gain0=np.bincount(want[0], weights=want[3] - want[2], minlength=NSETS).astype(np.int64))


@case("rows_union", ["catchhip_rows_union"])
def _rows_union(c, oracle):
    from test_rows_union import _model_union
    a, b = table(True, 1), table(False, 2)
    with closing(from_host(c, a), from_host(c, b)) as (ra, rb):
        with closing(ra.union(rb)) as u:
            got = dict(fetched(u), gain0=u.fetch_gain0(NSETS), longest=u.longest())
    rows, gain0, longest = _model_union(a, b)
    w = np.array(rows, dtype=np.int64)
    return got, dict(table_dict((w[:, 0], w[:, 1], w[:, 2], w[:, 3])), gain0=gain0, longest=longest)


@case("rows_below_depth", ["catchhip_rows_below_depth"])
def _rows_below_depth(c, oracle):
    from test_coverage_depth import _np_below_depth
    tab = table(True, 1)
    with closing(from_host(c, tab)) as r:
        d, reached = r.below_depth(NSETS, picks65(), 6)
        with closing(d):
            got = dict(fetched(d), reached=reached, gain0=d.fetch_gain0(NSETS), longest=d.longest())
    want, want_reached, _depth = _np_below_depth(tab, NSETS, picks65(), 6, GLEN)
    assert want_reached.sum() > 0 and want[0].size > NROWS // 2
    return got, dict(table_dict(want), reached=want_reached)


@case("rows_prune", ["catchhip_rows_prune"])
def _rows_prune(c, oracle):
    from test_prune_redundant import _walk
    tab, fixed = table(True, 1), tuple(a[:65] for a in table(False, 2))
    picks = [int(x) for x in np.random.default_rng(7).permutation(NSETS)]
    with closing(from_host(c, tab), from_host(c, fixed)) as (r, f):
        kept, removed = r.prune(NSETS, picks, 1, f)
        got = dict(kept=kept, removed=removed)
    want = _walk(tab, GLEN, picks, 1, fixed)
    assert want[1], "the walk removes something"
    return got, dict(kept=want[0], removed=want[1])


@case("rows_pick_gains", ["catchhip_rows_pick_gains"])
def _rows_pick_gains(c, oracle):
    from test_max_probes import _model
    tab = table(True, 1)
    ck, denom, covered0 = [1, 2, 33, 64, 65], [1500, 0, 1337], [3, 0, 7]
    with closing(from_host(c, tab)) as r:
        gains, tot, wu, wc = r.pick_gains(NSETS, picks65(), ck, denom, covered0)
        plain, _t, _u, _c = r.pick_gains(NSETS, picks65())
    want_gains, curve = _model(tab, GLEN, picks65(), ck, denom, covered0)
    return (dict(gains=gains, total=tot, worst=wu, worst_covered=wc, gains_alone=plain),
            dict(gains=want_gains, total=[x[0] for x in curve], worst=[x[1] for x in curve],
                 worst_covered=[x[2] for x in curve], gains_alone=want_gains))


@cached
def wanted_intervals():
    """Wanted intervals in normal form: one that ends at the last base, one across a universe's last word."""
    return [(0, 10, 700), (0, 705, 1500), (1, 0, 64), (1, 100, 1999), (2, 3, 4), (2, 900, 1337)]


@cached
def sequences():
    rng = np.random.default_rng(11)
    return ["".join(rng.choice(list("ACGTN"), p=[0.22, 0.22, 0.22, 0.22, 0.12], size=n)) for n in GLEN]


@case("basemask and the cuts by it", ["catchhip_basemask_create", "catchhip_basemask_fetch", "catchhip_basemask_destroy",
                                      "catchhip_rows_restrict", "catchhip_rows_uncovered", "catchhip_rows_uncovered_within",
                                      "catchhip_targets_create", "catchhip_targets_destroy"])
def _basemask(c, oracle):
    from test_target_regions import _host_within, _mask, _np_cut, _np_words, _wanted_bits
    from test_uncovered_regions import HostTargets, model_uncovered
    tab, iv, seqs = table(True, 1), wanted_intervals(), sequences()
    cover = tuple(a[::3] for a in tab)                   # a third of the rows: regions stay uncovered
    with closing(from_host(c, tab), from_host(c, cover), _mask(c, GLEN, iv), HostTargets(c, seqs)) as (r, k, m, t):
        words, wanted = m.fetch(), m.wanted
        with closing(r.restrict(m)) as d:
            cut = dict(fetched(d), gain0=d.fetch_gain0(NSETS), longest=d.longest())
        unc = k.uncovered(t, 2, 5, 3)
        base = k.uncovered(t, 2, 1, 0)
        within = k.uncovered(t, 2, 5, 3, mask=m)
        bare = k.uncovered(None, 1, 1, 1)
    got = dict(words=words, wanted=wanted, cut=cut, uncovered=list(unc), base=list(base), within=list(within), bare=list(bare))
    bits = _wanted_bits(GLEN, iv)
    off = np.concatenate(([0], np.cumsum(GLEN)))
    want_cut = _np_cut(tab, bits, GLEN)
    w_within, w_per = _host_within(base, iv, seqs, 5, 3)
    want = dict(words=_np_words(bits), wanted=[int(bits[off[u]:off[u + 1]].sum()) for u in range(len(GLEN))],
                cut=dict(table_dict(want_cut), longest=int((want_cut[3] - want_cut[2]).max())),
                uncovered=list(model_uncovered(GLEN, cover[1], cover[2], cover[3], seqs, 2, 5, 3)),
                base=list(model_uncovered(GLEN, cover[1], cover[2], cover[3], seqs, 2, 1, 0)),
                bare=list(model_uncovered(GLEN, cover[1], cover[2], cover[3], None, 1, 1, 1)))
    assert list(zip(within[0].tolist(), within[1].tolist(), within[2].tolist(), within[3].tolist())) == w_within
    assert np.array_equal(within[4], w_per) and len(w_within) > 3
    return got, want


@case("rows_stats, window_depth", ["catchhip_rows_stats", "catchhip_rows_window_depth"])
def _rows_stats(c, oracle):
    from test_analyze_probe_coverage import _expect_windows
    from test_extend_probes import _union_len
    tab = table(True, 1)
    spans = np.asarray([0, 1, 1, 3])
    with closing(from_host(c, tab)) as r:
        tl, ul, ps = r.stats(len(GLEN), NSETS)
        sums, counts, win_off = r.window_depth(spans, 50, 25)
        one, cnt1, off1 = r.window_depth([0, 3], 6000, 1000)      # a window longer than the space
    got = dict(total_len=tl, union_len=ul, per_set=ps, sums=sums, counts=counts, win_off=win_off,
               one=one, one_counts=cnt1, one_off=off1)
    w = _expect_windows(tab[1], tab[2], tab[3], np.asarray(GLEN), spans, 50, 25)
    w1 = _expect_windows(tab[1], tab[2], tab[3], np.asarray(GLEN), np.asarray([0, 3]), 6000, 1000)
    per_set = np.zeros(NSETS, dtype=np.int64)
    for s, u in set(zip(tab[0].tolist(), tab[1].tolist())):
        per_set[s] += 1
    want = dict(total_len=np.bincount(tab[1], weights=tab[3] - tab[2], minlength=len(GLEN)).astype(np.int64),
                union_len=_union_len(tab, len(GLEN)), per_set=per_set, sums=w[0], counts=w[1], win_off=w[2],
                one=w1[0], one_counts=w1[1], one_off=w1[2])
    return got, want


@case("rows_cover_check", ["catchhip_rows_cover_check"])
def _rows_cover_check(c, oracle):
    from test_gpu_parity import _np_cover_check
    tab = table(False, 1)
    p = [1.0, 0.9, 0.5]
    picks = oracle.approx_multiuniverse(tab[0], tab[1], tab[2], tab[3], NSETS, len(GLEN), None, p, None)
    lists = {"solved": list(picks), "first pick dropped": list(picks)[1:], "a pick again and one out of range": list(picks) + [picks[0], NSETS + 3]}
    with closing(from_host(c, tab)) as r:
        got = {k: r.cover_check(NSETS, v, p) for k, v in lists.items()}
    want = {}
    for k in ("solved", "first pick dropped"):           # (the replay knows no bad ids: that list is compared between the runs)
        nogain, short, ubases, cbases = _np_cover_check(tab[0], tab[1], tab[2], tab[3], np.asarray(GLEN), lists[k], p)
        want[k] = dict(picks_without_gain=nogain, universes_short=short, bad_pick_ids=0, universe_bases=ubases, covered_bases=cbases)
    assert want["solved"]["universes_short"] == 0 and want["first pick dropped"]["universes_short"] >= 1
    assert got["a pick again and one out of range"]["bad_pick_ids"] == 2
    return got, want


# ------------------------------------------------------------------ the solvers
@cached
def ranks257():
    return np.random.default_rng(257).integers(0, 3, size=NSETS)


def _greedy_case(c, oracle, long_rows, p, sequential_model=False):
    """rows.greedy without and with ranks on context c -> (picks in pick order and the exact counters, the oracle's)."""
    tab = table(long_rows, 1)
    got, want = {}, {}
    with closing(from_host(c, tab)) as r:
        for name, ranks in (("no ranks", None), ("ranks", ranks257())):
            got[name] = r.greedy(NSETS, ranks, p)
            cn = c.counters()
            got[name + ": picks counted"] = cn["picks"]
            key = ("greedy", long_rows, None if p is None else tuple(p), name)
            if key not in _cache:
                if long_rows or sequential_model:
                    _cache[key] = list(oracle.lazy_greedy(tab[0], tab[1], tab[2], tab[3], NSETS, np.asarray(GLEN), p, ranks))
                else:
                    _cache[key] = list(oracle.approx_multiuniverse(tab[0], tab[1], tab[2], tab[3], NSETS, len(GLEN), None, p, ranks))
            want[name] = _cache[key]
            want[name + ": picks counted"] = len(_cache[key])
            assert len(_cache[key]) > 5
    return got, want


SOLVER_ENTRIES = ["catchhip_setcover_greedy", "catchhip_ctx_last_counters", "catchhip_ctx_last_solver_counters",
                  "catchhip_ctx_last_solver_levels", "catchhip_ctx_last_solver_band_groups", "catchhip_ctx_last_seeds_dropped",
                  "catchhip_ctx_last_rows_direct", "catchhip_ctx_last_join_counters"]
PARTIAL_P = [1.0, 0.9, 0.5]


@case("greedy: fused frontier rounds", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS=str(1 << 40))
def _greedy_fused(c, oracle):
    got, want = _greedy_case(c, oracle, False, None)
    assert c.counters()["flat_rows_streamed"] == 0
    return got, want


@case("greedy: row-parallel, striped tiles", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS="0")
def _greedy_flat_striped(c, oracle):
    got, want = _greedy_case(c, oracle, False, None)
    assert c.counters()["flat_rows_streamed"] > 0
    return got, want


@case("greedy: row-parallel, contiguous tiles, changed-word statistics", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS="0",
      CATCHHIP_FLAT_TILE_SHIFT="16", CATCHHIP_FLAT_COUNT_DIRTY="1")
def _greedy_flat_contiguous(c, oracle):
    got, want = _greedy_case(c, oracle, False, None)
    assert c.counters()["flat_rows_streamed"] > 0
    return got, want


@case("greedy: rows longer than 257 bases", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS="0")
def _greedy_long_rows(c, oracle):
    got, want = _greedy_case(c, oracle, True, None)
    assert c.counters()["flat_rows_streamed"] == 0       # (the lane-per-word kernels of the fused family)
    return got, want


@case("greedy: short rows through the lane-per-word kernels", SOLVER_ENTRIES, CATCHHIP_GF_LONG="1",
      CATCHHIP_FLAT_MIN_ROWS=str(1 << 40))
def _greedy_forced_long(c, oracle):
    return _greedy_case(c, oracle, False, None)


@case("greedy: partial coverage, row-parallel", SOLVER_ENTRIES)
def _greedy_partial_flat(c, oracle):
    got, want = _greedy_case(c, oracle, False, PARTIAL_P)
    assert c.counters()["flat_rows_streamed"] > 0
    return got, want


@case("greedy: partial coverage, row-parallel, contiguous tiles", SOLVER_ENTRIES, CATCHHIP_FLAT_TILE_SHIFT="16",
      CATCHHIP_FLAT_COUNT_DIRTY="1")
def _greedy_partial_flat_contiguous(c, oracle):
    return _greedy_case(c, oracle, False, PARTIAL_P)


@case("greedy: partial coverage, persistent workgroup", SOLVER_ENTRIES, CATCHHIP_PARTIAL_SEQUENTIAL="1")
def _greedy_partial_sequential(c, oracle):
    got, want = _greedy_case(c, oracle, False, PARTIAL_P)
    assert c.counters()["flat_rows_streamed"] == 0 and c.counters()["rows_recounted"] > 0
    return got, want


@case("greedy: partial coverage, long rows, persistent workgroup", SOLVER_ENTRIES)
def _greedy_partial_long(c, oracle):
    return _greedy_case(c, oracle, True, PARTIAL_P)


@case("greedy: one pick per iteration", SOLVER_ENTRIES, CATCHHIP_GREEDY_SEQUENTIAL="1")
def _greedy_sequential(c, oracle):
    got, want = _greedy_case(c, oracle, False, None)
    assert c.counters()["rows_recounted"] > 0
    return got, want


def _banded(c, oracle, bands):
    got, want = _greedy_case(c, oracle, False, None)
    cn = c.counters()                                    # (of the solve with ranks: one band, whatever is asked for)
    assert cn["flat_rows_streamed"] > 0 and cn["flat_bands"] == 1
    tab = table(False, 1)
    with closing(from_host(c, tab)) as r:
        again = r.greedy(NSETS, None, None)
        cn = c.counters()
    assert again == got["no ranks"]
    got["bands"], got["levels"] = cn["flat_bands"], cn["flat_levels"]
    want["bands"] = want["levels"] = bands
    return got, want


@case("greedy: gain bands, striped tiles", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS="0", CATCHHIP_FLAT_BANDS="4",
      CATCHHIP_FLAT_BAND_RATIO="500")
def _greedy_bands_striped(c, oracle):
    return _banded(c, oracle, 4)


@case("greedy: gain bands, contiguous tiles", SOLVER_ENTRIES, CATCHHIP_FLAT_MIN_ROWS="0", CATCHHIP_FLAT_BANDS="64",
      CATCHHIP_FLAT_BAND_RATIO="500", CATCHHIP_FLAT_TILE_SHIFT="11")
def _greedy_bands_contiguous(c, oracle):
    # 4,837 bases in tiles of 2,048: 3 coordinate tiles, one per XCD, of up to 32 sub-tiles
    return _banded(c, oracle, 32)


SHARD_ENTRIES = ["catchhip_shard_create", "catchhip_shard_create_p", "catchhip_shard_create_pi", "catchhip_shard_destroy",
                 "catchhip_shard_count", "catchhip_shard_claim_check", "catchhip_shard_verdict", "catchhip_shard_apply",
                 "catchhip_shard_picks", "catchhip_shard_info", "catchhip_shard_buffers", "catchhip_shard_buffer_copy",
                 "catchhip_shard_allreduce_local", "catchhip_shard_solve"]


@case("shards: one rank, and two shards of one process", SHARD_ENTRIES)
def _shards(c, oracle):
    from catch_amd import engine
    tab = table(False, 1)
    got, want = {}, {}
    for name, p in (("full", None), ("partial", PARTIAL_P)):
        for ranks_name, ranks in (("no ranks", None), ("ranks", ranks257())):
            key = ("greedy", False, None if p is None else tuple(p), ranks_name)
            if key not in _cache:
                _cache[key] = list(oracle.approx_multiuniverse(tab[0], tab[1], tab[2], tab[3], NSETS, len(GLEN), None, p, ranks))
            with closing(from_host(c, tab)) as r:
                with closing(engine.Shard(r, NSETS, ranks, p)) as sh:
                    got[name, ranks_name, "solve"] = engine.shards_solve([sh], "local", 4)
                # ... and round by round, the exchange buffers through the host (a transport of the caller's own)
                with closing(engine.Shard(r, NSETS, ranks, p)) as sh:
                    done = 0
                    while not done:
                        sh.count()
                        sh.buffer_from_host(0, sh.buffer_to_host(0))
                        sh.claim_check()
                        sh.buffer_from_host(1, sh.buffer_to_host(1))
                        if sh.partial:
                            sh.verdict()
                            sh.buffer_from_host(1, sh.buffer_to_host(1))
                        done = sh.apply()
                    got[name, ranks_name, "steps"] = sh.picks()
            want[name, ranks_name, "solve"] = want[name, ranks_name, "steps"] = _cache[key]
        # two shards of one process: universes 0-1 and universe 2, exchanged on the device
        lo = tab[1] < 2
        a = tuple(x[lo] for x in tab)
        b = (tab[0][~lo], tab[1][~lo] - 2, tab[2][~lo], tab[3][~lo])
        with closing(from_host(c, a, GLEN[:2]), from_host(c, b, GLEN[2:])) as (ra, rb):
            pa, pb = (None, None) if p is None else (p[:2], p[2:])
            with closing(engine.Shard(ra, NSETS, None, pa, p is not None), engine.Shard(rb, NSETS, None, pb, p is not None)) as shards:
                got[name, "two shards"] = engine.shards_solve(list(shards), "local", 2)
        want[name, "two shards"] = _cache[("greedy", False, None if p is None else tuple(p), "no ranks")]
    return ({" / ".join(k): v for k, v in got.items()}, {" / ".join(k): v for k, v in want.items()})


# ------------------------------------------------------------------ the primitives' own entry points
@case("selftest_scan_u32", ["catchhip_selftest_scan_u32"])
def _selftest_scan(c, oracle):
    from test_primitives import _scan_input, expected_scan
    got, want = {}, {}
    for n in (1, 2049, 2048 * 3 + 1):                    # one tile, two levels of the recursion
        x = _scan_input("random", n)
        for in_place in (False, True):
            got[n, in_place] = c.selftest_scan_u32(x, in_place=in_place)
            want[n, in_place] = expected_scan(x)
    return ({str(k): v for k, v in got.items()}, {str(k): v for k, v in want.items()})


@case("selftest_sort_pairs", ["catchhip_selftest_sort_pairs"])
def _selftest_sort(c, oracle):
    from test_primitives import expected_perm, make_keys, sorted_bits
    rng = np.random.default_rng(4097)
    got, want = {}, {}
    for key_bits, first_bit in ((64, 0), (13, 32)):      # eight passes and two: the result in either buffer
        keys = make_keys(rng, 4097, key_bits, first_bit, "random")
        k, v = c.selftest_sort_pairs(keys, np.arange(4097, dtype=np.uint32), key_bits, first_bit)
        perm = expected_perm(keys, key_bits, first_bit)
        got[key_bits, first_bit] = [k, v]
        want[key_bits, first_bit] = [keys[perm], perm]
    keys = make_keys(rng, 3 * 4097, 32, 0, "two_values")
    k, v = c.selftest_sort_pairs(keys, np.arange(keys.size, dtype=np.uint32), 32, 0, nseg=3)
    perm = np.argsort(sorted_bits(keys.reshape(3, -1), 32, 0), axis=1, kind="stable")
    got["segments"] = [k, v]
    want["segments"] = [np.take_along_axis(keys.reshape(3, -1), perm, axis=1).reshape(-1), (perm + np.arange(3)[:, None] * 4097).reshape(-1)]
    return ({str(k): v for k, v in got.items()}, {str(k): v for k, v in want.items()})


@case("selftest_wave, find_segment", ["catchhip_selftest_wave", "catchhip_selftest_find_segment"])
def _selftest_wave(c, oracle):
    from test_primitives import LANE0_FORMS, _segment_tables, _wave_expected, _wave_input
    x = _wave_input("random", 256)
    out = c.selftest_wave(x)
    got = {k: (v[::64] if k in LANE0_FORMS else v) for k, v in out.items()}     # (the other lanes are promised nothing)
    want = dict(_wave_expected(x))
    off = _segment_tables()["n300"]
    xs = np.arange(int(off[-1]), dtype=np.uint32)
    got["segments"] = c.selftest_find_segment(off, xs)
    want["segments"] = np.searchsorted(off[1:], xs, side="right")
    return got, want


@case("selftest_spans", ["catchhip_selftest_spans"])
def _selftest_spans(c, oracle):
    from test_primitives import SPAN_INTERVALS, _span_bitmap, _span_expected, _words
    bits = _span_bitmap("random")
    a, b = np.array(SPAN_INTERVALS, dtype=np.uint32).T
    got = dict(c.selftest_spans(_words(bits), a, b, 5))
    want = dict(_span_expected(bits, 5))
    return got, want


@case("selftest_row_build", ["catchhip_selftest_row_build"])
def _selftest_row_build(c, oracle):
    from test_row_build import BOUNDS, reference, size_table
    sizes = (0, 1, 65, 129, 513, 1025)                   # the wavefront's buckets, and the workgroup's
    hits, nb = size_table("gaps", "random", sizes)
    keys = ("set", "seg", "start", "end", "mcnt", "blmax", "bsum", "hits", "rows", "lmax")
    ref = reference(hits, nb)
    got, want = {}, {}
    wave = [min(64, hits.shape[0] - 64 * i) for i in range(-(-hits.shape[0] // 64))]
    for form, kw in (("scattered", {}), ("compact", {"wave_hits": wave}), ("grouped", {})):
        for emit in ("host", "device"):
            out = c.selftest_row_build(hits, nb, form=form, emit=emit, **kw)
            got[form + " " + emit] = {k: out[k] for k in keys}
            want[form + " " + emit] = {k: ref[k] for k in keys}
    out = c.selftest_row_build(hits, nb, bounds=BOUNDS, build="radix")
    got["radix"] = {k: out[k] for k in ("set", "seg", "start", "end", "rows")}
    want["radix"] = {k: ref[k] for k in ("set", "seg", "start", "end", "rows")}
    return got, want


@case("selftest_seed_table", ["catchhip_selftest_seed_table", "catchhip_probes_create", "catchhip_probes_destroy"])
def _selftest_seed_table(c, oracle):
    from test_seed_table import _rs, check_table, make_probes, pigeonhole_entries
    rng = random.Random(1065)
    k0 = _rs(rng, 25)
    probes = [(k0 if i % 5 == 0 else _rs(rng, 25)) + _rs(rng, 75) for i in range(65)]     # one key of 13 entries
    k, nanch, ntab, low, high = pigeonhole_entries(probes, 100, 2)
    got = {}
    P, nent = make_probes(c, probes, 100, k)
    with closing(P):
        for name, kw in (("join", {}), ("list", {"as_list": True}), ("list, unfiltered", {"as_list": True, "allow_filter": False})):
            d = c.selftest_seed_table(P, nent, 2, **kw)
            slot_of = check_table(d, low, slot_only=set(high.values()) - set(low.values()) if d["filtered"] else ())
            # the defined content: which entries stand under which key (their order under a key, and the slot a key
            # lands in when two claim one, are the order of the atomics)
            ents = {"%x" % key: sorted(int(e) for e in d["ents"][d["slots"][s, 2]:d["slots"][s, 2] + d["slots"][s, 3]])
                    for key, s in slot_of.items()}
            got[name] = dict(capacity=d["capacity"], keys=d["keys"], entries=d["entries"], filtered=d["filtered"],
                             anchors=d["anchors_per_probe"], ents=ents)
            if d["filtered"]:
                got[name]["aslot keys"] = ["%x" % ((int(d["slots"][s & 0x7fffffff, 1]) << 32) | int(d["slots"][s & 0x7fffffff, 0]))
                                           for s in d["aslot"].tolist()]
    want = {name: dict(capacity=1024, keys=len(set(low.values())), entries=len(low)) for name in got}
    return got, want


# ------------------------------------------------------------------ scans
@cached
def scan_input():
    """Five genomes of one species and their candidate probes; the bases add up to 37 (mod 64)."""
    from util import candidates, small_species
    genomes = [list(g) for g in small_species(seed=77, n=5, length=1500, d1=0.04, d2=0.01)]
    total = sum(len(s) for g in genomes for s in g)
    cut = (total - 37) % 64
    genomes[-1][-1] = genomes[-1][-1][:len(genomes[-1][-1]) - cut]
    assert sum(len(s) for g in genomes for s in g) % 64 == 37
    return genomes, candidates(genomes, 100, 50)


def _scan_case(c, oracle, m, thres, island, ext, mode, seed=None, merge=True):
    from test_gpu_parity import _oracle_rows, _scan_rows
    genomes, probes = scan_input()
    if seed is not None:
        np.random.seed(seed)
    got = _scan_rows(c, probes, genomes, m, thres, island, ext, mode, merge=merge)
    key = ("scan", m, thres, island, ext, seed, merge)
    if merge and key not in _cache:
        if seed is not None:
            np.random.seed(seed)
        _cache[key] = _oracle_rows(oracle, probes, genomes, m, thres, island, ext)
    return got, _cache.get(key)


SCAN_ENTRIES = ["catchhip_cover_scan", "catchhip_targets_create_ptrs", "catchhip_ctx_create", "catchhip_ctx_destroy"]


@case("cover_scan: tiled", SCAN_ENTRIES)
def _scan_fast(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 2, 100, 0, 50, engine.SCAN_FAST)
    return dict(rows=got), dict(rows=want)


@case("cover_scan: hash-seeded, key-grouped join", SCAN_ENTRIES)
def _scan_seed_join(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 2, 100, 0, 50, engine.SCAN_SEED)
    cn = c.counters()
    assert cn["join_hit_positions"] > 0
    return dict(rows=got, hits=cn["raw_hits"], hit_positions=cn["join_hit_positions"], pairs=cn["join_pairs"]), dict(rows=want)


@case("cover_scan: hash-seeded, seed list", SCAN_ENTRIES, CATCHHIP_SEED_LIST="1")
def _scan_seed_list(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 2, 100, 0, 50, engine.SCAN_SEED)
    cn = c.counters()
    assert cn["join_hit_positions"] == 0 and cn["seeds_dropped"] > 0
    return dict(rows=got, hits=cn["raw_hits"], seeds=cn["seed_hits"] - cn["seeds_dropped"]), dict(rows=want)


@case("cover_scan: hash-seeded, seed list without the anchor-pair filter", SCAN_ENTRIES, CATCHHIP_SEED_LIST="1",
      CATCHHIP_SEED_KEEP_ALL="1")
def _scan_seed_list_keep_all(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 2, 100, 0, 50, engine.SCAN_SEED)
    return dict(rows=got, hits=c.counters()["raw_hits"]), dict(rows=want)


@case("cover_scan: hash-seeded, random anchors", SCAN_ENTRIES)
def _scan_seed_random(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 5, 100, 0, 50, engine.SCAN_SEED, seed=12)
    return dict(rows=got), dict(rows=want)


@case("cover_scan: general, table look-up and extension on the planes", SCAN_ENTRIES)
def _scan_general(c, oracle):
    from catch_amd import engine
    got, want = _scan_case(c, oracle, 3, 80, 25, 10, engine.SCAN_GENERAL, seed=13)
    return dict(rows=got, hits=c.counters()["raw_hits"]), dict(rows=want)


@case("cover_scan: general, any alphabet", SCAN_ENTRIES)
def _scan_general_bytes(c, oracle):
    from test_gpu_parity import _oracle_rows, _scan_rows
    rng = random.Random(9)
    alpha = "ABCDEFGHIJKLMNOPQRSTUVWXYZacgt"
    seq = "".join(rng.choice(alpha) for _ in range(677))
    genomes = [[seq], [seq[100:400].lower() + seq[400:]]]
    probes = [seq[i:i + 20] for i in range(0, 650, 7)]
    got = _scan_rows(c, probes, genomes, 1, 20, 0, 2, min_k=5)
    if "bytes" not in _cache:
        _cache["bytes"] = _oracle_rows(oracle, probes, genomes, 1, 20, 0, 2, min_k=5)
    return dict(rows=got), dict(rows=_cache["bytes"])


@case("cover_ranges", ["catchhip_cover_ranges"])
def _cover_ranges(c, oracle):
    from catch_amd import engine
    from test_gpu_parity import _scan_rows
    from util import candidates
    rng = random.Random(17)
    unit = "".join(rng.choice("ACGT") for _ in range(60))
    seq = unit * 12 + "".join(rng.choice("ACGT") for _ in range(225)) + unit * 3
    assert len(seq) % 64 == 37
    probes = candidates([[seq]], 50, 10)
    got, want = {}, {}
    for name, m, thres, mode in (("seed", 1, 50, engine.SCAN_AUTO), ("general", 2, 35, engine.SCAN_AUTO)):
        np.random.seed(3)
        got[name] = _scan_rows(c, probes, [[seq]], m, thres, 0, 5, mode, min_k=10, merge=False)
        if ("ranges", name) not in _cache:
            np.random.seed(3)
            k, entries = oracle.anchor_table(probes, m, thres, min_k=10, k=10)
            uniq, owner = oracle._unique_last(probes)
            cov = oracle.scan_sequence(seq, uniq, entries, k, m, thres, 0, merge=False)
            _cache["ranges", name] = sorted(set((int(owner[p]), 0, max(0, a - 5), min(len(seq), b + 5))
                                                for p, v in cov.items() for a, b in v))
        want[name] = _cache["ranges", name]
    return got, want


@case("tolerant_bp", ["catchhip_tolerant_bp"])
def _tolerant_bp(c, oracle):
    from catch_amd import engine, probe
    from test_gpu_parity import _oracle_rows
    genomes, probes = scan_input()
    k, uniq, owner, ep, eo = probe.anchor_table(probes, 2, 100)
    out = np.zeros(len(uniq), dtype=np.int64)
    with closing(engine.Targets(c, genomes), engine.Probes(c, uniq, owner, ep, eo, k)) as (t, p):
        engine.tolerant_bp(c, p, t, 2, 100, 0, out)
    if "bp" not in _cache:
        rows = _oracle_rows(oracle, probes, [[s] for g in genomes for s in g], 2, 100, 0, 0)
        want = np.zeros(len(probes), dtype=np.int64)
        for sid, _u, a, b in rows:
            want[sid] += b - a
        _cache["bp"] = want[np.asarray(owner)]
    return dict(bp=out), dict(bp=_cache["bp"])


@case("first-seen scan, adapter votes", ["catchhip_cover_scan_first_seen", "catchhip_rows_fetch_first_seen",
                                         "catchhip_rows_first_seen_per_set", "catchhip_adapter_votes"])
def _first_seen(c, oracle):
    from test_adapter_votes import NUNIV, _scan, make_input, replay_first_seen_per_set, replay_votes
    got, want = {}, {}
    for name in ("A", "B"):                              # the seed scan's work list, and the general scan's hit list
        inp = make_input(oracle, name)
        with closing(_scan(c, inp.uniq, inp.entries, inp.k, inp.seqs, inp.m, inp.thres, inp.ent_rank)) as rows:
            si, un, st, en = rows.fetch()
            keys = rows.fetch_first_seen()
            a, b = rows.adapter_votes(inp.mult)
            fu, fk = rows.first_seen_per_set(len(inp.uniq))
        got[name] = dict(set=si, universe=un, start=st, end=en, keys=keys, votes=list(zip(a.tolist(), b.tolist())),
                         first=list(zip(fu.tolist(), fk.tolist())))
        want[name] = dict(set=inp.cols[0], universe=inp.cols[1], start=inp.cols[2], end=inp.cols[3], keys=inp.cols[4],
                          votes=[list(v) for v in replay_votes(*inp.cols, inp.mult, NUNIV)[0]],
                          first=[list(v) for v in replay_first_seen_per_set(inp.cols[0], inp.cols[1], inp.cols[4], len(inp.uniq))])
        got[name]["votes"] = [list(v) for v in got[name]["votes"]]
        got[name]["first"] = [list(v) for v in got[name]["first"]]
    return got, want


# ------------------------------------------------------------------ fused and multi-context entries
def _filter_inputs(c, genomes, probes, m=2):
    from catch_amd import engine, probe
    k, uniq, owner, ep, eo = probe.anchor_table(probes, m, 100)
    return engine.Targets(c, genomes), engine.Probes(c, uniq, owner, ep, eo, k)


def _oracle_filter(oracle, key, probes, genomes, coverage, ext):
    if key not in _cache:
        _cache[key] = sorted(oracle.set_cover_filter([probes], [genomes], 2, 100, coverage=coverage, cover_extension=ext)[0])
    return _cache[key]


FILTER_ENTRIES = ["catchhip_setcover_filter", "catchhip_ctx_last_capacity_events"]


@case("setcover_filter: scan and solve queued together", FILTER_ENTRIES)
def _filter_deferred(c, oracle):
    from catch_amd import engine
    genomes, probes = scan_input()
    with closing(*_filter_inputs(c, genomes, probes)) as (t, p):
        ids, nrows = engine.setcover_filter(c, p, t, 2, 100, 0, 50, len(probes))
        events = c.capacity_events()
    return (dict(ids=ids, picked=sorted(ids), nrows=nrows, events=events),
            dict(picked=_oracle_filter(oracle, "filter 1.0", probes, genomes, 1.0, 50), events={k: 0 for k in events}))


@case("setcover_filter: synchronous, direct rows", FILTER_ENTRIES, CATCHHIP_FILTER_NO_DEFER="1", CATCHHIP_FLAT_MIN_ROWS="0")
def _filter_direct(c, oracle):
    from catch_amd import engine
    genomes, probes = scan_input()
    with closing(*_filter_inputs(c, genomes, probes)) as (t, p):
        ids, nrows = engine.setcover_filter(c, p, t, 2, 100, 0, 50, len(probes))
        assert c.counters()["rows_direct"] == 1
        part, _n = engine.setcover_filter(c, p, t, 2, 100, 0, 50, len(probes), None, [0.9] * len(genomes))
    return (dict(ids=ids, picked=sorted(ids), nrows=nrows, partial=part, partial_picked=sorted(part)),
            dict(picked=_oracle_filter(oracle, "filter 1.0", probes, genomes, 1.0, 50),
                 partial_picked=_oracle_filter(oracle, "filter 0.9", probes, genomes, 0.9, 50)))


@case("setcover_filter: synchronous, the SoA table", FILTER_ENTRIES, CATCHHIP_FILTER_NO_DEFER="1", CATCHHIP_ROWS_SOA="1")
def _filter_soa(c, oracle):
    from catch_amd import engine
    genomes, probes = scan_input()
    with closing(*_filter_inputs(c, genomes, probes)) as (t, p):
        ids, nrows = engine.setcover_filter(c, p, t, 2, 100, 0, 50, len(probes))
    return dict(ids=ids, picked=sorted(ids), nrows=nrows), dict(picked=_oracle_filter(oracle, "filter 1.0", probes, genomes, 1.0, 50))


@case("setcover_filter_many over three contexts", ["catchhip_setcover_filter_many", "catchhip_targets_rebind",
                                                   "catchhip_probes_rebind"])
def _filter_many(c, oracle):
    from catch_amd import engine
    from util import candidates
    genomes, _probes = scan_input()
    groups = [genomes[:3], genomes[1:4], genomes[2:]]
    ctxs = [c, engine.Context(c.device), engine.Context(c.device)]
    objs, res = [], None
    try:
        args = []
        for g, cx in zip(groups, ctxs):
            probes = candidates(g, 100, 50)
            # built on the first context and handed over, as the upload lanes do
            t, p = _filter_inputs(c, g, probes)
            objs += [t, p]
            args.append((cx, p.rebind(cx), t.rebind(cx), len(probes), None, None))
        res = engine.setcover_filter_many(args, 2, 100, 0, 50)
    finally:
        for o in reversed(objs):
            o.close()
        for cx in ctxs[1:]:
            cx.close()
    got = {"group %d" % i: dict(ids=ids, picked=sorted(ids), nrows=n) for i, (ids, n) in enumerate(res)}
    want = {"group %d" % i: dict(picked=_oracle_filter(oracle, "many %d" % i, candidates(g, 100, 50), g, 1.0, 50))
            for i, g in enumerate(groups)}
    return got, want


@case("setcover_grid, rows_extend", ["catchhip_setcover_grid", "catchhip_rows_extend", "catchhip_ctx_last_grid_counters"])
def _grid(c, oracle):
    from catch_amd import engine
    from test_gpu_parity import _oracle_rows
    from util import rows_as_tuples
    genomes, probes = scan_input()
    exts = [0, 10, 50, 65]
    with closing(*_filter_inputs(c, genomes, probes)) as (t, p):
        res = engine.setcover_grid(c, p, t, 2, 100, 0, exts, len(probes))
        counters = c.grid_counters()
        with closing(engine.Rows.scan(c, p, t, 2, 100, 0, 0)) as r0:
            derived = r0.extend(t, exts)
            tables = {}
            for e, d in zip(exts, derived):
                tables[e] = dict(rows=rows_as_tuples(*d.fetch()), gain0=d.fetch_gain0(len(probes)), longest=d.longest())
                d.close()
    got = dict(grid={e: dict(ids=ids, picked=sorted(ids), nrows=n) for e, (ids, n) in zip(exts, res)},
               counters=counters, tables=tables)
    want = dict(grid={}, tables={})
    for e in exts:
        if ("grid", e) not in _cache:
            _cache["grid", e] = (_oracle_filter(oracle, "grid %d" % e, probes, genomes, 1.0, e),
                                 _oracle_rows(oracle, probes, genomes, 2, 100, 0, e))
        want["grid"][e] = dict(picked=_cache["grid", e][0], nrows=len(_cache["grid", e][1]))
        want["tables"][e] = dict(rows=_cache["grid", e][1])
    return got, want


@case("pool_solve", ["catchhip_pool_solve"])
def _pool_solve(c, oracle):
    from test_pool import _restate, _solve
    rng = np.random.default_rng(65)
    inst = []                                            # 65 datasets of up to 8 options (tests/test_pool.py's form)
    for d in range(65):
        counts = sorted(int(x) for x in rng.integers(1, 400, size=int(rng.integers(1, 9))))
        inst.append(("d%02d" % d, [((k,), n, float(rng.integers(1, 64)) / 8.0) for k, n in enumerate(counts)]))
    budget = sum(min(n for _p, n, _l in opts) for _d, opts in inst) + 2049      # 2,050 cells and more: nine workgroups
    choice, total, loss = _solve(c, inst, budget)
    if "pool" not in _cache:
        _cache["pool"] = _restate(inst, budget)
    w = _cache["pool"]
    return dict(choice=choice, total=total, loss=loss), dict(choice=w[0], total=w[1], loss=w[2])


@case("grouped union: device candidates and string probes, banded rounds",
      ["catchhip_targets_set_groups", "catchhip_probes_set_groups", "catchhip_probes_from_candidates"],
      CATCHHIP_FILTER_NO_DEFER="1", CATCHHIP_FLAT_MIN_ROWS="0", CATCHHIP_FLAT_BANDS_GROUPED="2", CATCHHIP_FLAT_BAND_RATIO="500")
def _grouped_union(c, oracle):
    from catch_amd import engine, probe
    from test_banded_union import _per_group, _union
    from util import candidates
    genomes, _probes = scan_input()
    groups = [genomes[:3], genomes[3:]]                  # (the border between them lies inside a word)
    assert sum(len(s) for g in groups[0] for s in g) % 64
    strs = [candidates(g, 100, 50) for g in groups]
    t, cd, p = _union(c, engine, groups, [0, 1])
    with closing(t, cd, p):
        cg = cd.groups()
        ids, nrows = engine.setcover_filter(c, p, t, 2, 100, 0, 50, cd.n, None, None)
        cn = c.counters()
        assert cn["rows_direct"] == 1 and cn["flat_bands"] == 2 and cn["flat_band_groups"] == 2
    device = _per_group(ids, cg, [0, 1], [len(s) for s in strs])
    # the same union from strings: group numbers given for the probes too
    flat = strs[0] + strs[1]
    k, uniq, owner, ep, eo = probe.anchor_table(flat, 2, 100, assume_unique=True)
    with closing(engine.Targets(c, genomes), engine.Probes(c, uniq, owner, ep, eo, k)) as (t, p):
        t.set_groups(np.repeat(np.arange(2), [len(g) for g in groups]))
        p.set_groups(np.repeat(np.arange(2), [len(s) for s in strs]))
        ids2, nrows2 = engine.setcover_filter(c, p, t, 2, 100, 0, 50, len(flat), None, None)
    strings = [[int(x) for x in ids2 if x < len(strs[0])], [int(x) - len(strs[0]) for x in ids2 if x >= len(strs[0])]]
    if "union" not in _cache:
        _cache["union"] = [sorted(w) for w in oracle.set_cover_filter(strs, groups, 2, 100, coverage=1.0, cover_extension=50)]
    return (dict(ids=ids, nrows=nrows, ids_strings=ids2, nrows_strings=nrows2, device=[sorted(x) for x in device],
                 strings=[sorted(x) for x in strings]),
            dict(device=_cache["union"], strings=_cache["union"]))


# ------------------------------------------------------------------ candidates and filters
def _pad_to_37(seqs, L, seed):
    """seqs and one sequence more of at least L random bases, so that the bases add up to 37 (mod 64)."""
    rnd = random.Random(seed)
    total = sum(len(s) for s in seqs)
    return list(seqs) + ["".join(rnd.choice("ACGT") for _ in range(L + (37 - total - L) % 64))]


def _listed(cands, concat):
    """The defined content of a candidate list: the windows in order, their groups and multiplicities, the counts."""
    pos = cands.positions()
    return dict(windows=[concat[p:p + cands.L] for p in pos.tolist()], groups=cands.groups(), mult=cands.multiplicities(),
                positions=pos, n=cands.n, ncandidates=cands.ncandidates)


def _model_list(key, seqs, L, stride, group_of=None, skip=None):
    """tests/test_candidate_list.py's restatement of the list, as NumPy arrays; computed once."""
    from test_candidate_list import per_sequence
    if key not in _cache:
        ncand, windows, groups, mult = per_sequence(seqs, L, stride, skip, group_of)
        _cache[key] = dict(windows=windows, groups=np.array(groups, dtype=np.int64), mult=np.array(mult, dtype=np.int64),
                           ncandidates=ncand, n=len(windows))
    return _cache[key]


def _masked(model, keep):
    keep = np.asarray(keep, dtype=bool)
    return dict(windows=[w for w, k in zip(model["windows"], keep.tolist()) if k], groups=model["groups"][keep],
                mult=model["mult"][keep], n=int(keep.sum()), ncandidates=model["ncandidates"])


def _filter_case(c, key, seqs, L, stride, apply, expect):
    """One drop_* call on the candidates of seqs: apply(cands) -> further outputs; expect(model list) -> (keep mask,
    further outputs) by the family's own rule.  The list before and after goes through the model of the list."""
    from catch_amd import engine
    concat = "".join(seqs)
    with closing(engine.Targets(c, [[s] for s in seqs])) as t:
        with closing(engine.Candidates(c, t, L, stride)) as cd:
            before = _listed(cd, concat)
            more = apply(cd)
            after = _listed(cd, concat)
    model = _model_list(key, seqs, L, stride)
    if (key, "expect") not in _cache:
        _cache[key, "expect"] = expect(model)
    keep, want_more = _cache[key, "expect"]
    assert 0 < int(np.sum(keep)) < model["n"] and model["mult"].max() > 1 and model["n"] > 256
    del before["positions"], after["positions"]
    return dict(before=before, after=after, more=more), dict(before=model, after=_masked(model, keep), more=want_more)


@case("candidates: windows, groups, multiplicities, positions by id",
      ["catchhip_candidates_create", "catchhip_candidates_destroy", "catchhip_candidates_fetch", "catchhip_candidates_groups",
       "catchhip_candidates_multiplicities"])
def _candidate_list(c, oracle):
    from catch_amd import engine
    from test_candidate_list import random_form
    L, stride = 9, 2
    seqs = _pad_to_37(random_form(L)[:4000], L, 5)
    group_of = [q % 3 for q in range(len(seqs))]
    concat = "".join(seqs)
    got = {}
    with closing(engine.Targets(c, [[s] for s in seqs])) as t:
        for name, groups, skip in (("one group", None, None), ("short ones skipped", None, 10), ("three groups", group_of, None)):
            if groups is not None:
                t.set_groups(np.asarray(groups, dtype=np.int32))
            with closing(engine.Candidates(c, t, L, stride, seq_length_to_skip=skip)) as cd:
                got[name] = _listed(cd, concat)
                ids = np.random.default_rng(9).permutation(cd.n)[:65]        # 65 of them, in no order
                got[name]["by id"] = cd.positions(ids)
                assert ids.size == 65 and got[name]["by id"].tolist() == got[name]["positions"][ids].tolist()
    want = {"one group": _model_list("list 1", seqs, L, stride),
            "short ones skipped": _model_list("list skip", seqs, L, stride, None, 10),
            "three groups": _model_list("list 3", seqs, L, stride, group_of)}
    assert want["one group"]["n"] > want["short ones skipped"]["n"] > 1024 and want["three groups"]["mult"].max() > 1
    return got, want


@case("candidates_drop_polya", ["catchhip_candidates_drop_polya"])
def _drop_polya(c, oracle):
    from test_design_filters import _np_keep, _sequences_with_unique_windows
    if "polya seqs" not in _cache:
        _cache["polya seqs"] = _pad_to_37(_sequences_with_unique_windows(np.random.default_rng(1100), 100, 50, 1025), 100, 6)
    seqs = _cache["polya seqs"]
    return _filter_case(c, "polya", seqs, 100, 50, lambda cd: cd.drop_polya(12, 2, 6),
                        lambda m: (_np_keep(m["windows"], 100, 12, 2, 6), None))


@case("candidates_drop_composition", ["catchhip_candidates_drop_composition"])
def _drop_composition(c, oracle):
    from test_composition_filter import CF, _expect, _targets
    seqs = _pad_to_37(_targets(1100, 100, 50, 700), 100, 7)
    kwargs = dict(gc_range=("0.35", "0.6"), max_homopolymer=5, max_dust=20)

    def apply(cd):
        f = CF(**kwargs)
        f._apply_to_candidates(cd)
        return list(f.dropped)
    return _filter_case(c, "composition", seqs, 100, 50, apply,
                        lambda m: _expect(CF(**kwargs), m["windows"], m["mult"], 100))


@case("candidates_drop_structure", ["catchhip_candidates_drop_structure"])
def _drop_structure(c, oracle):
    from test_structure_filter import _candidates, _expected
    L, K, P, D = 100, 3, 3, 4
    seqs = _candidates(L)                                # (one sequence per candidate, stride = L)

    def expect(m):
        table = _expected(L, K, P, D)
        fails = np.array([table[s] for s in m["windows"]], dtype=bool).reshape(-1, 2)
        drop = fails[:, 0] | fails[:, 1]
        return ~drop, [int(m["mult"][fails[:, 0]].sum()), int(m["mult"][fails[:, 1]].sum()), int(m["mult"][drop].sum())]
    return _filter_case(c, "structure", seqs, L, L, lambda cd: cd.drop_structure(K, P, D), expect)


@case("candidates_drop_tm", ["catchhip_candidates_drop_tm"])
def _drop_tm(c, oracle):
    from test_tm_filter import TF, _expect, _settings, _targets
    seqs = _pad_to_37(_targets(1100, 100, 50, 700), 100, 8)
    if "tm filter" not in _cache:
        _cache["tm filter"] = _settings(_model_list("tm", seqs, 100, 50)["windows"])[0][1]
    f = TF(**_cache["tm filter"])

    def expect(m):
        keep, three, hist = _expect(f, m["windows"], m["mult"], 100)
        return keep, [three, hist]
    return _filter_case(c, "tm", seqs, 100, 50, lambda cd: list(cd.drop_tm(f._q(100), f.offset_c, f.lo_c, f.hi_c)), expect)


def _background_case(c, key, mod, K, M):
    """drop_background and the index behind it, by tests/test_background_filter.py (M = 0) or
    tests/test_background_mismatches.py (M > 0)."""
    from catch_amd import engine
    records = mod._background(200 + K + M, K)
    seqs = _pad_to_37(mod._targets(3000 + 37 * K + M, 100, 50, 500, records, K), 100, 9)
    f = mod.BF(records, kmer=K, **({"mismatches": M} if M else {}))
    if key not in _cache:                                # the threshold: the median, so that about half of them go
        _cache[key] = int(np.median(f._hits_equal_length(_model_list((key, "list"), seqs, 100, 50)["windows"], 100)))
    H = _cache[key]
    index = engine.KmerIndex(c, records, K, mismatches=M)
    try:
        views = {"counts": [index.n_valid, index.n_unique], "codes": index.fetch()}
        for b in range(M + 1):
            views["view %d" % b] = index.fetch_view(b)

        def expect(m):
            out = mod._expect(mod.BF(records, kmer=K, max_hits=H, **({"mismatches": M} if M else {})), m["windows"], m["mult"], 100)
            return out[0], [out[1], out[2]]
        got, want = _filter_case(c, (key, "list"), seqs, 100, 50, lambda cd: list(cd.drop_background(index, H)), expect)
    finally:
        index.close()
    codes = mod._canonical_codes(records, K)
    distinct = sorted(set(codes))
    want_views = {"counts": [len(codes), len(distinct)], "codes": np.array(distinct, dtype=np.uint64), "view 0": np.array(distinct, dtype=np.uint64)}
    for b in range(1, M + 1):
        want_views["view %d" % b] = np.array(sorted(mod._rotl(x, 2 * mod._starts(K, M)[b], K) for x in distinct), dtype=np.uint64)
    return dict(got, index=views), dict(want, index=want_views)


@case("candidates_drop_background, the exact index", ["catchhip_candidates_drop_background", "catchhip_kmer_index_create",
                                                     "catchhip_kmer_index_fetch", "catchhip_kmer_index_destroy"])
def _drop_background(c, oracle):
    import test_background_filter
    return _background_case(c, "background", test_background_filter, 32, 0)


@case("candidates_drop_background, an index tolerant of one mismatch", ["catchhip_kmer_index_create_tolerant",
                                                                        "catchhip_kmer_index_fetch_view"])
def _drop_background_tolerant(c, oracle):
    import test_background_mismatches
    return _background_case(c, "background 1", test_background_mismatches, 32, 1)


@case("candidates_measure", ["catchhip_candidates_measure"])
def _measure(c, oracle):
    from catch_amd import engine
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.filter.tm_filter import TmFilter
    from test_quality_measure import FIVE, _candidates, _composition, _hist_of, _structure
    L = 100
    seqs = _candidates(L)
    concat = "".join(seqs)
    model = _model_list("measure", seqs, L, L)
    strs = model["windows"]
    tf = TmFilter(sodium_mm="75", formamide_pct="5")
    records = ["".join(strs[:40]), "".join(s for s in strs[40:60] if set(s) <= set("ACGT"))]
    bf = BackgroundFilter(records, kmer=12)
    with closing(engine.Targets(c, [[s] for s in seqs])) as t:
        with closing(engine.Candidates(c, t, L, L), engine.KmerIndex(c, records, 12)) as (cd, index):
            before = _listed(cd, concat)
            got = cd.measure(what=("composition", "structure", "tm", "hits"), min_loop=3, dust_window=64,
                             tm=(tf._q(L), tf.offset_c), index=index, values=True, histograms=True)
            alone = cd.measure(what="structure", min_loop=7, values=True, histograms=False)
            after = _listed(cd, concat)
    del before["positions"]
    if "measure values" not in _cache:
        comp, struct = _composition(L, 64), _structure(L, 3)
        five = np.array([comp[s] + struct[s] for s in strs], dtype=np.int64).reshape(len(strs), 5)
        want = {name: five[:, k] for k, name in enumerate(FIVE)}
        want["histograms"] = {name: _hist_of(five[:, k], model["mult"].astype(np.float64)) for k, name in enumerate(FIVE)}
        want["tm_c"] = tf._tm_c_equal_length(strs, L)
        want["hits"] = bf._hits_equal_length(strs, L)
        s7 = _structure(L, 7)
        _cache["measure values"] = (want, {"stem": np.array([s7[s][0] for s in strs]), "dimer": np.array([s7[s][1] for s in strs])})
    want, want_alone = _cache["measure values"]
    assert _differing(before, {k: v for k, v in after.items() if k != "positions"}) == []
    return dict(before=before, all=got, structure=alone), dict(before=model, all=want, structure=want_alone)


@case("probes_from_candidates: pigeonhole anchors, given anchors, anchors from draws",
      ["catchhip_probes_from_candidates_draws"])
def _probes_from_candidates(c, oracle):
    from catch_amd import engine, probe
    from util import candidates, rows_as_tuples
    genomes, strs = scan_input()
    got = {}
    with closing(engine.Targets(c, genomes)) as t:
        with closing(engine.Candidates(c, t, 100, 50)) as cd:
            assert cd.n == len(strs)
            np.random.seed(2)
            k5, _uniq, _owner, ep, eo = probe.anchor_table(strs, 5, 100, assume_unique=True)
            np.random.seed(2)
            k5d, draws = probe.anchor_draws_equal_length(cd.n, 100, 5, 100)
            assert k5d == k5
            k2 = probe.anchor_table(strs[:1], 2, 100, assume_unique=True)[0]
            for name, m, make in (("pigeonhole", 2, lambda: cd.probes(k2)), ("given", 5, lambda: cd.probes(k5, ep, eo)),
                                  ("draws", 5, lambda: cd.probes_from_draws(k5, draws))):
                with closing(make()) as p:
                    with closing(engine.Rows.scan(c, p, t, m, 100, 0, 50)) as r:
                        got[name] = rows_as_tuples(*r.fetch())
    from test_gpu_parity import _oracle_rows
    if "from candidates" not in _cache:
        np.random.seed(2)
        five = _oracle_rows(oracle, strs, genomes, 5, 100, 0, 50)
        _cache["from candidates"] = dict(pigeonhole=_oracle_rows(oracle, strs, genomes, 2, 100, 0, 50), given=five, draws=five)
    return got, _cache["from candidates"]


# ------------------------------------------------------------------ near-duplicate filters
NDF_SIZES = (257, 8193, 65)                              # a group the device orders (8,192 kept and more) between two of the host's


def _chains(sizes):
    from test_candidate_list import chain_genome
    return [chain_genome(n, 700 + 10 * i + n) for i, n in enumerate(sizes)]


def _kept_want(oracle, sizes, kind, thres):
    from test_candidate_list import _oracle_list
    return [_oracle_list(oracle, ("chain", n, 700 + 10 * i + n), seqs, kind, thres)
            for i, (n, seqs) in enumerate(zip(sizes, _chains(sizes)))]


@case("candidates_ndf_hamming, candidates_ndf_hamming_many", ["catchhip_candidates_ndf_hamming", "catchhip_candidates_ndf_hamming_many"])
def _candidates_ndf_hamming(c, oracle):
    from test_candidate_list import POSITIONS, _kept, _oracle_list, planted_genome
    planted = planted_genome(1025, 65, 511)
    one = _kept(c, [planted[0]], False, lambda cd: cd.ndf_hamming(POSITIONS, 1))
    many = _kept(c, _chains(NDF_SIZES), True, lambda cd: cd.ndf_hamming_many([POSITIONS] * len(NDF_SIZES), 0))
    want_one = _oracle_list(oracle, ("planted", 1025, 511), planted[0], "hamming", 1)
    want_many = _kept_want(oracle, NDF_SIZES, "hamming", 0)
    assert len(want_one) <= 1025 and len(want_many[1]) == 8193
    return (dict(one=[list(x) for x in one], many=[list(x) for x in many]),
            dict(one=[[0, w] for w in want_one], many=[[g, w] for g, ws in enumerate(want_many) for w in ws]))


@case("candidates_ndf_minhash, candidates_ndf_minhash_many", ["catchhip_candidates_ndf_minhash", "catchhip_candidates_ndf_minhash_many"])
def _candidates_ndf_minhash(c, oracle):
    from test_candidate_list import MINHASH_KMER, MINHASH_PARAMS, _kept, _oracle_list, chain_genome
    sizes, thres = (257, 1025, 65), 0.2                  # (from 1/7 on a kept window drops its neighbours: about half stay)
    chain = chain_genome(1025, 811)
    one = _kept(c, [chain], False, lambda cd: cd.ndf_minhash(MINHASH_KMER, MINHASH_PARAMS, thres))
    many = _kept(c, _chains(sizes), True, lambda cd: cd.ndf_minhash_many(MINHASH_KMER, [MINHASH_PARAMS] * len(sizes), thres))
    want_one = _oracle_list(oracle, ("chain", 1025, 811), chain, "minhash", thres)
    want_many = _kept_want(oracle, sizes, "minhash", thres)
    assert 100 < len(want_one) < 900
    return (dict(one=[list(x) for x in one], many=[list(x) for x in many]),
            dict(one=[[0, w] for w in want_one], many=[[g, w] for g, ws in enumerate(want_many) for w in ws]))


@case("ndf_hamming, ndf_minhash, ndf_minhash_many on strings", ["catchhip_ndf_hamming", "catchhip_ndf_minhash", "catchhip_ndf_minhash_many"])
def _ndf_strings(c, oracle):
    from catch_amd.filter.near_duplicate_filter import _order_strs_by_multiplicity
    from test_candidate_list import MINHASH_KMER, MINHASH_PARAMS, PL, POSITIONS, chain_genome, planted_genome, replay
    sizes, thres = (257, 1025, 65), 0.2
    planted = replay(planted_genome(1025, 65, 511)[0], PL, 1)
    chains = [replay(seqs, PL, 1) for seqs in [chain_genome(1025, 811)] + _chains(sizes)]
    order = _order_strs_by_multiplicity(planted)         # (the filters' priority order: what the entries are given)
    orders = [_order_strs_by_multiplicity(w) for w in chains]
    keep_h = c.ndf_hamming(order, PL, POSITIONS, 1)
    keep_m = c.ndf_minhash(orders[0], MINHASH_KMER, MINHASH_PARAMS, thres)
    keep_many = c.ndf_minhash_many(orders[1:], MINHASH_KMER, [MINHASH_PARAMS] * len(sizes), thres)
    got = dict(hamming=keep_h, minhash=keep_m, many=list(keep_many),
               hamming_kept=sorted(s for s, k in zip(order, keep_h) if k),
               minhash_kept=sorted(s for s, k in zip(orders[0], keep_m) if k),
               many_kept=[sorted(s for s, k in zip(o, kp) if k) for o, kp in zip(orders[1:], keep_many)])
    if "ndf strings" not in _cache:
        _cache["ndf strings"] = dict(
            hamming_kept=sorted(oracle.ndf_hamming_c(planted, 1, POSITIONS)),
            minhash_kept=sorted(oracle.ndf_minhash(chains[0], thres, MINHASH_PARAMS, kmer_size=MINHASH_KMER)),
            many_kept=[sorted(oracle.ndf_minhash(w, thres, MINHASH_PARAMS, kmer_size=MINHASH_KMER)) for w in chains[1:]])
    return got, _cache["ndf strings"]


@case("pyset_order_device", ["catchhip_pyset_order_device"])
def _pyset_order(c, oracle):
    got, want = {}, {}
    for n in (1025, 50001):                              # (tables grow fourfold up to 50,000 keys, twofold beyond)
        keys = [int(x) for x in np.random.RandomState(n).permutation(4 * n)[:n] + 1]     # hash(i) == i
        s = set()
        for k in keys:
            s.add(k)
        order = c.pyset_order(np.asarray(keys, dtype=np.int64))
        got[n] = dict(order=order, keys=[keys[i] for i in order.tolist()])
        want[n] = dict(keys=list(s))
    return got, want


# ------------------------------------------------------------------ redundancy graph
@case("redundancy graph: the graph, the naive pass, the rows of the dominating set",
      ["catchhip_redundancy_graph", "catchhip_redundancy_fetch", "catchhip_redundancy_naive", "catchhip_redundancy_rows",
       "catchhip_redundancy_destroy"])
def _redundancy(c, oracle):
    from catch_amd import engine
    from test_naive import _probe_set, naive_loop, restate_graph
    strs = _probe_set(np.random.default_rng(257), 257, 40, 0.01)
    got, want = {}, {}
    for kind, code, p0, p1 in (("lcf", engine.REDUNDANT_LCF, 2, 20), ("shift", engine.REDUNDANT_SHIFT, 5, 3)):
        with closing(engine.RedundancyGraph(c, strs, code, p0, p1)) as g:
            ptr, idx = g.fetch()
            keep = g.naive()
            with closing(g.rows()) as r:
                got[kind] = dict(fetched(r), ptr=ptr, idx=idx, keep=keep, nedges=g.nedges, rows=r.n)
        if ("redundancy", kind) not in _cache:
            adj = restate_graph(strs, kind, p0, p1)
            row, col = np.nonzero(adj)
            wptr = np.concatenate(([0], np.cumsum(adj.sum(axis=1))))
            with_self = adj.copy()
            np.fill_diagonal(with_self, True)
            ws, we = np.nonzero(with_self)
            _cache["redundancy", kind] = dict(ptr=wptr, idx=col, keep=naive_loop(wptr, col), nedges=int(col.size), set=ws,
                                              universe=np.zeros(ws.size, dtype=np.int64), start=2 * we, end=2 * we + 1,
                                              rows=int(ws.size))
        want[kind] = _cache["redundancy", kind]
        assert want[kind]["nedges"] > 0
    return got, want


# ------------------------------------------------------------------ clustering
def _signatures_from_one_buffer(c, seqs, k, N, a, b):
    """engine.Signatures through catchhip_sigs_create (the engine itself hands over one pointer per sequence)."""
    import ctypes
    from catch_amd import engine
    s = engine.Signatures.__new__(engine.Signatures)
    s.ctx, s.n, s.N, s._h = c, len(seqs), int(N), ctypes.c_void_p()
    buf = np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8).copy()
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    engine.check(c._L.catchhip_sigs_create(c._h, engine._ptr(buf, engine.c_u8p), engine._ptr(off, engine.c_u64p), s.n, int(k),
                                           s.N, int(a), int(b), ctypes.byref(s._h)))
    return s


@cached
def signature_input():
    """65 sequences of ragged lengths cut from one root, a few characters spoilt, two of them equal; 37 (mod 64) bases."""
    rnd = random.Random(65)
    root = "".join(rnd.choice("ACGT") for _ in range(900))
    seqs = []
    for _ in range(65):
        ln = rnd.randrange(300, 901)
        st = rnd.randrange(0, 900 - ln + 1)
        s = list(root[st:st + ln])
        for _ in range(rnd.choice([0, 0, 1, 3, 10, 40])):
            s[rnd.randrange(ln)] = rnd.choice("ACGTNacgtRY-")
        seqs.append("".join(s))
    seqs[0] = seqs[-1]
    cut = (sum(map(len, seqs)) - 37) % 64
    seqs[1] = seqs[1][:len(seqs[1]) - cut]
    assert sum(map(len, seqs)) % 64 == 37 and len(seqs[1]) > 100
    return tuple(seqs)


@case("signatures: rows, neighbour lists, the graph, the condensed matrix",
      ["catchhip_sigs_create", "catchhip_sigs_create_ptrs", "catchhip_sigs_fetch", "catchhip_sigs_destroy",
       "catchhip_sigs_common_row", "catchhip_sigs_neighbors", "catchhip_sigs_neighbors_many", "catchhip_sigs_graph",
       "catchhip_sigs_graph_fetch", "catchhip_sigs_condensed"])
def _signatures(c, oracle):
    from catch_amd import engine
    seqs, k, N, a, b, least = list(signature_input()), 12, 100, 123456789, 987654321, 20
    n = len(seqs)
    js = [0, 1, 31, 32, 33, 64]
    lut = (1.0 - np.arange(N + 1, dtype=np.float64) / float(N)).astype(np.float32)
    with closing(engine.Signatures(c, seqs, k, N, a, b), _signatures_from_one_buffer(c, seqs, k, N, a, b)) as (s, s1):
        got = dict(signatures=s.fetch(), from_one_buffer=s1.fetch(), rows={j: s.common_row(j) for j in js},
                   lists={j: list(s.neighbors(j, least)) for j in js}, many=[list(x) for x in s.neighbors_many(js, least)],
                   graph=list(s.graph(least)), condensed=s.condensed(lut))
    if "signatures" not in _cache:
        sig = [oracle.minhash_signature(x, k, N, a, b) for x in seqs]
        common = np.array([[oracle.signature_common(sig[i], sig[j], N)[0] for j in range(n)] for i in range(n)], dtype=np.int64)
        near = [np.nonzero(common[i] >= least)[0] for i in range(n)]
        others = [x[x != i] for i, x in enumerate(near)]
        _cache["signatures"] = dict(
            signatures=np.array(sig, dtype=np.int64), from_one_buffer=np.array(sig, dtype=np.int64),
            rows={j: common[j] for j in js}, lists={j: [near[j], common[j][near[j]]] for j in js},
            many=[[near[j], common[j][near[j]]] for j in js],
            graph=[np.concatenate(([0], np.cumsum([x.size for x in others]))), np.concatenate(others),
                   np.concatenate([common[i][x] for i, x in enumerate(others)])],
            condensed=oracle.condensed_dist_matrix(n, lambda i, j: oracle.estimate_jaccard_dist(sig[i], sig[j], N)))
    return got, _cache["signatures"]


@case("sigs_linkage_average: the recorded hierarchical clusterings", ["catchhip_sigs_linkage_average"])
def _sigs_linkage(c, oracle):
    from catch_amd import engine
    from catch_amd.utils import cluster
    from test_linkage import _hierarchical_records, _rows_of
    _g, recs = _hierarchical_records()
    got, want = {}, {}
    for i, rec in enumerate(recs):
        lut = (1.0 - np.arange(rec["N"] + 1, dtype=np.float64) / float(rec["N"])).astype(np.float32)
        thr = cluster._jaccard_dist_from_mash_dist(rec["threshold"], rec["k"])
        with closing(engine.Signatures(c, rec["seqs"], rec["k"], rec["N"], rec["a"], rec["b"])) as s:
            cl, merges = s.linkage_clusters(lut, thr, return_merges=True)
        got[i] = dict(clusters=[[rec["names"][j] for j in x] for x in cl], merges=_rows_of(merges))
        want[i] = dict(clusters=rec["out"])
    assert len(recs) >= 3
    return got, want


@case("linkage_average: 1,025 points of the recorded matrices", ["catchhip_linkage_average"])
def _linkage(c, oracle):
    from catch_amd.utils import cluster
    from test_linkage import _cases, _matrix, _merge_rows, _rows_of
    rec = _cases()["size_1025"]
    if "linkage" not in _cache:
        _cache["linkage"] = _matrix(rec)
    dm = _cache["linkage"]
    got, want = {}, {}
    for k in (1, 2):
        t = float.fromhex(rec["thresholds"][k])
        cl, merges = cluster.cluster_hierarchically_on_device(dm, t, ctx=c, return_merges=True)
        got[k] = dict(clusters=cl, merges=_rows_of(merges))
        want[k] = dict(clusters=rec["clusters"][k], merges=_merge_rows(rec["Z"]))
    return got, want


# ------------------------------------------------------------------ the test
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_poisoned_runs_equal_the_plain_run_and_the_model(ctx, oracle, monkeypatch, case):
    from catch_amd import engine
    for k, v in case.hooks.items():
        monkeypatch.setenv(k, v)
    outs, want = {}, None
    for poison in POISONS:
        # (set before the context is created: its first blocks are poisoned too)
        if poison is None:
            monkeypatch.delenv(HOOK, raising=False)
        else:
            monkeypatch.setenv(HOOK, str(poison))
        c = engine.Context(ctx.device)
        try:
            got, model = case.fn(c, oracle)
        finally:
            c.close()
        outs[poison] = got
        if poison is None:
            want = model
    monkeypatch.delenv(HOOK, raising=False)
    plain = outs[None]
    wrong = []                                           # everything that is wrong, in one message
    for key, w in (want or {}).items():
        g = plain[key]
        if isinstance(w, dict) and isinstance(g, dict):          # (a model may speak of a part of an output)
            g = {k: _sub(g[k], w[k]) for k in w}
        if _values(g) != _values(w):
            wrong.append(("the plain run against the model", key))
    for poison in POISONS[1:]:
        bad = _differing(plain, outs[poison])
        if bad:
            wrong.append(("poison %d against the plain run" % poison, bad))
    assert not wrong, (case.name, wrong)


def _sub(g, w):
    return {k: _sub(g[k], w[k]) for k in w} if isinstance(w, dict) and isinstance(g, dict) else g


# ------------------------------------------------------------------ without a GPU: every declared entry has a case
EXEMPT = {
    "catchhip_abi_version": "allocates no device memory",
    "catchhip_last_error": "allocates no device memory",
    "catchhip_device_count": "allocates no device memory",
    "catchhip_ctx_sync": "allocates no device memory",
    "catchhip_pool_stats": "allocates no device memory",
    "catchhip_pool_trim": "allocates no device memory",
    "catchhip_ctx_last_kernel_ms": "allocates no device memory",
    "catchhip_ctx_last_ndf_counters": "allocates no device memory",
    "catchhip_candidates_rebind": "allocates no device memory",
    "catchhip_selftest_candidate_plan": "allocates no device memory",
    "catchhip_pyset_order": "allocates no device memory",
    "catchhip_pyset_order_strs": "allocates no device memory",
    "catchhip_linkage_labels": "allocates no device memory",
    "catchhip_linkage_fits": "allocates no device memory",
    "catchhip_dfs_create": "allocates no device memory",
    "catchhip_dfs_destroy": "allocates no device memory",
    "catchhip_dfs_run": "allocates no device memory",
    "catchhip_dfs_seen": "allocates no device memory",
    "catchhip_dfs_new_queued": "allocates no device memory",
    "catchhip_dfs_set_copy_rank": "allocates no device memory",
    "catchhip_dfs_set_copy_members": "allocates no device memory",
    "catchhip_dfs_push": "allocates no device memory",
    "catchhip_dfs_counts": "allocates no device memory",
    "catchhip_dfs_run_all": "allocates no device memory",
    "catchhip_pyintset_create": "allocates no device memory",
    "catchhip_pyintset_destroy": "allocates no device memory",
    "catchhip_pyintset_isub": "allocates no device memory",
    "catchhip_pyintset_list": "allocates no device memory",
    "catchhip_comm_unique_id": "memory is the communication library's, not the pool's",
    "catchhip_comm_init": "memory is the communication library's, not the pool's",
    "catchhip_comm_destroy": "memory is the communication library's, not the pool's",
    "catchhip_comm_selftest": "memory is the communication library's, not the pool's",
    "catchhip_comm_info": "memory is the communication library's, not the pool's",
    "catchhip_shard_allreduce": "memory is the communication library's, not the pool's",
}
REASONS = ("allocates no device memory", "memory is the communication library's, not the pool's")


def declared_entries():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(catchhip_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_entry_has_a_case_or_a_reason():
    entries = declared_entries()
    assert len(entries) >= 150 and "catchhip_cover_scan" in entries and "catchhip_rows_cover_check" in entries
    named = {}
    for c in CASES:
        for e in c.entries:
            named.setdefault(e, []).append(c.name)
    assert len({c.name for c in CASES}) == len(CASES)
    unknown = sorted((set(named) | set(EXEMPT)) - set(entries))
    assert not unknown, "named by a case or exempt, but not declared in catchhip.h: %s" % unknown
    assert not set(named) & set(EXEMPT), sorted(set(named) & set(EXEMPT))
    assert set(EXEMPT.values()) <= set(REASONS)
    missing = [e for e in entries if e not in named and e not in EXEMPT]
    assert not missing, "entries of catchhip.h without a case in tests/test_poisoned_memory.py: %s" % missing
