"""The bucketed row build (csrc/rows_bucket.inc, host side in csrc/scan.hip: bucket_finish_async, build_rows_radix,
rows_emit) against a sequential merge in NumPy, at every size class, arrival order and merge edge.

Two ways in.  The first half goes through the test entry point catchhip_selftest_row_build
(Context.selftest_row_build), which files hit records the way a producer does -- scattered with ranks, scattered
with compact filing, or grouped with anchor runs -- and calls the build's own functions; the test chooses bucket
sizes, arrival order and what merges, none of which a whole scan lets it choose.  The second half plants a random
100-mer n times in random background, so that a probe gets exactly n hits, and sends that through the scans, the
key-grouped join, cover_ranges, tolerant_bp and the fused filter's direct rows; the expected rows come from the CPU
oracle and, in closed form, from the plant list (extend, clip to the sequence, merge per genome), and the two must
agree before either is used.  All values are integers and every comparison is for equality.

The nine routes of a bucket, the case that reaches each, and why it must:

  odd-even finish   wave buckets (1 .. 512 hits) arriving "sorted", "swapped", "displaced" or with all keys equal:
                    the replay in test_arrival_orders_sit_on_their_side_of_the_round_budget finds a round without
                    a swap inside the budget of 6 / 12 / 32 rounds, so `dirty` is false and no rank sort runs.
  rank sort x 1     the 63- and 64-hit buckets arriving "reversed" or "random": the same replay shows them still
                    out of order after 6 rounds (a reversed bucket of n needs n phases = n / 2 rounds), and
                    n <= 64 picks bucket_rank_sort<64, 1>.
  rank sort x 2     the 65-, 127- and 128-hit buckets, reversed or random: out of order after 12 rounds, 64 < n <= 128.
  rank sort x 8     the 129-, 511- and 512-hit buckets, reversed or random: out of order after 32 rounds
                    (reversed 129 needs 65), n > 128 picks bucket_rank_sort<64, 8>.
  merged runs       test_grouped_runs: grouped records with run counts that sum to the bucket (sizes 2, 65, 129 and
                    512 and random ones), 1 .. 5 runs; `merged_runs` sets the round budget to 0 and skips the
                    rank sort, so a wrong rank from the binary search is a wrong table.
  workgroup 1,024   buckets of 513, 1,023 and 1,024 hits: above BK_SMALL the wave kernel skips them
                    (n > CAP) and only the launch with lo = 512 < n <= cap = 1,024 lists them.
  workgroup 2,048   buckets of 1,025, 2,047 and 2,048 hits (lo = 1,024, cap = 2,048).
  workgroup 4,096   buckets of 2,049, 4,095 and 4,096 hits (lo = 2,048, cap = 4,096).
  workgroup 8,192   buckets of 4,097, 8,191 and 8,192 hits (lo = 4,096, cap = 8,192 = BK_BIG).
  radix             test_bucket_past_the_workgroup_takes_the_radix_build: one bucket of 8,193 hits; every
                    workgroup launch passes it over, the cap-8,192 one raises the overflow flag, and the callers'
                    rule (radix iff overflow) then builds the table by sorting.  The radix build forced on the
                    size table must give the bucketed build's rows.

test_every_size_class_has_its_edges holds the arithmetic of the class borders, the branch-point test the arithmetic of
the round budget; both read the constants from the source.
"""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BK_SMALL, BK_BIG, BK_RUNS_MAX = 512, 8192, 5
ROUND_BUDGET = ((64, 6), (128, 12), (BK_SMALL, 32))      # buckets up to n hits: rounds of odd-even transposition
SCAN1_MAX = 16384                                        # bucket_scan: one workgroup up to here, tiles above
SCT_TILE = 4096
EMIT_WINDOW = 257                                        # rows_emit_kernel: offsets staged per 256-row block
# (lo, cap] per route of bucket_merge_kernel<64, 512> and the four launches of bucket_merge_big_kernel
SIZE_CLASSES = ((0, 64), (64, 128), (128, 512), (512, 1024), (1024, 2048), (2048, 4096), (4096, 8192))
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
         8191, 8192)
SEGLEN = 1 << 23                                         # the segments of the coordinate space: 4 of 8 Mbases
BOUNDS = np.arange(5, dtype=np.int64) * SEGLEN

NEARLY_SORTED = ("sorted", "swapped", "displaced")
SCRAMBLED = ("reversed", "random")
ORDERS = NEARLY_SORTED + SCRAMBLED
PATTERNS = ("none", "all", "gaps", "swallow", "span3", "segs", "equal", "random")


# ------------------------------------------------------------------ reference
def reference(hits, nb, dedupe=False, bucket_set=None):
    """The row table of hit records {start, end, segment, bucket}, whatever their order.  Per bucket: stable sort by
    (start, end), then one pass: a record joins the row in progress iff it has the same segment and start <= the
    row's end, whose end is the running maximum; in dedupe mode equal (start, end) collapse and nothing merges."""
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 4)
    order = np.lexsort((h[:, 1], h[:, 0], h[:, 3]))
    rows, cur = [], None
    for s, e, g, b in h[order].tolist():
        if cur is not None and cur[0] == b:
            assert g >= cur[1], "a bucket's segments must not decrease with start"
            if dedupe:
                if cur[2] == s and cur[3] == e:
                    continue
            elif cur[1] == g and s <= cur[3]:
                cur[3] = max(cur[3], e)
                continue
        if cur is not None:
            rows.append(cur)
        cur = [b, g, s, e]
    if cur is not None:
        rows.append(cur)
    r = np.array(rows, dtype=np.int64).reshape(-1, 4)
    length = r[:, 3] - r[:, 2]
    mcnt = np.bincount(r[:, 0], minlength=nb)
    blmax, bsum = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    np.maximum.at(blmax, r[:, 0], length)
    np.add.at(bsum, r[:, 0], length)
    sets = r[:, 0] if bucket_set is None else np.asarray(bucket_set, dtype=np.int64)[r[:, 0]]
    t = np.lexsort((r[:, 2], r[:, 1], sets))                # the table: by (set, segment, start)
    return {"set": sets[t], "seg": r[t, 1], "start": r[t, 2], "end": r[t, 3], "mcnt": mcnt, "blmax": blmax,
            "bsum": bsum, "lmax": int(length.max()) if len(rows) else 0, "rows": len(rows), "hits": h.shape[0],
            "bucket_rows": r}      # (bucket, segment, start, end), a bucket's rows together and in start order


def test_reference_on_a_case_written_down_by_hand():
    hits = [  # start, end, segment, bucket -- in no order
        (30, 40, 0, 1), (10, 20, 0, 1), (20, 25, 0, 1),        # bucket 1: 10-20 touches 20-25; 30-40 stands alone
        (100, 200, 0, 3), (150, 160, 0, 3), (190, 260, 0, 3),  # bucket 3: 150-160 lies inside; 190 <= 200, the max
        (261, 270, 0, 3),                                      # ... one base past 260: a row of its own
        (500, 600, 0, 4), (600, 700, 1, 4),                    # bucket 4: touching, but two segments
        (5, 9, 0, 5), (5, 9, 0, 5), (5, 7, 0, 5)]              # bucket 5: equal records and a shorter one
    ref = reference(hits, 6)
    assert list(zip(ref["set"], ref["seg"], ref["start"], ref["end"])) == [
        (1, 0, 10, 25), (1, 0, 30, 40), (3, 0, 100, 260), (3, 0, 261, 270), (4, 0, 500, 600), (4, 1, 600, 700),
        (5, 0, 5, 9)]
    assert ref["mcnt"].tolist() == [0, 2, 0, 2, 2, 1] and ref["blmax"].tolist() == [0, 15, 0, 160, 100, 4]
    assert ref["bsum"].tolist() == [0, 25, 0, 169, 200, 4] and ref["lmax"] == 160 and ref["rows"] == 7
    ded = reference(hits, 6, dedupe=True, bucket_set=[10, 11, 12, 13, 14, 15])
    assert list(zip(ded["set"], ded["seg"], ded["start"], ded["end"])) == [
        (11, 0, 10, 20), (11, 0, 20, 25), (11, 0, 30, 40), (13, 0, 100, 200), (13, 0, 150, 160), (13, 0, 190, 260),
        (13, 0, 261, 270), (14, 0, 500, 600), (14, 1, 600, 700), (15, 0, 5, 7), (15, 0, 5, 9)]
    assert ded["mcnt"].tolist() == [0, 3, 0, 4, 2, 2] and ded["lmax"] == 100 and ded["bsum"][5] == 6
    with pytest.raises(AssertionError):
        reference([(10, 20, 1, 0), (30, 40, 0, 0)], 1)
    assert reference([], 3)["rows"] == 0 and reference([], 3)["mcnt"].tolist() == [0, 0, 0]


# ------------------------------------------------------------------ buckets
def make_bucket(n, pattern, seed=0):
    """n records (start, end, segment) sorted by (start, end); the segment is the one BOUNDS gives the start."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "none":                  # 100 bases every 200: nothing merges
        start = 1000 + 200 * i
        end = start + 100
    elif pattern == "all":                 # 100 bases every 50: one row
        start = 1000 + 50 * i
        end = start + 100
    elif pattern == "gaps":                # touching exactly, one base apart, overlapping by 10, and again
        step = 100 + np.array([0, 1, -10], dtype=np.int64)[i % 3]
        start = 1000 + np.concatenate(([0], np.cumsum(step[:-1]))) if n else i
        end = start + 100
    elif pattern == "swallow":             # every 97th record swallows the next 70, which do not touch each other:
        blk, j = i // 97, i % 97           # the running maximum, not the previous end, joins them; 71 .. 96 stand alone
        start = 1000 + 2910 * blk + 30 * j
        end = start + np.where(j == 0, 2115, 10)
    elif pattern == "span3":               # chains of 150 records: head in chunk c, last item in chunk c + 2
        start = 1000 + 50 * i + 1000 * (i // 150)
        end = start + 100
    elif pattern == "segs":                # a segment border between items 63 | 64 (short buckets: in the middle),
        split = 64 if n > 64 else n // 2   # the records touch all along -- and across the border, where they must not merge
        start = SEGLEN + 100 * (i - split)
        end = start + 100
    elif pattern == "equal":
        start = np.full(n, 1000, dtype=np.int64)
        end = start + 100
    elif pattern == "random":
        rng = np.random.default_rng(1000 * n + seed)
        start = np.sort(rng.integers(1000, 1000 + 60 * max(n, 1), size=n))
        end = start + rng.integers(1, 121, size=n)
        o = np.lexsort((end, start))
        start, end = start[o], end[o]
    else:
        raise AssertionError(pattern)
    seg = start // SEGLEN
    assert n == 0 or (end <= BOUNDS[seg + 1]).all()         # clipped to its segment, as a producer leaves it
    return np.stack([start, end, seg], axis=1).reshape(n, 3)


def arrival(n, order, seed=0):
    """perm[k] = the sorted position of the k-th record to arrive."""
    p = np.arange(n)
    if order == "swapped":                 # neighbours swapped all along
        p = p ^ 1
        if n & 1:
            p[-1] = n - 1
    elif order == "displaced":             # one record five places early
        if n > 6:
            k = n // 2
            p = np.concatenate((p[:k - 5], [k], p[k - 5:k], p[k + 1:]))
    elif order == "reversed":
        p = p[::-1].copy()
    elif order == "random":
        p = np.random.default_rng(77 * n + seed).permutation(n)
    else:
        assert order == "sorted"
    assert np.array_equal(np.sort(p), np.arange(n))
    return p


def file_hits(buckets, seed=0):
    """(n, 4) hit records in arrival order from per-bucket record arrays (each in ITS arrival order): the buckets'
    arrivals interleaved at random, every bucket's own order kept."""
    sizes = np.array([len(b) for b in buckets], dtype=np.int64)
    cat = np.concatenate([np.concatenate((b, np.full((len(b), 1), k, dtype=np.int64)), axis=1)
                          for k, b in enumerate(buckets)] + [np.zeros((0, 4), dtype=np.int64)])
    labels = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(buckets)), sizes))
    out = np.zeros_like(cat)
    out[np.argsort(labels, kind="stable")] = cat
    return out


def size_table(pattern, order, sizes=SIZES):
    """One bucket per size, empty buckets first, last and after every third; (hits in arrival order, nb)."""
    buckets = [np.zeros((0, 3), dtype=np.int64)] * 2
    for k, n in enumerate(sizes):
        buckets.append(make_bucket(n, pattern, k)[arrival(n, order, k)])
        if k % 3 == 2:
            buckets.append(np.zeros((0, 3), dtype=np.int64))
    buckets.append(np.zeros((0, 3), dtype=np.int64))
    return file_hits(buckets, len(pattern)), len(buckets)


def oddeven_clean_round(keys, budget):
    """The odd-even transposition rounds of bucket_merge_kernel on 64-bit keys in arrival order: the number of the
    first round without a swap if there is one among the first `budget` (the bucket is then sorted and no rank sort
    runs), else None."""
    a = np.array(keys, dtype=np.uint64)
    for rnd in range(1, budget + 1):
        swapped = False
        for ph in (0, 1):
            j = np.arange(ph, a.size - 1, 2)
            m = a[j] > a[j + 1]
            if m.any():
                lo, hi = a[j[m]].copy(), a[j[m] + 1].copy()
                a[j[m]], a[j[m] + 1] = hi, lo
                swapped = True
        if not swapped:
            assert (a[:-1] <= a[1:]).all()
            return rnd
    return None


def round_budget(n):
    return next(r for cap, r in ROUND_BUDGET if n <= cap)


# ------------------------------------------------------------------ without a GPU
def test_entry_point_declared_bound_and_wrapped_and_the_constants_stand():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    scan = open(os.path.join(REPO, "catch_amd", "csrc", "scan.hip")).read()
    inc = open(os.path.join(REPO, "catch_amd", "csrc", "rows_bucket.inc")).read()
    name = "catchhip_selftest_row_build"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert re.search(r'extern "C" int %s\s*\(' % name, scan)
    assert name in _lib.PROTOTYPES and callable(engine.Context.selftest_row_build)
    assert len(_lib.PROTOTYPES[name][1]) == 25
    # the entry point calls the product's functions, and the radix form its two kernels
    body = scan[scan.index('extern "C" int %s' % name):]
    body = body[:body.index('\nextern "C"', 10)]
    for callee in ("bucket_prepare(", "bucket_finish_async(", "rows_emit(", "build_rows_radix(", "rows_compact_kernel"):
        assert callee in body, callee
    assert "rows_merge_kernel" in scan[scan.index("static int build_rows_radix"):scan.index("struct ScanOut")]
    # the structural constants this file is written around
    assert re.search(r"#define BK_SMALL %d\b" % BK_SMALL, inc) and re.search(r"#define BK_BIG %d\b" % BK_BIG, inc)
    assert re.search(r"#define BK_RUNS_MAX %d\b" % BK_RUNS_MAX, inc)
    assert "n <= (u32)THREADS ? 6 : n <= 2u * THREADS ? 12 : 32" in inc and "bucket_merge_kernel<64, BK_SMALL>" in scan
    assert [r for _, r in ROUND_BUDGET] == [6, 12, 32]
    assert re.search(r"if \(n <= %d\) \{\s*hipLaunchKernelGGL\(scan1_kernel" % SCAN1_MAX, scan)
    assert re.search(r"#define SCT_THREADS 256\b", inc) and re.search(r"#define SCT_IPT 16\b", inc) and SCT_TILE == 256 * 16
    assert "s_rs[%d]" % EMIT_WINDOW in inc and "q < %d" % EMIT_WINDOW in inc
    assert "for (u32 cap = 1024; cap <= (u32)BK_BIG; cap <<= 1)" in scan
    assert "if (n > (u32)CAP) continue;" in inc and "n > lo && n <= cap" in inc


def test_every_size_class_has_its_edges():
    """Every route's size class (lo, cap] holds a bucket at lo + 1 and at cap, and the one below its lower border."""
    assert [c for _, c in SIZE_CLASSES[3:]] == [1024 << k for k in range(4)] and SIZE_CLASSES[-1][1] == BK_BIG
    assert SIZE_CLASSES[2][1] == BK_SMALL
    for lo, cap in SIZE_CLASSES:
        assert lo + 1 in SIZES and cap in SIZES and lo in SIZES, (lo, cap)
    assert max(SIZES) == BK_BIG and BK_BIG + 1 not in SIZES    # 8,193 goes in a build of its own
    # the 23 sizes fit one build of a few tens of thousands of records
    assert len(SIZES) == 23 and sum(SIZES) < 50000
    # the merge patterns do what their names say, at a size that straddles two chunk borders
    for pattern, rows in (("none", 150), ("all", 1), ("gaps", 51), ("swallow", 1 + 26 + 1), ("span3", 1), ("segs", 2),
                          ("equal", 1)):
        ref = reference(file_hits([make_bucket(150, pattern)]), 1)
        assert ref["rows"] == rows, (pattern, ref["rows"])
    sw = make_bucket(150, "swallow")
    assert sw[70, 0] > sw[69, 1] and sw[70, 0] <= sw[0, 1] < sw[71, 0]   # only the running maximum joins item 70
    sg = make_bucket(150, "segs")
    assert sg[63, 2] == 0 and sg[64, 2] == 1 and sg[63, 1] == sg[64, 0] == SEGLEN
    sp = reference(file_hits([make_bucket(400, "span3")]), 1)
    assert sp["rows"] == 3 and sp["lmax"] == 50 * 149 + 100


def test_arrival_orders_sit_on_their_side_of_the_round_budget():
    """Which sort a wave bucket takes depends on how it arrives.  A replay of the kernel's odd-even rounds: every
    nearly sorted order finishes inside the budget of its size (no rank sort), every scrambled order does not (rank
    sort at 1, 2 or 8 items per thread), at every wave size large enough to be out of order at all."""
    for n in (s for s in SIZES if 0 < s <= BK_SMALL):
        b = make_bucket(n, "none")
        keys = (b[:, 0].astype(np.uint64) << np.uint64(32)) | b[:, 1].astype(np.uint64)
        budget = round_budget(n)
        assert budget == (6 if n <= 64 else 12 if n <= 128 else 32)
        for order in NEARLY_SORTED:
            rnd = oddeven_clean_round(keys[arrival(n, order)], budget)
            assert rnd is not None and rnd <= {"sorted": 1, "swapped": 2, "displaced": 4}[order], (n, order, rnd)
        if n >= 63:
            for order in SCRAMBLED:
                assert oddeven_clean_round(keys[arrival(n, order)], budget) is None, (n, order)
            # a reversed bucket of n needs n phases = n / 2 rounds, and one more to see no swap
            assert oddeven_clean_round(keys[arrival(n, "reversed")], n) == (n + 1) // 2 + 1
            assert (n + 1) // 2 + 1 > budget
        # all keys equal: nothing ever swaps
        e = make_bucket(n, "equal")
        assert oddeven_clean_round((e[:, 0].astype(np.uint64) << np.uint64(32)) | e[:, 1].astype(np.uint64), budget) == 1
    assert oddeven_clean_round(np.arange(512, dtype=np.uint64)[::-1], 600) == 257 and round_budget(512) == 32
    # the rank sort's items per thread: 1 up to 64, 2 up to 128, 8 = BK_SMALL / 64 above
    assert [(63, 1), (64, 1), (65, 2), (128, 2), (129, 8), (512, 8)] == [
        (n, 1 if n <= 64 else 2 if n <= 128 else BK_SMALL // 64) for n in (63, 64, 65, 128, 129, 512)]


# ------------------------------------------------------------------ on the device, through the entry point
_REF = {}


def ref_of(key, hits, nb, **kw):
    """One reference per table, shared by the tests that file it in different orders and forms (the reference does
    not depend on the arrival order)."""
    if key not in _REF:
        _REF[key] = reference(hits, nb, **kw)
    return _REF[key]


def check(out, ref, what, slots=True):
    assert (out["hits"], out["rows"], out["lmax"]) == (ref["hits"], ref["rows"], ref["lmax"]), \
        (what, out["hits"], out["rows"], out["lmax"], ref["hits"], ref["rows"], ref["lmax"])
    for k in ("set", "seg", "start", "end"):
        bad = np.nonzero(out[k].astype(np.int64) != ref[k])[0]
        assert bad.size == 0, (what, k, bad[:5].tolist(), out[k][bad[:5]].tolist(), ref[k][bad[:5]].tolist())
    if not slots:
        return
    assert not out["overflow"], what
    for k in ("mcnt", "blmax", "bsum"):
        if out[k] is not None:
            bad = np.nonzero(out[k].astype(np.int64) != ref[k])[0]
            assert bad.size == 0, (what, k, bad[:5].tolist(), out[k][bad[:5]].tolist(), ref[k][bad[:5]].tolist())
    # the slot rule of the direct rows: slot i carries the bucket whose [bstart, bstart + n) holds it, and the slots
    # with i - bstart[w] < mcnt[w] are the bucket's rows in start order
    S, bstart = out["S"].astype(np.int64), out["bstart"].astype(np.int64)
    nb = ref["mcnt"].size
    assert bstart[0] == 0 and bstart[nb] == ref["hits"] and (np.diff(bstart) >= 0).all(), what
    slot = np.arange(S.shape[0])
    assert np.array_equal(S[:, 3], np.searchsorted(bstart, slot, side="right") - 1), what
    is_row = slot - bstart[S[:, 3]] < ref["mcnt"][S[:, 3]]
    got = S[is_row][:, [3, 2, 0, 1]]
    assert np.array_equal(got, ref["bucket_rows"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sizes_orders_and_merge_patterns(ctx, pattern):
    """All 23 sizes in one build, empty buckets first, last and between, per merge pattern; every arrival order;
    scattered, compactly filed and grouped (without runs: the grouped producers' buckets take the same sorts)."""
    for order in ORDERS:
        hits, nb = size_table(pattern, order)
        ref = ref_of(("sizes", pattern), hits, nb)
        n = hits.shape[0]
        assert n == sum(SIZES)
        if pattern == "none":
            assert ref["rows"] == n                       # nothing merged: the emit is the plain transform
        forms = [("scattered", {})]
        if order in ("sorted", "random"):
            rng = np.random.default_rng(3)
            wave = []
            while sum(wave) < n:
                wave.append(min(n - sum(wave), int(rng.choice([0, 1, 15, 63, 64]))))
            forms += [("scattered", {"hit_slots": np.cumsum(rng.integers(1, 4, size=n)) - 1}),
                      ("compact", {"wave_hits": wave}), ("grouped", {})]
        for form, kw in forms:
            for emit in ("host", "device"):
                out = ctx.selftest_row_build(hits, nb, form=form, emit=emit, **kw)
                check(out, ref, (pattern, order, form, emit))
    out = ctx.selftest_row_build(hits, nb, want_sum=False)
    assert out["bsum"] is None
    check(out, ref, (pattern, "no sums"))


@pytest.mark.gpu
def test_bucket_past_the_workgroup_takes_the_radix_build(ctx):
    """8,193 hits in one bucket: the bucketed build raises the overflow flag and leaves that bucket out (the others
    are still right); the radix build the callers then take gives the reference.  Forced on the size tables, the
    radix build gives the rows of the bucketed build, with and without a bucket -> set table."""
    for pattern in ("gaps", "segs", "swallow"):
        big = make_bucket(BK_BIG + 1, pattern)[arrival(BK_BIG + 1, "random")]
        small = [make_bucket(n, pattern)[arrival(n, "reversed")] for n in (0, 65, 700, 0)]
        hits = file_hits([small[0], small[1], big, small[2], small[3]], 5)
        ref = reference(hits, 5)
        out = ctx.selftest_row_build(hits, 5, bounds=BOUNDS)
        assert out["overflow"] and not out["radix"] and out["hits"] == hits.shape[0]
        assert out["mcnt"].tolist() == [0, ref["mcnt"][1], 0, ref["mcnt"][3], 0]      # the overflowed bucket: no rows
        assert out["rows"] == ref["mcnt"][1] + ref["mcnt"][3]
        out = ctx.selftest_row_build(hits, 5, bounds=BOUNDS, build="radix_if_overflow")
        assert out["overflow"] and out["radix"]
        check(out, ref, (pattern, "8193"), slots=False)
        sets = [2, 3, 7, 11, 4000]
        out = ctx.selftest_row_build(hits, 5, bounds=BOUNDS, build="radix_if_overflow", bucket_set=sets)
        check(out, reference(hits, 5, bucket_set=sets), (pattern, "8193 with sets"), slots=False)
    for pattern in ("none", "gaps", "segs", "random"):
        hits, nb = size_table(pattern, "random")
        ref = ref_of(("sizes", pattern), hits, nb)
        out = ctx.selftest_row_build(hits, nb, bounds=BOUNDS, build="radix_if_overflow")
        assert not out["radix"] and not out["overflow"]
        check(out, ref, (pattern, "no overflow"))
        out = ctx.selftest_row_build(hits, nb, bounds=BOUNDS, build="radix", form="compact",
                                     wave_hits=[64] * (hits.shape[0] // 64) + [hits.shape[0] % 64])
        assert out["radix"] and not out["overflow"]
        check(out, ref, (pattern, "radix forced"), slots=False)


@pytest.mark.gpu
def test_dedupe_walk(ctx):
    """cover_ranges' mode: equal (start, end) collapse, nothing merges.  Duplicates adjacent, across items 63 | 64
    and (grouped) across runs, in a wave bucket and in a bucket of the 4,096 class."""
    for n in (100, 3000):
        b = make_bucket(n, "gaps")                       # would merge in threes: here it must not
        short = b[20:23] - np.array([0, 7, 0])           # the same starts with other ends: ranges of their own
        dup = np.concatenate((b, b[10:12], b[10:11], b[56:57], b[n - 1:], b[0:1], short))
        dup = dup[np.lexsort((dup[:, 1], dup[:, 0]))]
        assert (dup[63] == dup[64]).all() and (dup[0] == dup[1]).all() and (dup[-1] == dup[-2]).all()
        assert dup[24, 0] == dup[25, 0] and dup[24, 1] + 7 == dup[25, 1]
        for order in ("sorted", "reversed", "random"):
            hits = file_hits([np.zeros((0, 3), dtype=np.int64), dup[arrival(len(dup), order)], make_bucket(5, "equal")])
            ref = ref_of(("dedupe", n), hits, 3, dedupe=True)
            assert ref["mcnt"].tolist() == [0, n + 3, 1]
            for form in ("scattered", "grouped"):
                check(ctx.selftest_row_build(hits, 3, form=form, dedupe=True), ref, ("dedupe", n, order, form))
        # across runs: every run holds every record once
        runs = 3
        hits = file_hits([np.concatenate([b] * runs)])
        if n <= BK_SMALL // runs:
            out = ctx.selftest_row_build(hits, 1, form="grouped", dedupe=True, run_cnt=[[n] * runs], nruns=runs)
            check(out, reference(hits, 1, dedupe=True), ("dedupe runs", n))
            assert out["rows"] == n


def _split_into_runs(b, run_of):
    """The sorted records b dealt to runs (run_of[i] = the run of record i): the bucket as the join leaves it, run
    after run, each in (start, end) order; and the run lengths."""
    nr = int(run_of.max()) + 1 if len(run_of) else 1
    o = np.argsort(run_of, kind="stable")
    return b[o], np.bincount(run_of, minlength=nr)


@pytest.mark.gpu
def test_grouped_runs(ctx):
    """The rank-by-binary-search merge of up to 5 sorted runs: 1 .. 5 runs, empty runs first, in the middle and
    last, equal keys in different runs, sizes 2, 65, 129 and 512 merged by runs, 513 handed to the workgroup
    kernel, and run counts that do not sum to the bucket (the fall-back to the sorts)."""
    rng = np.random.default_rng(11)
    for nruns in range(1, BK_RUNS_MAX + 1):
        for empty in (None, 0, nruns // 2, nruns - 1):
            if empty is not None and (nruns == 1 or (empty == nruns // 2 and empty in (0, nruns - 1))):
                continue
            buckets, cnts = [], []
            for n, pattern in ((2, "none"), (65, "gaps"), (129, "swallow"), (512, "random"), (0, "none"),
                               (300, "equal"), (200, "segs"), (513, "gaps"), (1, "none"), (140, "span3")):
                b = make_bucket(n, pattern)
                live = [a for a in range(nruns) if a != empty]
                run_of = np.asarray(rng.choice(live, size=n), dtype=np.int64)
                if n == 2 and len(live) > 1:
                    run_of = np.array([live[-1], live[0]])         # the later record in the earlier run
                recs, c = _split_into_runs(b, run_of)
                buckets.append(recs)
                cnts.append(np.concatenate((c, np.zeros(BK_RUNS_MAX + 1 - len(c), dtype=np.int64))))
            hits = file_hits(buckets, 0)
            # (file_hits interleaves the buckets and keeps each one's order: grouped, a bucket is its runs side by side)
            nb = len(buckets)
            ref = ref_of(("runs",), hits, nb)
            stride = nruns + (nruns & 1)                           # the row stride is the caller's, not nruns
            run_cnt = np.array(cnts)[:, :stride]
            out = ctx.selftest_row_build(hits, nb, form="grouped", run_cnt=run_cnt, nruns=nruns)
            check(out, ref, ("runs", nruns, empty))
            # counts that do not sum to their bucket: that bucket is sorted the other way, the rest by runs
            wrong = run_cnt.copy()
            wrong[3, 0] += 1
            wrong[1, nruns - 1] = 0 if run_cnt[1, nruns - 1] else 1
            out = ctx.selftest_row_build(hits, nb, form="grouped", run_cnt=wrong, nruns=nruns)
            check(out, ref, ("runs with wrong counts", nruns, empty))
    # equal keys in different runs: two runs hold the same records
    b = make_bucket(200, "gaps")
    hits = file_hits([np.concatenate((b, b))])
    out = ctx.selftest_row_build(hits, 1, form="grouped", run_cnt=[[200, 200]], nruns=2)
    check(out, reference(hits, 1), "equal keys in two runs")


def _many_buckets(nb, longest_in, seed):
    """nb buckets of 0 .. 3 hits, some merging, and one bucket whose row is the longest of the table."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 4, size=nb)
    cnt[longest_in] = 3
    b = np.repeat(np.arange(nb, dtype=np.int64), cnt)
    j = np.arange(b.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    start = 1000 + b % 7 + 150 * j
    end = start + np.where(b % 5 == 0, 160, 100)            # every fifth bucket merges into one row
    end[b == longest_in] += 333                             # one row of 150 * 2 + 433 or more
    hits = np.stack([start, end, np.zeros_like(b), b], axis=1)
    return hits[rng.permutation(b.size)]


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 1024, SCAN1_MAX, SCAN1_MAX + 1])
def test_bucket_counts_around_the_scan_threshold(ctx, nb):
    """scan1_kernel up to 16,384 buckets, the tiled scan above: offsets, row numbers and the longest row."""
    hits = _many_buckets(nb, nb // 3, nb)
    ref = reference(hits, nb)
    assert ref["lmax"] >= 733 and ref["blmax"][nb // 3] == ref["lmax"] and (np.delete(ref["blmax"], nb // 3) < 733).all()
    for emit in ("host", "device"):
        check(ctx.selftest_row_build(hits, nb, emit=emit), ref, (nb, emit))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first bucket", "last bucket", "last tile", "end of a tile", "start of a tile",
                                   "middle of a tile"])
def test_tiled_scan_carries_the_longest_row(ctx, where):
    """More than two scan tiles past the threshold, the last tile partly filled; the longest row of the table in the
    first bucket, in the last bucket, in the first bucket of the last tile, and at the end, the start and the middle
    of a tile in between -- a wrong longest row chooses the wrong solver family without a wrong row anywhere."""
    nb = SCAN1_MAX + 2 * SCT_TILE + 37
    assert nb > SCAN1_MAX and nb % SCT_TILE not in (0, 1)
    at = {"first bucket": 0, "last bucket": nb - 1, "last tile": (nb // SCT_TILE) * SCT_TILE,
          "end of a tile": 3 * SCT_TILE - 1, "start of a tile": 2 * SCT_TILE, "middle of a tile": SCT_TILE + 2345}[where]
    hits = _many_buckets(nb, at, 5)
    ref = reference(hits, nb)
    assert int(np.argmax(ref["blmax"])) == at and (np.delete(ref["blmax"], at) < ref["lmax"]).all()
    out = ctx.selftest_row_build(hits, nb)
    check(out, ref, where)
    assert out["lmax"] == ref["lmax"] >= 733


@pytest.mark.gpu
def test_emit_forms(ctx):
    """rows_emit's three forms: the plain transform when nothing merged (known to the host, and found on the
    device), the staged-window search, and the full search behind a stretch of 300 empty buckets inside one 256-row
    block; with and without a bucket -> set table."""
    empty = np.zeros((0, 3), dtype=np.int64)
    for merging in (False, True):
        pattern = "gaps" if merging else "none"
        buckets = [make_bucket(30, pattern)[arrival(30, "random")] for _ in range(10)]      # 110 or 300 rows, then
        buckets += [empty] * 300                                                          # ... 300 empty buckets
        buckets += [make_bucket(n, pattern)[arrival(n, "swapped")] for n in (3, 700, 0, 40, 1)]
        buckets += [empty] * 260 + [make_bucket(9, pattern)]
        hits, nb = file_hits(buckets, 2), len(buckets)
        sets = 3 * np.arange(nb) + 1
        for bucket_set in (None, sets):
            ref = reference(hits, nb, bucket_set=bucket_set)
            assert (ref["rows"] == ref["hits"]) == (not merging)
            if merging:
                # the last rows of the first block lie behind the empty stretch: more than 256 buckets from its first
                rstart = np.concatenate(([0], np.cumsum(ref["mcnt"])))
                assert rstart[10] == rstart[310] < 256 < rstart[312] and rstart[256] == rstart[10]
            for emit in ("host", "device"):
                out = ctx.selftest_row_build(hits, nb, bucket_set=bucket_set, emit=emit)
                check(out, ref, ("emit", merging, bucket_set is not None, emit))
    # no hits at all
    out = ctx.selftest_row_build(np.zeros((0, 4), dtype=np.int64), 7)
    assert (out["hits"], out["rows"], out["lmax"]) == (0, 0, 0) and not out["mcnt"].any()


@pytest.mark.gpu
def test_entry_point_refuses_indices_that_point_outside(ctx):
    """The entry point looks at the caller's indices before anything reaches the device."""
    hits = file_hits([make_bucket(5, "none")])
    with pytest.raises(ValueError):
        ctx.selftest_row_build(hits, 0)
    with pytest.raises(ValueError, match="invalid argument"):
        ctx.selftest_row_build(hits, 1, build="radix")             # no segment bounds
    with pytest.raises(ValueError, match="invalid argument"):
        ctx.selftest_row_build(hits, 1, build="radix", bounds=[0, 1500])   # a start past the last bound
    with pytest.raises(ValueError, match="invalid argument"):
        ctx.selftest_row_build(hits, 1, form="grouped", run_cnt=[[5] * 6], nruns=6)
    check(ctx.selftest_row_build(hits, 1), reference(hits, 1), "after the refusals")


# ------------------------------------------------------------------ the producers at the same edges: whole scans
# A random 100-mer planted n times in random background gives its probe exactly n hits, and the rows follow from the
# plant list: extend, clip to the sequence, merge per genome.
PL, PM, PEXT = 100, 2, 20
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CASES = {}


def _dna(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)]


def model_rows(plants, glen, ext, merge=True, plen=PL):
    """The closed form: plants = [(probe, genome, offset)], one sequence per genome.  Rows (probe, genome, start,
    end) sorted; merge=False: the distinct extended ranges."""
    ranges = sorted((p, g, max(0, x - ext), min(glen[g], x + plen + ext)) for p, g, x in plants)
    if not merge:
        return sorted(set(ranges))
    rows = []
    for p, g, s, e in ranges:
        if rows and rows[-1][0] == p and rows[-1][1] == g and s <= rows[-1][3]:
            rows[-1][3] = max(rows[-1][3], e)
        else:
            rows.append([p, g, s, e])
    return [tuple(r) for r in rows]


def plant_case(key, counts, ext=PEXT, mutate_runs=0, pairs=False, seed=1):
    """Probes, two genomes (one sequence each) and the plant list.  Probe p stands counts[p] times: the first two
    thirds in genome 0, the rest in genome 1, the gaps between its copies cycling through 2 ext (the extended ranges
    touch), 2 ext + 1 (one base apart) and 2 ext - 10 (they overlap); the first copy of a genome lies 7 bases in (its
    range is clipped at the start; 50 with pairs) and the last ends flush with the genome's end.
    mutate_runs = r > 0: copy j carries one changed base inside each of the probe's first j mod r anchors (positions
    from the probe's anchor table at r - 1 mismatches), so that the first anchor to match exactly -- the run the
    key-grouped join files the hit in -- goes round all r.
    pairs: the copies stand as tandem pairs (two copies back to back), the pairs 30 bases apart -- the same 30 bases
    every time, so that the windows of a candidate grid over the pairs are few and the oracle stays quick -- and
    10,000 bases of plain background close each genome."""
    if key in _CASES:
        return _CASES[key]
    from catch_amd import probe as probe_mod
    rng = np.random.default_rng(seed)
    probes = [_dna(rng, PL) for _ in counts]
    spacers = [_dna(rng, 30) for _ in counts] if pairs else None
    strs = [p.tobytes().decode() for p in probes]
    anchors = None
    if mutate_runs:
        k, uniq, _, ep, eo = probe_mod.anchor_table(strs, mutate_runs - 1, PL)
        assert uniq == strs
        anchors = [sorted(int(o) for q, o in zip(ep, eo) if q == p)[:mutate_runs] for p in range(len(strs))]
        assert all(len(a) == mutate_runs for a in anchors), (k, anchors[0])
    gaps = (2 * ext, 2 * ext + 1, max(2 * ext - 10, 1))
    parts, plants, glen = [[], []], [], [0, 0]
    for g in (0, 1):
        pos = 0

        def put(a):
            nonlocal pos
            parts[g].append(a)
            pos += len(a)
        put(_dna(rng, 50 if pairs else 7))                  # (pairs: the first copy is a window of a stride-50 grid)
        for p, n in enumerate(counts):
            n0 = n - n // 3
            mine = range(0, n0) if g == 0 else range(n0, n)
            for j in mine:
                copy = probes[p].copy()
                if mutate_runs:
                    for a in anchors[p][:j % mutate_runs]:
                        at = a + int(rng.integers(0, k))
                        copy[at] = _ACGT[(int(np.nonzero(_ACGT == copy[at])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
                plants.append((p, g, pos))
                put(copy)
                if pairs:
                    put(spacers[p] if j & 1 or j == mine[-1] else spacers[p][:0])
                else:
                    put(_dna(rng, gaps[j % 3]))
            if len(mine):
                put(_dna(rng, 2 * ext + 50))
        if pairs:
            put(_dna(rng, 10000))                           # plain background: candidates with one hit each
        seq = np.concatenate(parts[g])
        if not pairs:                                       # the last copy of the genome ends flush with it
            seq = seq[:max(x for _, gg, x in plants if gg == g) + PL]
        parts[g], glen[g] = seq, len(seq)
    genomes = [[parts[0].tobytes().decode()], [parts[1].tobytes().decode()]]
    _CASES[key] = {"probes": strs, "genomes": genomes, "plants": plants, "glen": glen, "ext": ext,
                   "counts": list(counts)}
    return _CASES[key]


def _expected(oracle, case, m=PM):
    """The oracle's rows of a plant case -- which must be the closed form's."""
    import test_gpu_parity as gp
    if ("rows", m) not in case:
        exp = gp._oracle_rows(oracle, case["probes"], case["genomes"], m, PL, 0, case["ext"])
        assert exp == model_rows(case["plants"], case["glen"], case["ext"])
        hits = np.bincount([p for p, _, _ in case["plants"]], minlength=len(case["counts"]))
        assert hits.tolist() == case["counts"]
        case[("rows", m)] = exp
    return case[("rows", m)]


def _rows0(oracle, case, m):
    """The oracle's rows per sequence at extension 0 (what tolerant_bp sums) -- and the closed form's."""
    import test_gpu_parity as gp
    if ("rows0", m) not in case:
        exp = gp._oracle_rows(oracle, case["probes"], [[s] for g in case["genomes"] for s in g], m, PL, 0, 0)
        assert exp == model_rows(case["plants"], case["glen"], 0)
        case[("rows0", m)] = exp
    return case[("rows0", m)]


def _size_case():
    return plant_case("sizes", SIZES)


def _overflow_case():
    return plant_case("8193", (5, BK_BIG + 1, 70), seed=2)


def test_plant_model_equals_the_oracle(oracle):
    """The closed form of the planted cases against the CPU oracle, with no device: a wrong plant cannot hide."""
    case = plant_case("small", (0, 1, 2, 7, 65), seed=3)
    exp = _expected(oracle, case)
    assert len(exp) < sum(case["counts"])                                    # something merged
    assert any(s == 0 for _, _, s, _ in exp)                                 # clipped at the start of a genome
    assert all(any(e == case["glen"][g] for _, gg, _, e in exp if gg == g) for g in (0, 1))   # flush with its end
    lens = sorted({e - s for _, _, s, e in exp})
    assert 7 + PL + PEXT in lens and 2 * PL + 4 * PEXT in lens              # a lone clipped range; two that touch exactly
    mut = plant_case("small-mutated", (9, 20), mutate_runs=5, seed=4)
    _expected(oracle, mut, 4)
    with pytest.raises(AssertionError):                                      # ... and does not at 2 mismatches
        _expected(oracle, mut, 2)
    pr = plant_case("small-pairs", (5, 8), ext=0, pairs=True, seed=5)
    assert sorted({e - s for _, _, s, e in _expected(oracle, pr)}) == [PL, 2 * PL]


@pytest.mark.gpu
def test_scans_at_every_size_class(ctx, oracle):
    """One scan whose probes have 0 .. 8,192 hits, every size of SIZES: the seed scan (the key-grouped join files
    grouped records), the general scan (scattered records) and the tiled scan all give the oracle's rows; and
    cover_ranges gives the distinct ranges of the same hits, a bucket of exactly 8,192 among them."""
    import test_gpu_parity as gp
    engine = gp._engine()
    case = _size_case()
    exp = _expected(oracle, case)
    for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL, engine.SCAN_FAST):
        got = gp._scan_rows(ctx, case["probes"], case["genomes"], PM, PL, 0, PEXT, mode)
        # (the seed scan files one record per hit; the general scan one per anchor that found it -- four here --, so
        # its buckets are four times these sizes and merge equal ranges on top)
        hits = ctx.counters()["raw_hits"]
        assert hits == sum(SIZES) if mode == engine.SCAN_SEED else hits >= sum(SIZES), (mode, hits)
        assert got == exp, mode
    want = model_rows(case["plants"], case["glen"], PEXT, merge=False)
    assert max(np.bincount([r[0] for r in want])) == BK_BIG
    k, entries = oracle.anchor_table(case["probes"], PM, PL)
    orc = sorted({(int(p), g, max(0, a - PEXT), min(case["glen"][g], b + PEXT)) for g in (0, 1) for p, v in
                  oracle.scan_sequence(case["genomes"][g][0], case["probes"], entries, k, PM, PL, 0, merge=False).items()
                  for a, b in v})
    assert orc == want
    assert gp._scan_rows(ctx, case["probes"], case["genomes"], PM, PL, 0, PEXT, merge=False) == want


@pytest.mark.gpu
def test_scan_with_a_bucket_of_8193_and_the_cover_ranges_refusal(ctx, oracle):
    """One probe planted 8,193 times: every scan mode takes the radix build and gives the oracle's rows;
    cover_ranges refuses, says why, and hands its memory back."""
    import gc
    import test_gpu_parity as gp
    engine = gp._engine()
    case = _overflow_case()
    exp = _expected(oracle, case)
    for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL, engine.SCAN_FAST):
        assert gp._scan_rows(ctx, case["probes"], case["genomes"], PM, PL, 0, PEXT, mode) == exp, mode
    probe_mod = gp._probe_mod()
    k, uniq, owner, ep, eo = probe_mod.anchor_table(case["probes"], PM, PL)
    p, t = engine.Probes(ctx, uniq, owner, ep, eo, k), engine.Targets(ctx, case["genomes"])
    gc.collect()

    def in_use():
        st = engine.pool_stats()
        return st["bytes_held"] - st["bytes_cached_free"]
    before = in_use()
    with pytest.raises(ValueError, match="more than 8192 cover ranges"):
        engine.Rows.scan(ctx, p, t, PM, PL, 0, PEXT, merge=False)
    assert in_use() == before
    p.close(); t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 4])
def test_join_files_large_buckets_over_all_runs(ctx, oracle, m):
    """The key-grouped join at m + 1 = 3 and 5 anchor runs, buckets of 513, 2,049 and 4,097 hits (and wave buckets of
    2, 65, 129 and 512) whose copies are mutated so that their hits go round all runs; tolerant_bp (buckets =
    probes: the wave buckets are merged by runs) gives the sum of the oracle's per-sequence rows."""
    import test_gpu_parity as gp
    engine = gp._engine()
    case = plant_case(("join", m), (513, 2049, 4097, 2, 65, 129, 512), mutate_runs=m + 1, seed=10 + m)
    exp = _expected(oracle, case, m)
    got = gp._scan_rows(ctx, case["probes"], case["genomes"], m, PL, 0, PEXT, engine.SCAN_SEED)
    c = ctx.counters()
    assert c["join_pairs"] > 0 and c["raw_hits"] >= sum(case["counts"]), c
    assert got == exp
    _rows0(oracle, case, m)
    _check_tolerant_bp(ctx, case, m)


def _check_tolerant_bp(ctx, case, m):
    import test_gpu_parity as gp
    engine, probe_mod = gp._engine(), gp._probe_mod()
    k, uniq, owner, ep, eo = probe_mod.anchor_table(case["probes"], m, PL)
    p, t = engine.Probes(ctx, uniq, owner, ep, eo, k), engine.Targets(ctx, case["genomes"])
    out = np.zeros(len(uniq), dtype=np.int64)
    engine.tolerant_bp(ctx, p, t, m, PL, 0, out)
    p.close(); t.close()
    want = np.zeros(len(uniq), dtype=np.int64)
    for sid, _, a, b in case[("rows0", m)]:
        want[sid] += b - a
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:5]


@pytest.mark.gpu
def test_tolerant_bp_over_large_buckets(ctx, oracle):
    """tolerant_bp over the scan of the size table (a 2,049-hit bucket among them) = the sum of the oracle's
    per-sequence row lengths."""
    case = _size_case()
    _rows0(oracle, case, PM)
    _check_tolerant_bp(ctx, case, PM)


def _pairs_case():
    return plant_case("pairs", (1025, 4097), ext=0, pairs=True, seed=6)


@pytest.mark.gpu
def test_direct_rows_with_large_merging_buckets(ctx, oracle, monkeypatch):
    """The fused filter on device candidates (identity buckets) whose probes stand as tandem pairs at extension 0:
    the two copies of a pair touch and merge into one row of 200 bases, so the rows stay within 257 bases and the
    row-parallel solver reads the bucketed records in place -- behind 513 and 2,049 merged rows the stale records of
    a 1,025- and a 4,097-hit bucket.  Same picks as through the SoA table, and the oracle's selection."""
    import test_gpu_parity as gp
    from util import candidates
    engine, probe_mod = gp._engine(), gp._probe_mod()
    monkeypatch.setenv("CATCHHIP_FILTER_NO_DEFER", "1")
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    case = _pairs_case()
    genomes = case["genomes"]
    strs = candidates(genomes, PL, 50)
    ids = [strs.index(p) for p in case["probes"]]                         # the planted probes are candidates
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, PL, 50)
    assert c.n == len(strs)
    p = c.probes(probe_mod.anchor_table([case["probes"][0]], PM, PL, assume_unique=True)[0])
    rows = engine.Rows.scan(ctx, p, t, PM, PL, 0, 0)
    sid, _, st, en = rows.fetch()
    want = (rows.greedy(c.n), rows.n)
    rows.close()
    for i, n in zip(ids, case["counts"]):
        assert int((sid == i).sum()) == n // 2 + 1 and set((en - st)[sid == i].tolist()) == {PL, 2 * PL}
    assert int((en - st).max()) == 2 * PL <= 257
    got = engine.setcover_filter(ctx, p, t, PM, PL, 0, 0, c.n)
    cnt = ctx.counters()
    assert cnt["rows_direct"] == 1 and cnt["flat_rows_streamed"] > 0
    assert cnt["raw_hits"] > got[1]                                       # something merged: stale records in the table
    assert got == want
    if "picks" not in case:
        case["picks"] = sorted(oracle.set_cover_filter([strs], [genomes], PM, PL, coverage=1.0, cover_extension=0)[0])
    assert sorted(got[0]) == case["picks"]
    p.close(); c.close(); t.close()
