"""The no-touch path of the bucketed row build (csrc/rows_bucket.inc: bucket_no_touch, bucket_merge_kernel<64, 512, true>)
against a sequential merge in NumPy.

Buckets given as anchor runs whose records do not touch leave the kernel without the LDS permute and the merge walk:
the records that are not at their place are stored from registers, the rest stay.  A bucket in which anything touches
takes the general path.  Everything goes through Context.selftest_row_build(form="grouped", run_cnt=..., nruns=...);
every case compares the rows S[bstart[b] : bstart[b] + mcnt[b]], mcnt, blmax, bsum and `.w == b` on every slot (the
rows and the stale slots behind them).  All values are integers and every comparison is for equality.

What each launch is for:
  clean sizes     n = 1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512 (every register-slot count of the path, the
                  sizes around its borders, and the sizes past its last slot), 1 .. 5 runs, an empty run first, in the
                  middle and last, all records in one run, runs that interleave record by record, in blocks, at random.
  planted touch   one touch in an otherwise clean bucket: inside a run and across two runs, between merged positions
                  5|6, 63|64, 127|128 and the last two; start == previous end (merges) beside start == previous end + 1
                  (does not); equal starts in two runs; a long record that reaches a record three places on.
  segments        two records of different segments that touch (must not merge), beside two of one segment (must).
  second bucket   more than 2^20 buckets in one launch: the grid is capped at 2^20 workgroups, so the first 70
                  wavefronts take a second bucket; the two alternate between touched and clean, and between one, two
                  and four register slots and a single record.
  dedupe          cover_ranges' mode with runs: equal records collapse, nothing merges, touching or not.
"""
import numpy as np
import pytest

SEGLEN = 1 << 23
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512)
GRID_CAP = 1 << 20


# ------------------------------------------------------------------ reference
def merge_reference(hits, nb, dedupe=False):
    """The rows of hit records {start, end, segment, bucket}: per bucket, sorted by (start, end), a record joins the
    row in progress iff it has the row's segment and start <= the row's end, the running maximum of the ends.  The
    sequential pass, written with a running maximum per (bucket, segment) group.  dedupe: equal (start, end) collapse,
    nothing merges.  Returns rows (bucket, segment, start, end) in (bucket, start) order and mcnt, blmax, bsum."""
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 4)
    o = np.lexsort((h[:, 1], h[:, 0], h[:, 3]))
    s, e, g, b = h[o, 0], h[o, 1], h[o, 2], h[o, 3]
    n = s.size
    if n == 0:
        z = np.zeros(nb, dtype=np.int64)
        return np.zeros((0, 4), dtype=np.int64), z, z.copy(), z.copy()
    first = np.ones(n, dtype=bool)
    if dedupe:
        first[1:] = (b[1:] != b[:-1]) | (s[1:] != s[:-1]) | (e[1:] != e[:-1])
        rows = np.stack([b[first], g[first], s[first], e[first]], axis=1)
    else:
        first[1:] = (b[1:] != b[:-1]) | (g[1:] != g[:-1])
        gid = np.cumsum(first) - 1
        big = np.int64(1) << 33
        runmax = np.maximum.accumulate(e + gid * big) - gid * big     # running maximum of the ends inside the group
        head = first.copy()
        head[1:] |= s[1:] > runmax[:-1]
        last = np.append(head[1:], True)
        rows = np.stack([b[head], g[head], s[head], runmax[last]], axis=1)
    length = rows[:, 3] - rows[:, 2]
    mcnt = np.bincount(rows[:, 0], minlength=nb)
    blmax, bsum = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    np.maximum.at(blmax, rows[:, 0], length)
    np.add.at(bsum, rows[:, 0], length)
    return rows, mcnt, blmax, bsum


def test_reference_on_a_case_written_down_by_hand():
    hits = [(30, 40, 0, 1), (10, 20, 0, 1), (20, 25, 0, 1),          # 10-20 touches 20-25; 30-40 stands alone
            (100, 200, 0, 3), (150, 160, 0, 3), (190, 260, 0, 3),    # 150-160 lies inside; 190 <= 200, the maximum
            (261, 270, 0, 3),                                        # one base past 260: a row of its own
            (500, 600, 0, 4), (600, 700, 1, 4),                      # touching, but two segments
            (5, 9, 0, 5), (5, 9, 0, 5), (5, 7, 0, 5)]
    rows, mcnt, blmax, bsum = merge_reference(hits, 6)
    assert rows.tolist() == [[1, 0, 10, 25], [1, 0, 30, 40], [3, 0, 100, 260], [3, 0, 261, 270], [4, 0, 500, 600],
                             [4, 1, 600, 700], [5, 0, 5, 9]]
    assert mcnt.tolist() == [0, 2, 0, 2, 2, 1] and blmax.tolist() == [0, 15, 0, 160, 100, 4]
    assert bsum.tolist() == [0, 25, 0, 169, 200, 4]
    rows, mcnt, _, bsum = merge_reference(hits, 6, dedupe=True)
    assert mcnt.tolist() == [0, 3, 0, 4, 2, 2] and bsum[5] == 6 and rows[-2:].tolist() == [[5, 0, 5, 7], [5, 0, 5, 9]]


# ------------------------------------------------------------------ buckets
def clean_bucket(n, first=1000):
    """n records (start, end, segment) of 100 bases every 200: nothing touches."""
    start = first + 200 * np.arange(n, dtype=np.int64)
    return np.stack([start, start + 100, start // SEGLEN], axis=1)


def deal(n, live, style, rng):
    """The run of each of n sorted records: over the runs `live`, record by record, in blocks, or at random."""
    live = np.asarray(live, dtype=np.int64)
    if style == "interleave":
        return live[np.arange(n) % live.size]
    if style == "blocks":
        return live[np.minimum(np.arange(n) * live.size // max(n, 1), live.size - 1)]
    return live[rng.integers(0, live.size, size=n)]


def as_runs(b, run_of, nruns):
    """The sorted records b as the join leaves them: run after run, each in (start, end) order; and the run lengths."""
    o = np.argsort(run_of, kind="stable")
    return b[o], np.bincount(run_of, minlength=nruns)


def launch(ctx, buckets, cnts, nruns, stride=None, dedupe=False):
    """One build of the buckets (record arrays standing run after run) with their run lengths."""
    nb = len(buckets)
    stride = nruns + (nruns & 1) if stride is None else stride
    hits = np.concatenate([np.concatenate((b, np.full((len(b), 1), k, dtype=np.int64)), axis=1)
                           for k, b in enumerate(buckets)])
    run_cnt = np.zeros((nb, stride), dtype=np.int64)
    run_cnt[:, :nruns] = np.array(cnts, dtype=np.int64).reshape(nb, nruns)
    out = ctx.selftest_row_build(hits, nb, form="grouped", run_cnt=run_cnt, nruns=nruns, dedupe=dedupe)
    return hits, out


def check(out, hits, nb, what, dedupe=False):
    rows, mcnt, blmax, bsum = merge_reference(hits, nb, dedupe=dedupe)
    assert not out["overflow"] and out["hits"] == len(hits) and out["rows"] == len(rows), (what, out["rows"], len(rows))
    for k, ref in (("mcnt", mcnt), ("blmax", blmax), ("bsum", bsum)):
        bad = np.nonzero(out[k].astype(np.int64) != ref)[0]
        assert bad.size == 0, (what, k, bad[:5].tolist(), out[k][bad[:5]].tolist(), ref[bad[:5]].tolist())
    S, bstart = out["S"].astype(np.int64), out["bstart"].astype(np.int64)
    slot = np.arange(S.shape[0])
    # every slot, row or stale, carries the bucket whose [bstart, bstart + n) holds it
    assert np.array_equal(S[:, 3], np.searchsorted(bstart, slot, side="right") - 1), what
    is_row = slot - bstart[S[:, 3]] < mcnt[S[:, 3]]
    got = S[is_row][:, [3, 2, 0, 1]]
    bad = np.nonzero((got != rows).any(axis=1))[0] if got.shape == rows.shape else np.array([-1])
    assert bad.size == 0, (what, bad[:5].tolist(), got[bad[:5]].tolist(), rows[bad[:5]].tolist())
    return mcnt


# ------------------------------------------------------------------ on the device
@pytest.mark.gpu
@pytest.mark.parametrize("nruns", [1, 2, 3, 4, 5])
def test_clean_buckets_of_every_size_and_run_layout(ctx, nruns):
    rng = np.random.default_rng(100 + nruns)
    buckets, cnts = [], []
    for n in SIZES:
        for empty in (None, 0, nruns // 2, nruns - 1):
            if empty is not None and (nruns == 1 or (empty == nruns // 2 and empty in (0, nruns - 1))):
                continue
            live = [a for a in range(nruns) if a != empty]
            for style in ("interleave", "blocks", "random"):
                recs, c = as_runs(clean_bucket(n), deal(n, live, style, rng), nruns)
                buckets.append(recs)
                cnts.append(c)
        one = np.full(n, nruns - 1, dtype=np.int64)                 # all records in one run, the last
        recs, c = as_runs(clean_bucket(n), one, nruns)
        buckets.append(recs)
        cnts.append(c)
    hits, out = launch(ctx, buckets, cnts, nruns)
    mcnt = check(out, hits, len(buckets), ("clean", nruns))
    assert np.array_equal(mcnt, [len(b) for b in buckets])          # nothing merged: every record is a row
    # ... and the bucket comes back as its records in start order: a one-run bucket unchanged
    S = out["S"].astype(np.int64)
    assert np.array_equal(S, hits[np.lexsort((hits[:, 0], hits[:, 3]))])


def planted(n, j, kind):
    """A clean bucket of n sorted records with one plant at sorted positions j | j + 1; True if it merges anything."""
    b = clean_bucket(n)
    if kind == "touch":                    # start == previous end: merges
        b[j, 1] = b[j + 1, 0]
    elif kind == "one_past":               # start == previous end + 1: does not
        b[j, 1] = b[j + 1, 0] - 1
    elif kind == "equal_starts":           # two records of one start (sorted by end)
        b[j + 1, 0] = b[j, 0]
        b[j + 1, 1] = b[j, 1] + 7
    elif kind == "long":                   # reaches the record three places on, and so the two between
        b[j, 1] = b[min(j + 3, n - 1), 0] + 5
    else:
        raise AssertionError(kind)
    return b, kind != "one_past"


@pytest.mark.gpu
@pytest.mark.parametrize("nruns", [2, 3, 5])
def test_one_planted_touch_in_a_clean_bucket(ctx, nruns):
    rng = np.random.default_rng(200 + nruns)
    buckets, cnts, merges = [], [], []
    live = list(range(nruns))
    for n in (7, 66, 130, 200):
        for j in sorted({5, 63, 127, n - 2}):
            if j + 1 >= n:
                continue
            for kind in ("touch", "one_past", "equal_starts", "long"):
                # blocks of 8: j | j + 1 inside one run (j % 8 != 7); interleave: in two runs; "far": the record before
                # j + 1 in its own run is far away, j stands alone in another run
                for style in ("blocks8", "interleave", "far"):
                    b, m = planted(n, j, kind)
                    if style == "blocks8":
                        run_of = (np.arange(n) // 8) % nruns
                    elif style == "interleave":
                        run_of = deal(n, live, "interleave", rng)
                    else:
                        run_of = np.zeros(n, dtype=np.int64)
                        run_of[j] = nruns - 1
                    recs, c = as_runs(b, run_of, nruns)
                    buckets.append(recs)
                    cnts.append(c)
                    merges.append(m)
    hits, out = launch(ctx, buckets, cnts, nruns)
    mcnt = check(out, hits, len(buckets), ("planted", nruns))
    sizes = np.array([len(b) for b in buckets])
    assert np.array_equal(mcnt < sizes, merges)                     # the plants do what their names say


@pytest.mark.gpu
def test_segments_and_neighbours_that_alternate(ctx):
    """A touch across a segment border does not merge, one inside a segment does; and 64 buckets of 70 records that
    alternate between touched and clean."""
    buckets, cnts = [], []
    for same_segment in (False, True):
        b = clean_bucket(100, SEGLEN - 200 * 50)                    # record 50 starts the second segment
        assert b[49, 2] == 0 and b[50, 2] == 1 and b[50, 0] == SEGLEN
        j = 20 if same_segment else 49
        b[j, 1] = b[j + 1, 0]
        for run_of in (np.arange(100) % 3, np.arange(100) // 34):
            recs, c = as_runs(b, run_of, 3)
            buckets.append(recs)
            cnts.append(c)
    for k in range(64):
        b = clean_bucket(70)
        if k % 2:
            b[3 + k, 1] = b[4 + k, 0] + 1
        recs, c = as_runs(b, np.arange(70) % 3, 3)
        buckets.append(recs)
        cnts.append(c)
    hits, out = launch(ctx, buckets, cnts, 3)
    mcnt = check(out, hits, len(buckets), "segments")
    assert mcnt[:4].tolist() == [100, 100, 99, 99] and mcnt[4:].tolist() == [70, 69] * 32


@pytest.mark.gpu
def test_a_wavefront_takes_a_second_bucket(ctx):
    """2^20 + 70 buckets in one launch: wavefront w < 70 merges bucket w and bucket 2^20 + w.  The first holds 60 + w
    records (one, two and four register slots), the second one to three; of each pair one is touched and one is clean,
    in alternation; a tenth of the other buckets (one to three records) are touched."""
    nb, nruns = GRID_CAP + 70, 3
    rng = np.random.default_rng(5)
    cnt = rng.integers(1, 4, size=nb)
    cnt[:70] = 60 + np.arange(70)
    touchy = rng.random(nb) < 0.1
    touchy[:70] = np.arange(70) % 2 == 0
    touchy[GRID_CAP:] = np.arange(70) % 2 == 1
    cnt[GRID_CAP:][touchy[GRID_CAP:]] = np.maximum(cnt[GRID_CAP:][touchy[GRID_CAP:]], 2)
    b = np.repeat(np.arange(nb, dtype=np.int64), cnt)
    j = np.arange(b.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    start = 1000 + b % 7 + 150 * j
    end = start + 100
    plant = touchy[b] & (j == (cnt[b] - 2) // 2)                    # one record per touched bucket reaches the next
    end[plant] += 60
    run = rng.integers(0, nruns, size=b.size)
    o = np.lexsort((start, run, b))                                 # a bucket = its runs side by side, each by start
    hits = np.stack([start, end, start // SEGLEN, b], axis=1)[o]
    run_cnt = np.zeros((nb, 4), dtype=np.int64)
    run_cnt[:, :nruns] = np.bincount(b * nruns + run, minlength=nb * nruns).reshape(nb, nruns)
    out = ctx.selftest_row_build(hits, nb, form="grouped", run_cnt=run_cnt, nruns=nruns)
    mcnt = check(out, hits, nb, "second bucket")
    expect = cnt - (touchy & (cnt > 1))
    assert np.array_equal(mcnt, expect)


@pytest.mark.gpu
def test_dedupe_with_runs_keeps_its_walk(ctx):
    """dedupe=True with runs: equal records collapse, nothing merges -- a clean bucket, a touched one, one with four
    records twice (in two runs each) and one whose every record stands in all three runs."""
    clean, touched = clean_bucket(150), clean_bucket(150)
    touched[70, 1] = touched[71, 0] + 3
    dup = np.concatenate((clean, clean[10:12], clean[63:65]))
    dup = dup[np.lexsort((dup[:, 1], dup[:, 0]))]
    buckets, cnts = [], []
    for b in (clean, touched, dup):
        recs, c = as_runs(b, np.arange(len(b)) % 3, 3)
        buckets.append(recs)
        cnts.append(c)
    buckets.append(np.concatenate([clean] * 3))
    cnts.append([150, 150, 150])
    hits, out = launch(ctx, buckets, cnts, 3, dedupe=True)
    mcnt = check(out, hits, 4, "dedupe", dedupe=True)
    assert mcnt.tolist() == [150, 150, 150, 150]
