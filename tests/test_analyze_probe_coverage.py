"""The coverage analysis command (catch_amd.analyze_probe_coverage) and the sliding-window depth on the device
(catchhip_rows_window_depth in csrc/analysis.hip, Rows.window_depth, Analyzer.sliding_coverage).

The reference results are recorded by tests/golden/make_analysis_golden.py from the live reference
(tests/golden/analysis_cli.json.gz): per case the inputs, the cover ranges, `sliding_coverage`, the three written
files and the printed report.  The window rule is restated here in NumPy (restate_windows); the restatement is
pinned to the recorded reference results without a GPU, and the kernel is then tested against the restatement."""
import functools
import gzip
import json
import logging
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def golden_cases():
    with gzip.open(os.path.join(GOLDEN, "analysis_cli.json.gz"), "rt") as f:
        return json.load(f)["cases"]


# ------------------------------------------------------------------ the window rule, restated
def restate_windows(starts, ends, n, length, stride):
    """catch/coverage_analysis.py:377-411 on ranges [start, end) of a genome of n bases: the depth per base as
    uint16, windows from 0, stride, .. < n, one that passes the end moved to [n - length, n) -- as a slice, so a
    negative start follows Python's rule.  -> [(reported start, sum of the depth, bases)] per window, in order."""
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, np.asarray(starts, dtype=np.int64), 1)
    np.add.at(diff, np.asarray(ends, dtype=np.int64), -1)
    depth = np.cumsum(diff[:n]).astype(np.uint16)
    out = []
    for ws in range(0, n, stride):
        we = ws + length
        if we > n:
            we = n
            ws = we - length
        piece = depth[ws:we]
        out.append((ws, int(piece.sum(dtype=np.uint64)), int(piece.size)))
    return out


def restate_windows_vectorised(starts, ends, n, length, stride):
    """restate_windows without the Python loop over the windows (a table of millions of positions has hundreds of
    thousands): the depth as uint16, its prefix sums in 64 bits, and the slice rule written out -- a window that
    passes the end becomes depth[n - length : n], whose negative start counts from the end and stops at 0.  Same
    result, the reported start (negative when n < length) included."""
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, np.asarray(starts, dtype=np.int64), 1)
    np.add.at(diff, np.asarray(ends, dtype=np.int64), -1)
    depth = np.cumsum(diff[:n]).astype(np.uint16)
    prefix = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(depth, dtype=np.uint64, out=prefix[1:])
    ws = np.arange(0, n, stride, dtype=np.int64)
    we = ws + length
    over = we > n
    we = np.where(over, n, we)
    ws = np.where(over, we - length, ws)
    lo = np.where(ws < 0, np.maximum(ws + n, 0), ws)            # the slice's own start
    sums = prefix[we] - prefix[lo]
    return list(zip(ws.tolist(), sums.tolist(), (we - lo).tolist()))


def restated_dict(starts, ends, n, length, stride):
    return {ws + length / 2: float(s) / c for ws, s, c in restate_windows(starts, ends, n, length, stride)}


# ------------------------------------------------------------------ without a GPU
def _base_argv():
    return ["-d", "a.fasta", "-f", "p.fasta", "-m", "2", "-l", "100"]


def test_argument_surface_matches_the_reference():
    """Option names, required options and defaults of bin/analyze_probe_coverage.py:96-220."""
    from catch_amd import analyze_probe_coverage as apc
    a = apc.parse_args(_base_argv())
    assert (a.dataset, a.probes_fasta, a.mismatches, a.lcf_thres) == (["a.fasta"], "p.fasta", 2, 100)
    assert (a.island_of_exact_match, a.cover_extension, a.limit_target_genomes) == (0, 0, None)
    assert (a.print_analysis, a.write_analysis_to_tsv, a.write_sliding_window_coverage,
            a.write_probe_map_counts_to_tsv) == (False, None, None, None)
    assert (a.kmer_probe_map_k, a.max_num_processes, a.log_level, a.params) == (10, None, logging.WARNING, None)
    a = apc.parse_args(["--dataset", "a.fasta", "b.fasta", "--probes-fasta", "p.fasta", "--mismatches", "3",
                        "--lcf-thres", "80", "--island-of-exact-match", "20", "--cover-extension", "25",
                        "--limit-target-genomes", "4", "--print-analysis", "--write-analysis-to-tsv", "a.tsv",
                        "--write-sliding-window-coverage", "s.tsv", "--write-probe-map-counts-to-tsv", "c.tsv",
                        "--kmer-probe-map-k", "12", "--max-num-processes", "3", "--verbose"])
    assert (a.dataset, a.mismatches, a.lcf_thres, a.island_of_exact_match, a.cover_extension) == \
        (["a.fasta", "b.fasta"], 3, 80, 20, 25)
    assert (a.limit_target_genomes, a.print_analysis, a.write_analysis_to_tsv, a.write_sliding_window_coverage,
            a.write_probe_map_counts_to_tsv, a.kmer_probe_map_k, a.max_num_processes, a.log_level) == \
        (4, True, "a.tsv", "s.tsv", "c.tsv", 12, 3, logging.INFO)
    assert apc.parse_args(_base_argv() + ["--debug"]).log_level == logging.DEBUG
    assert apc.parse_args(_base_argv() + ["-e", "7"]).cover_extension == 7
    for flag in ("-d", "-f", "-m", "-l"):
        argv = _base_argv()
        at = argv.index(flag)
        with pytest.raises(SystemExit):
            apc.parse_args(argv[:at] + argv[at + 2:])
    with pytest.raises(SystemExit):
        apc.parse_args(_base_argv() + ["--max-num-processes", "0"])


def test_download_labels_and_missing_files_are_refused(tmp_path):
    from catch_amd import analyze_probe_coverage as apc
    probes = tmp_path / "p.fasta"
    probes.write_text(">p\nACGT\n")
    for label, why in (("download:11320", "network"), (str(tmp_path / "not_there.fasta"), "not a file"),
                       ("zaire_ebolavirus", "not a file")):
        args = apc.parse_args(["-d", label, "-f", str(probes), "-m", "0", "-l", "4"])
        with pytest.raises(ValueError, match=why):
            apc.main(args)


def _params(path, rows):
    path.write_text("dataset\tmismatches\tcover_extension\n" + "".join("%s\t%s\t%s\n" % r for r in rows))
    return str(path)


def test_params_is_exclusive_with_m_and_e_and_names_every_dataset(tmp_path, capsys):
    from catch_amd import analyze_probe_coverage as apc
    argv = ["-d", "dir/ebola.fasta", "other/lassa.fa.gz", "-f", "p.fasta", "-l", "100"]
    table = _params(tmp_path / "params.tsv", [("lassa", 3, 20), ("ebola", 1, 0)])
    a = apc.parse_args(argv + ["--params", table])
    assert (a.params, a.mismatches, a.cover_extension) == (table, None, None)
    for extra in (["-m", "2"], ["-e", "10"], ["-m", "2", "-e", "10"]):
        with pytest.raises(SystemExit):
            apc.parse_args(argv + ["--params", table] + extra)
        assert "--params" in capsys.readouterr().err
    # every dataset under its own row, in -d order whatever the order of the rows
    assert apc.params_per_dataset(table, a.dataset) == [(1, 0), (3, 20)]
    with pytest.raises(ValueError, match="no row for dataset lassa"):
        apc.params_per_dataset(_params(tmp_path / "a.tsv", [("ebola", 1, 0)]), a.dataset)
    with pytest.raises(ValueError, match="not given with -d: zika"):
        apc.params_per_dataset(_params(tmp_path / "b.tsv", [("lassa", 3, 20), ("ebola", 1, 0), ("zika", 0, 0)]),
                               a.dataset)
    with pytest.raises(ValueError, match="not an integer"):
        apc.params_per_dataset(_params(tmp_path / "c.tsv", [("lassa", "2.5", 20), ("ebola", 1, 0)]), a.dataset)
    with pytest.raises(ValueError, match="two rows"):
        apc.params_per_dataset(_params(tmp_path / "d.tsv", [("lassa", 3, 20), ("ebola", 1, 0), ("ebola", 2, 0)]),
                               a.dataset)
    with pytest.raises(ValueError, match="share a name"):
        apc.params_per_dataset(table, ["x/ebola.fasta", "y/ebola.fa", "lassa.fasta"])
    # values written as %f by pool without --round-params are read when they are whole
    assert apc.params_per_dataset(_params(tmp_path / "e.tsv", [("lassa", "3.000000", "20.000000"),
                                                                ("ebola", "1.000000", "0.000000")]),
                                  a.dataset) == [(1, 0), (3, 20)]


def test_window_depth_symbol_declared_and_bound():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    name = "catchhip_rows_window_depth"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert "coverage_analysis.py:336-413" in hdr
    assert name in _lib.PROTOTYPES
    assert "analysis.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert callable(engine.Rows.window_depth)


def test_restated_window_rule_equals_the_recorded_reference():
    """restate_windows on the recorded cover ranges gives the recorded sliding_coverage of every genome and strand
    of every case, keys and values -- among them genomes shorter than the window and than half of it that ARE
    covered unevenly: the 40-base genome is covered on [0, 30) and its window [30, 40) averages 0, the
    20-base genome's window is the whole genome."""
    seen_short = set()
    ngenomes = 0
    for c in golden_cases():
        for i, grp in enumerate(c["genome_lengths"]):
            for j, n in enumerate(grp):
                for r in range(2):
                    cov = c["target_covers"][i][j][r]
                    got = restated_dict([a for a, _ in cov], [b for _, b in cov], n, 50, 25)
                    want = {k: v for k, v in c["sliding_coverage"][i][j][r]}
                    assert got == want, (c["name"], i, j, r)
                    ngenomes += 1
                    if n < 50 and cov:
                        seen_short.add("half" if n < 25 else "window")
    assert ngenomes >= 60 and seen_short == {"half", "window"}
    # the slice rule on its own: n < length
    assert restate_windows([0], [30], 40, 50, 25) == [(-10, 0, 10), (-10, 0, 10)]
    assert restate_windows([0], [15], 20, 50, 25) == [(-30, 15, 20)]
    assert restate_windows([], [], 0, 50, 25) == []


# ------------------------------------------------------------------ on the GPU
def _random_table(rng, lengths, nsets, max_intervals):
    """Rows sorted by (set, universe, start), disjoint and not touching inside a (set, universe)."""
    si, un, st, en = [], [], [], []
    for s in range(nsets):
        for u, ln in enumerate(lengths):
            k = int(rng.integers(0, max_intervals + 1))
            k = min(k, (ln + 1) // 2)
            if k == 0:
                continue
            pts = np.sort(rng.choice(ln + 1, size=2 * k, replace=False))
            for a, b in zip(pts[0::2], pts[1::2]):
                si.append(s); un.append(u); st.append(int(a)); en.append(int(b))
    return (np.asarray(si, np.int32), np.asarray(un, np.int32), np.asarray(st, np.int64), np.asarray(en, np.int64))


def _expect_windows(un, st, en, lengths, span_first, length, stride, restate=restate_windows):
    off = np.concatenate(([0], np.cumsum(lengths)))
    sums, counts, per_span = [], [], []
    for u0, u1 in zip(span_first[:-1], span_first[1:]):
        inside = (un >= u0) & (un < u1)
        base = off[un[inside]] - off[u0]
        w = restate(st[inside] + base, en[inside] + base, int(off[u1] - off[u0]), length, stride)
        sums += [x[1] for x in w]
        counts += [x[2] for x in w]
        per_span.append(len(w))
    return sums, counts, np.concatenate(([0], np.cumsum(per_span))).tolist()


def _kernel_test_shapes():
    """The table, the span sets and the (window, stride) pairs of test_window_depth_kernel_equals_the_restatement."""
    rng = np.random.default_rng(5)
    lengths = np.asarray([700, 0, 1300, 37, 2048, 1, 24, 5000, 0, 0, 90, 4096, 333, 49, 50, 51], dtype=np.int64)
    table = _random_table(rng, lengths, nsets=40, max_intervals=3)
    nu = len(lengths)
    span_sets = [
        np.arange(nu + 1),                                    # every universe a span
        np.asarray([0, 3, 3, 5, 8, 8, 8, 10, 12, 16]),        # several universes per span, empty spans
        np.asarray([2, 7, 13]),                               # not from universe 0, not to the last
        np.asarray([0, nu]),                                  # everything one genome
        np.asarray([4, 4]),                                   # one empty span
    ]
    return lengths, table, span_sets, ((50, 25), (1, 1), (7, 3), (3, 7), (20000, 1000), (4000, 1), (2048, 2048))


def test_vectorised_window_rule_equals_the_looped_one_and_the_recorded_reference():
    """No GPU: restate_windows_vectorised == restate_windows, window by window (reported start, sum, bases), on every
    span and (window, stride) pair of the kernel test -- spans shorter than the window and than half of it, empty
    ones and windows longer than every span among them -- and on the recorded cover ranges, where it therefore gives
    the recorded sliding_coverage as restate_windows does."""
    lengths, (_si, un, st, en), span_sets, shapes = _kernel_test_shapes()
    off = np.concatenate(([0], np.cumsum(lengths)))
    seen = set()
    for span_first in span_sets:
        for u0, u1 in zip(span_first[:-1], span_first[1:]):
            inside = (un >= u0) & (un < u1)
            base = off[un[inside]] - off[u0]
            n = int(off[u1] - off[u0])
            for length, stride in shapes:
                args = (st[inside] + base, en[inside] + base, n, length, stride)
                assert restate_windows_vectorised(*args) == restate_windows(*args), (u0, u1, length, stride)
                seen.add("empty" if n == 0 else "half" if 2 * n < length else "window" if n < length else "long")
    assert seen == {"empty", "half", "window", "long"}
    for length, stride in shapes:
        want = _expect_windows(un, st, en, lengths, span_sets[1], length, stride)
        assert _expect_windows(un, st, en, lengths, span_sets[1], length, stride, restate=restate_windows_vectorised) == want
    assert restate_windows_vectorised([0], [30], 40, 50, 25) == [(-10, 0, 10), (-10, 0, 10)]
    assert restate_windows_vectorised([0], [15], 20, 50, 25) == [(-30, 15, 20)]
    assert restate_windows_vectorised([], [], 0, 50, 25) == []
    ngenomes = 0
    for c in golden_cases():
        for i, grp in enumerate(c["genome_lengths"]):
            for j, n in enumerate(grp):
                for r in range(2):
                    cov = c["target_covers"][i][j][r]
                    args = ([a for a, _ in cov], [b for _, b in cov], n, 50, 25)
                    got = restate_windows_vectorised(*args)
                    assert got == restate_windows(*args), (c["name"], i, j, r)
                    assert {ws + 50 / 2: float(s) / k for ws, s, k in got} == \
                        {k: v for k, v in c["sliding_coverage"][i][j][r]}, (c["name"], i, j, r)
                    ngenomes += 1
    assert ngenomes >= 60


@pytest.mark.gpu
def test_window_depth_kernel_equals_the_restatement(ctx):
    """catchhip_rows_window_depth on tables built with catchhip_rows_from_host: random spans of several universes
    (empty universes and empty spans among them, spans that start after universe 0, tiles of 2048 positions
    crossed), window / stride pairs with the window longer than every span among them."""
    from catch_amd import engine
    lengths, (si, un, st, en), span_sets, shapes = _kernel_test_shapes()
    rows = engine.Rows.from_host(ctx, si, un, st, en, lengths)
    covered = 0
    for span_first in span_sets:
        for length, stride in shapes:
            sums, counts, win_off = rows.window_depth(span_first, length, stride)
            want = _expect_windows(un, st, en, lengths, span_first, length, stride)
            assert win_off.tolist() == want[2], (span_first, length, stride)
            assert sums.tolist() == want[0], (span_first, length, stride)
            assert counts.tolist() == want[1], (span_first, length, stride)
            covered += sum(want[0])
    assert covered > 0
    # no spans, and a table without rows
    sums, counts, win_off = rows.window_depth([], 50, 25)
    assert (sums.size, counts.size, win_off.tolist()) == (0, 0, [0])
    rows.close()
    empty = engine.Rows.from_host(ctx, [], [], [], [], [120, 30])
    sums, counts, win_off = empty.window_depth([0, 1, 2], 50, 25)
    assert sums.tolist() == [0] * 7 and counts.tolist() == [50, 50, 50, 50, 50, 20, 20] and win_off.tolist() == [0, 5, 7]
    empty.close()


@pytest.mark.gpu
def test_window_depth_wraps_at_65536_and_refuses_bad_arguments(ctx):
    """A position under 65,537 sets has depth 1 (the reference's uint16); the CATCHHIP_EINVAL cases.  (A deferred
    row table is refused too, but the library never hands one to a caller.)"""
    from catch_amd import engine
    nsets = 65537
    lengths = [200, 100]
    si = np.arange(nsets, dtype=np.int32)
    rows = engine.Rows.from_host(ctx, np.concatenate((si, [nsets])), np.zeros(nsets + 1, np.int32),
                                 np.concatenate((np.full(nsets, 60), [10])), np.concatenate((np.full(nsets, 90), [75])),
                                 lengths)
    un = np.zeros(nsets + 1, np.int64)
    st = np.concatenate((np.full(nsets, 60), [10])).astype(np.int64)
    en = np.concatenate((np.full(nsets, 90), [75])).astype(np.int64)
    for length, stride in ((50, 25), (1, 1), (300, 100)):
        sums, counts, _off = rows.window_depth([0, 1, 2], length, stride)
        want = _expect_windows(un, st, en, np.asarray(lengths), [0, 1, 2], length, stride)
        assert sums.tolist() == want[0] and counts.tolist() == want[1]
    sums, _counts, _off = rows.window_depth([0, 1], 1, 1)
    # 65,538 sets cover 60..74 (depth 2 after the wrap), 65,537 cover 75..89 (depth 1), one covers 10..59
    assert sums.tolist() == [0] * 10 + [1] * 50 + [2] * 15 + [1] * 15 + [0] * 110
    for span_first, length, stride in (([0, 1], 0, 25), ([0, 1], 50, 0), ([0, 1], -3, 25), ([0, 1], 50, -1),
                                       ([1, 0], 50, 25), ([0, 2, 1, 2], 50, 25), ([0, 3], 50, 25),
                                       ([-1, 1], 50, 25), ([0, 5, 2], 50, 25)):
        with pytest.raises(ValueError):
            rows.window_depth(span_first, length, stride)
    # too little room for the windows
    sf = np.asarray([0, 2], dtype=np.int64)
    per = np.zeros(1, np.int64)
    out_s, out_c = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    from catch_amd._lib import c_i64p, c_u32p, c_u64p
    rc = ctx._L.catchhip_rows_window_depth(ctx._h, rows._h, sf.ctypes.data_as(c_i64p), 1, 50, 25,
                                           per.ctypes.data_as(c_i64p), out_s.ctypes.data_as(c_u64p),
                                           out_c.ctypes.data_as(c_u32p), 4)
    assert rc == -1 and per[0] == 12
    rows.close()


# ------------------------------------------------------------------ the second turns: more than 1,024 tiles, more windows than threads
WD_TILE = 2048                     # positions per tile of wd_tile_kernel; wd_tilescan_kernel scans 1,024 tile sums per turn
CARRY_AT = 1024 * WD_TILE          # = 2,097,152: the first position whose prefix needs the carry of the second turn
BIG_LENGTHS = (777, 0, 2_200_123)  # a short universe, an empty one, one of a little more than 2,200,000 bases


@functools.lru_cache(maxsize=1)
def _big_table():
    """A few thousand rows over 7 sets by _random_table's rules; set 6 is written by hand around CARRY_AT (global
    coordinates: the long universe starts at 777)."""
    rng = np.random.default_rng(2097152)
    lengths = np.asarray(BIG_LENGTHS, dtype=np.int64)
    si, un, st, en = _random_table(rng, lengths, nsets=6, max_intervals=600)
    x = CARRY_AT - int(lengths[0])               # the long universe's own coordinate of CARRY_AT
    by_hand = [(5, 90), (x - 70000, x - 3), (x - 2, x + 1), (x + 2, x + 2049), (x + 5000, x + 90000),
               (int(lengths[2]) - 4000, int(lengths[2]))]
    si = np.concatenate((si, np.full(len(by_hand), 6, np.int32)))
    un = np.concatenate((un, np.full(len(by_hand), 2, np.int32)))
    st = np.concatenate((st, np.asarray([a for a, _ in by_hand], np.int64)))
    en = np.concatenate((en, np.asarray([b for _, b in by_hand], np.int64)))
    return lengths, si, un, st, en


def test_big_window_table_is_what_it_claims():
    """No GPU: the table obeys _random_table's rules, has more than 1,024 tiles, rows on both sides of CARRY_AT and
    rows that straddle it."""
    lengths, si, un, st, en = _big_table()
    assert 2000 <= si.size <= 9000 and np.unique(si).size == 7
    order = np.lexsort((st, un, si))
    assert (order == np.arange(si.size)).all()                              # sorted by (set, universe, start)
    assert (st < en).all() and (st >= 0).all() and (en <= lengths[un]).all()
    same = (si[1:] == si[:-1]) & (un[1:] == un[:-1])
    assert (st[1:][same] > en[:-1][same]).all()                             # disjoint and not touching
    total = int(lengths.sum())
    assert 2_200_000 < total and (total >> 11) + 1 > 1024                   # the kernel's tile count
    off = np.concatenate(([0], np.cumsum(lengths)))
    gs, ge = st + off[un], en + off[un]
    assert ((gs < CARRY_AT) & (ge > CARRY_AT)).sum() >= 3                   # straddling rows
    assert (gs == CARRY_AT - 2).any() and (gs == CARRY_AT + 2).any()
    assert (gs > CARRY_AT).sum() >= 50 and (ge < CARRY_AT).sum() >= 1000
    assert set(un.tolist()) == {0, 2}


def _compute_units(ctx):
    """Compute units of the context's device, asked of the HIP runtime the library is linked to."""
    import ctypes
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    count = ctypes.c_int(0)
    hip_device_attribute_multiprocessor_count = 63
    rc = ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(count), hip_device_attribute_multiprocessor_count,
                                                 int(ctx.device))
    assert rc == 0 and 1 <= count.value <= 4096, (rc, count.value)
    return count.value


@pytest.mark.gpu
def test_window_depth_beyond_1024_tiles_and_beyond_one_window_per_thread(ctx):
    """wd_tilescan_kernel's second turn (the carry over 1,024 tile sums) and wd_window_kernel's second turn (more
    windows than the 8 x CUs workgroups of 256 it is launched with), against the vectorised restatement.  Reached on
    an MI355X: 1,075 tiles; 550,225 windows of (4, 4) over the table as one span against 524,288 threads at 256
    compute units (with more compute units the stride shrinks until the windows outnumber the threads)."""
    from catch_amd import engine
    lengths, si, un, st, en = _big_table()
    total = int(lengths.sum())
    threads = 8 * 256 * _compute_units(ctx)
    stride = 4
    while stride > 1 and (total - 1) // stride + 1 <= threads:
        stride -= 1
    nwin = (total - 1) // stride + 1
    assert nwin > threads, (nwin, threads)
    rows = engine.Rows.from_host(ctx, si, un, st, en, lengths)
    try:
        for span_first in (np.asarray([0, 3]), np.asarray([0, 1, 2, 3]), np.asarray([2, 3])):
            for length, step in ((4, stride), (100000, 50000), (3_000_000, 1_000_000)):
                sums, counts, win_off = rows.window_depth(span_first, length, step)
                want = _expect_windows(un, st, en, lengths, span_first, length, step, restate=restate_windows_vectorised)
                assert win_off.tolist() == want[2], (span_first, length, step)
                want_sums, want_counts = np.asarray(want[0], np.uint64), np.asarray(want[1], np.uint32)
                bad = np.nonzero(sums != want_sums)[0]
                assert bad.size == 0, (span_first.tolist(), length, step, bad[:5].tolist(), sums[bad[:5]].tolist(),
                                       want_sums[bad[:5]].tolist())
                assert np.array_equal(counts, want_counts), (span_first.tolist(), length, step)
                if span_first.tolist() == [0, 3] and length == 4:
                    assert sums.size == nwin
                    past_carry = sums[CARRY_AT // step + 1:]             # windows that start beyond CARRY_AT
                    past_threads = sums[threads:]                         # windows of a thread's second turn
                    assert int(past_carry.sum()) > 0 and int(past_threads.sum()) > 0
                    print("window depth: %d positions, %d tiles (> 1024); windows (%d, %d): %d > %d threads launched; "
                          "sum of the depth beyond position %d: %d, over the windows past the first turn: %d"
                          % (total, (total >> 11) + 1, length, step, nwin, threads, CARRY_AT, int(past_carry.sum()),
                             int(past_threads.sum())))
                if length == 3_000_000:
                    assert (counts < length).all()                       # the window is longer than every span
    finally:
        rows.close()


def _write_fasta(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _sliding_lists(analyzer):
    return [[[sorted([float(k), float(v)] for k, v in analyzer.sliding_coverage[i][j][rc].items())
              for rc in (False, True)] for j in range(len(grp))] for i, grp in enumerate(analyzer.target_genomes)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_command_equals_the_recorded_reference(ctx, case, tmp_path, capsys):
    """analyze_probe_coverage.main (for the genomes of several chromosomes, which the command cannot read from a
    FASTA file, Analyzer itself) against the live reference's recorded run: sliding_coverage equal, the three files
    byte-identical, the printed report identical."""
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd import coverage_analysis, genome, probe
    out = [str(tmp_path / n) for n in ("analysis.tsv", "sliding.tsv", "counts.tsv")]
    o = case["options"]
    np.random.seed(case["np_seed"])
    capsys.readouterr()
    if case["kind"] == "cli":
        files = [_write_fasta(tmp_path / d["file"], d["records"]) for d in case["datasets"]]
        argv = ["-d"] + files + ["-f", _write_fasta(tmp_path / "probes.fasta", case["probes"]),
                                 "-m", str(o["mismatches"]), "-l", str(o["lcf_thres"]),
                                 "-e", str(o.get("cover_extension", 0)),
                                 "--island-of-exact-match", str(o.get("island_of_exact_match", 0)),
                                 "--kmer-probe-map-k", str(o.get("kmer_probe_map_k", 10)),
                                 "--print-analysis", "--write-analysis-to-tsv", out[0],
                                 "--write-sliding-window-coverage", out[1], "--write-probe-map-counts-to-tsv", out[2]]
        if o.get("limit_target_genomes"):
            argv += ["--limit-target-genomes", str(o["limit_target_genomes"])]
        (a,) = apc.main(apc.parse_args(argv))
    else:
        gens = [[genome.Genome.from_one_seq(g[0]) if len(g) == 1 else
                 genome.Genome.from_chrs(dict(("c%d" % i, x) for i, x in enumerate(g))) for g in grp]
                for grp in case["groups"]]
        a = coverage_analysis.Analyzer([probe.Probe.from_str(s) for s in case["probes"]], o["mismatches"],
                                       o["lcf_thres"], gens, case["group_names"],
                                       cover_extension=o.get("cover_extension", 0),
                                       kmer_probe_map_k=o.get("kmer_probe_map_k", 10))
        a.run()
        a.write_data_matrix_as_tsv(out[0])
        a.write_sliding_window_coverage(out[1])
        a.write_probe_map_counts(out[2])
        a.print_analysis()
    report = capsys.readouterr().out
    assert _sliding_lists(a) == case["sliding_coverage"]
    assert open(out[0]).read() == case["analysis_tsv"]
    assert open(out[1]).read() == case["sliding_tsv"]
    assert open(out[2]).read() == case["map_counts_tsv"]
    assert report == case["report"]


@pytest.mark.gpu
def test_device_windows_equal_host_windows_and_fetch_no_rows(ctx, tmp_path, monkeypatch):
    """A seeded design analysed on both strands: CATCHHIP_ANALYSIS_HOST_WINDOWS=1 (the host computation from the
    fetched ranges) and the default (the device) give equal sliding_coverage dicts and byte-identical files, for
    two window shapes; the default path calls neither Rows.fetch nor target_covers."""
    from catch_amd import coverage_analysis, engine, genome
    from catch_amd.filter import duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(91))
    groups = [[genome.Genome.from_one_seq(g[0]) for g in synthetic.make_species(rng, [3100], 4, 2, 0.04, 0.01)],
              [genome.Genome.from_chrs(dict(("c%d" % i, x) for i, x in enumerate(g)))
               for g in synthetic.make_species(rng, [1500, 700, 130], 3, 2, 0.05, 0.02)]]
    np.random.seed(9)
    pb = probe_designer.ProbeDesigner(
        groups, [duplicate_filter.DuplicateFilter(),
                 set_cover_filter.SetCoverFilter(mismatches=2, lcf_thres=100, cover_extension=30)],
        probe_length=100, probe_stride=50)
    pb.design()
    assert len(pb.final_probes) > 10

    fetches, covers = [], []
    real_fetch = engine.Rows.fetch
    real_covers = coverage_analysis.Analyzer._fetch_covers
    monkeypatch.setattr(engine.Rows, "fetch", lambda self: (fetches.append(1), real_fetch(self))[1])
    monkeypatch.setattr(coverage_analysis.Analyzer, "_fetch_covers",
                        lambda self: (covers.append(1), real_covers(self))[1])

    def analyse(tag, window):
        a = coverage_analysis.Analyzer(pb.final_probes, 2, 100, groups, ["one", "segmented"], cover_extension=30)
        a.run(*window)
        fn = str(tmp_path / ("sliding_%s_%d_%d.tsv" % ((tag,) + window)))
        a.write_sliding_window_coverage(fn)
        return a.sliding_coverage, open(fn, "rb").read()

    for window in ((50, 25), (120, 7)):
        monkeypatch.delenv("CATCHHIP_ANALYSIS_HOST_WINDOWS", raising=False)
        fetches.clear(), covers.clear()
        dev_dict, dev_file = analyse("device", window)
        assert (fetches, covers) == ([], [])
        monkeypatch.setenv("CATCHHIP_ANALYSIS_HOST_WINDOWS", "1")
        host_dict, host_file = analyse("host", window)
        assert len(fetches) == 2 and len(covers) == 1
        assert dev_dict == host_dict
        assert dev_file == host_file and len(dev_file) > 1000
        assert max(v for g in dev_dict[1].values() for d in g.values() for v in d.values()) > 0


@pytest.mark.gpu
def test_params_equals_the_datasets_analysed_one_by_one(ctx, tmp_path, capsys):
    """design_grid -> pool -> combine_pooled -> analyze_probe_coverage --params, end to end: each dataset's rows of
    the report, of the TSV and of the sliding-window file are those of the command run on that dataset alone with
    -m / -e set to its row, in -d order; the map counts are the sums; NUMBER OF PROBES is printed once."""
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd import combine_pooled, design_grid, grid, pool
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(43))
    species = [("sp_a.fasta", synthetic.make_species(rng, [2400], 4, 2, 0.05, 0.01)),
               ("sp_b.fasta", synthetic.make_species(rng, [1800], 3, 3, 0.06, 0.02)),
               ("sp_c.fasta", synthetic.make_species(rng, [1500], 4, 2, 0.04, 0.015))]
    files = [_write_fasta(tmp_path / fn, [("g%d" % j, g[0]) for j, g in enumerate(gs)]) for fn, gs in species]
    outdir, table, params = tmp_path / "grid", tmp_path / "num-probes.tsv", tmp_path / "params.tsv"
    counts = design_grid.main(design_grid.parse_args(
        files + ["--grid-mismatches", "0", "3", "--grid-cover-extension", "0", "40", "-o", str(outdir),
                 "-pl", "100", "-ps", "50", "--write-probe-count-table", str(table)]))
    per = {}
    for name, _m, _e, n in counts:
        per.setdefault(name, []).append(n)
    budget = (sum(min(v) for v in per.values()) + sum(max(v) for v in per.values())) // 2
    pool.main([str(table), str(budget), str(params)])
    pooled = tmp_path / "pooled.fasta"
    combine_pooled.main([str(params), str(outdir), "-o", str(pooled)])
    rows = dict((d, (m, e)) for d, m, e in combine_pooled.read_params(str(params)))
    assert len(set(rows.values())) > 1       # (the budget makes the datasets differ)
    capsys.readouterr()

    def run(argv, tag):
        out = [str(tmp_path / ("%s_%s" % (tag, n))) for n in ("analysis.tsv", "sliding.tsv", "counts.tsv")]
        apc.main(apc.parse_args(argv + ["-f", str(pooled), "-l", "100", "--print-analysis",
                                        "--write-analysis-to-tsv", out[0], "--write-sliding-window-coverage", out[1],
                                        "--write-probe-map-counts-to-tsv", out[2]]))
        return [open(p).read() for p in out] + [capsys.readouterr().out]

    order = [files[2], files[0], files[1]]
    tsv, sliding, mapc, report = run(["-d"] + order + ["--params", str(params)], "all")
    want_tsv, want_sliding, want_rows, want_counts, nprobes = "", "", [], {}, None
    for fn in order:
        m, e = rows[grid.dataset_name(fn)]
        t, s, c, r = run(["-d", fn, "-m", str(m), "-e", str(e)], grid.dataset_name(fn))
        want_tsv += t if not want_tsv else t.split("\n", 1)[1]
        want_sliding += s
        lines = r.splitlines()
        nprobes = lines[0]
        want_rows += [ln.split() for ln in lines[5:] if ln]
        for ln in c.splitlines()[1:]:
            ident, seq, n = ln.split("\t")
            want_counts[(ident, seq)] = want_counts.get((ident, seq), 0) + int(n)
    assert tsv == want_tsv and sliding == want_sliding and len(sliding) > 1000
    lines = report.splitlines()
    assert lines[0] == nprobes and report.count("NUMBER OF PROBES") == 1
    assert [ln.split() for ln in lines[5:] if ln] == want_rows and len(want_rows) == 2 * 11
    assert report.endswith("\n\n") and not report.endswith("\n\n\n")
    got_counts = {}
    for ln in mapc.splitlines()[1:]:
        ident, seq, n = ln.split("\t")
        assert (ident, seq) not in got_counts
        got_counts[(ident, seq)] = int(n)
    assert got_counts == want_counts and sum(got_counts.values()) > 0
