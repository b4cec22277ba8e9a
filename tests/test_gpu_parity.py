"""Parity of the HIP path (through the C ABI of libcatchhip.so) with the CPU
oracle and with golden vectors recorded from the live reference.
Bit-exact: everything here is integer/index work."""
import os
import random
import sys

import numpy as np
import pytest

from util import (candidates, load_golden, np_state_from_json, rows_as_tuples,
                  small_species)

pytestmark = pytest.mark.gpu


def _engine():
    from catch_amd import engine
    return engine


def _probe_mod():
    from catch_amd import probe
    return probe


def _scan_rows(ctx, probe_strs, genomes, m, thres, island=0, ext=0, mode=0,
               min_k=20, entries=None, k=None, merge=True):
    """Rows (set, universe, start, end) from the HIP path."""
    engine, probe = _engine(), _probe_mod()
    if entries is None:
        k, uniq, owner, ep, eo = probe.anchor_table(probe_strs, m, thres,
                                                    min_k=min_k, k=min_k)
    else:
        uniq = list(probe_strs)
        owner = np.arange(len(uniq), dtype=np.int32)
        ep = np.array([e[0] for e in entries], dtype=np.int32)
        eo = np.array([e[1] for e in entries], dtype=np.int32)
    t = engine.Targets(ctx, genomes)
    p = engine.Probes(ctx, uniq, owner, ep, eo, k)
    rows = engine.Rows.scan(ctx, p, t, m, thres, island, ext, mode, merge)
    out = rows_as_tuples(*rows.fetch())
    rows.close(); p.close(); t.close()
    return out


def _seed_scan_stats(ctx, probe_strs, genomes, entries, k, m, ext):
    """Work counters of one seed scan: raw hits and the seeds its verify launch looked at."""
    engine = _engine()
    ep = np.array([e[0] for e in entries], dtype=np.int32)
    eo = np.array([e[1] for e in entries], dtype=np.int32)
    t = engine.Targets(ctx, genomes)
    p = engine.Probes(ctx, list(probe_strs), np.arange(len(probe_strs), dtype=np.int32), ep, eo, k)
    rows = engine.Rows.scan(ctx, p, t, m, len(probe_strs[0]), 0, ext, engine.SCAN_SEED, True)
    c = ctx.counters()
    rows.close(); p.close(); t.close()
    return dict(hits=c["raw_hits"], seeds=c["seed_hits"] - c["seeds_dropped"])


def _oracle_rows(oracle, probe_strs, genomes, m, thres, island=0, ext=0,
                 min_k=20):
    k, entries = oracle.anchor_table(probe_strs, m, thres, min_k=min_k, k=min_k)
    uniq, owner = oracle._unique_last(probe_strs)
    pr, un, st, en = oracle.make_sets(uniq, entries, k, genomes, m, thres,
                                      island, ext)
    own = np.array(owner, dtype=np.int32)
    return rows_as_tuples(own[pr] if pr.size else pr, un, st, en)


# ---------------------------------------------------------------- K1
@pytest.mark.parametrize("L,stride,m,ext", [(75, 25, 2, 50), (100, 50, 2, 50),
                                            (100, 50, 3, 0), (75, 25, 0, 10),
                                            (64, 32, 1, 5), (32, 16, 0, 0),
                                            (40, 20, 1, 3),
                                            (130, 65, 4, 20)])
def test_scan_fast_matches_oracle(ctx, oracle, L, stride, m, ext):
    engine = _engine()
    genomes = small_species()
    probes = candidates(genomes, L, stride)
    exp = _oracle_rows(oracle, probes, genomes, m, L, 0, ext)
    got = _scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_FAST)
    assert got == exp
    # the seed-join + extension path must agree with the tiled Hamming kernel
    got_g = _scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_GENERAL)
    assert got_g == exp
    # ... and so must the seed scan: the key-grouped join (K1d, round 4) and, forced, the seed-list scan it replaced
    # for pigeonhole tables (K1c: still what random anchor tables and the first-seen scans take)
    got_s = _scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_SEED)
    assert got_s == exp
    assert ctx.counters()["join_hit_positions"] > 0
    os.environ["CATCHHIP_SEED_LIST"] = "1"
    try:
        got_l = _scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_SEED)
        assert ctx.counters()["join_hit_positions"] == 0
    finally:
        del os.environ["CATCHHIP_SEED_LIST"]
    assert got_l == exp


def test_seed_lookup_anchor_pair_filter_edge_cases(ctx, oracle):
    """The look-up's anchor-pair filter (-m 2, L = 100: four anchors of 25, at
    least two exact in a covered window, reported from the lowest exact one):
    copies of a window whose mismatches sit in chosen anchors -- every pattern
    of 0..3 mismatches over the four anchors --, N's on either side inside and
    outside anchors, windows at the very start / end of short sequences, and
    copies straddling the look-up's 2048-position tiles."""
    engine = _engine()
    rng = np.random.Generator(np.random.PCG64(4711))
    alpha = np.array(list("ACGT"))

    def rnd(n):
        return "".join(alpha[rng.integers(0, 4, size=n)])

    def mutate(w, positions, to_n=False):
        w = list(w)
        for q in positions:
            w[q] = "N" if to_n else alpha[(list("ACGT").index(w[q]) + 1 + rng.integers(0, 3)) % 4] if w[q] in "ACGT" else "A"
        return "".join(w)

    base = rnd(100)
    probes = [base, mutate(base, [10], to_n=True), rnd(100)]
    copies = []
    for mask in range(16):                       # which anchors get a mismatch
        hit = [a for a in range(4) if mask >> a & 1]
        for extra in (0, 1):                     # one or two mismatches in the first chosen anchor
            pos = [a * 25 + int(rng.integers(0, 25)) for a in hit]
            if extra and hit:
                pos.append(hit[0] * 25 + (pos[0] % 25 + 7) % 25)
            copies.append(mutate(base, pos))
    copies.append(mutate(base, [30], to_n=True))            # N in the target inside anchor 1
    copies.append(mutate(base, [10], to_n=True))            # the same N as probe 1 has
    copies.append(mutate(base, [3, 60], to_n=True))
    filler = lambda: rnd(int(rng.integers(3, 60)))
    seq = filler().join(copies)
    pad = rnd(2048 * 2 - len(seq) % 2048 - 40)              # the next copies straddle a tile boundary
    long_seq = seq + pad + base + rnd(13) + mutate(base, [5, 80]) + rnd(30)
    genomes = [[long_seq], [base], [base[:60] + rnd(40) + base], [rnd(20) + base], [mutate(base, [99]) + rnd(9)]]
    exp = _oracle_rows(oracle, probes, genomes, 2, 100, 0, 10)
    assert len(exp) > 30
    for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL):
        assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 10, mode) == exp, mode      # (SCAN_SEED: the join)
    # the seed-list scan with its anchor-pair filter, and through the unfiltered look-up (CATCHHIP_SEED_KEEP_ALL) --
    # the filter must not change a row
    os.environ["CATCHHIP_SEED_LIST"] = "1"
    try:
        assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 10, engine.SCAN_SEED) == exp
        os.environ["CATCHHIP_SEED_KEEP_ALL"] = "1"
        assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 10, engine.SCAN_SEED) == exp
    finally:
        os.environ.pop("CATCHHIP_SEED_KEEP_ALL", None)
        del os.environ["CATCHHIP_SEED_LIST"]


def test_seed_lookup_random_anchor_filter_edge_cases(ctx, oracle):
    """The look-up's filter for RANDOM anchor tables (round 6; -m 5, k = 20, anchors
    anywhere in [0, L - k]: a pair is reported from its lowest exact anchor, so a
    table match whose probe has an exact anchor among the two just below it, in
    the same window, is dropped before the verify kernel).  Chosen anchor
    lay-outs (adjacent, overlapping, far apart, at both ends of the probe, a
    single anchor), copies of a window with mismatches / N's placed inside
    chosen anchors and between them, windows at the ends of short sequences,
    copies straddling the look-up's 2,048-position tiles; rows must equal the
    oracle's and those of the unfiltered look-up and of the general path."""
    engine = _engine()
    rng = np.random.Generator(np.random.PCG64(90210))
    alpha = np.array(list("ACGT"))

    def rnd(n):
        return "".join(alpha[rng.integers(0, 4, size=n)])

    def mutate(w, positions, to_n=False):
        w = list(w)
        for q in positions:
            w[q] = "N" if to_n else alpha[(list("ACGT").index(w[q]) + 1 + rng.integers(0, 3)) % 4] if w[q] in "ACGT" else "A"
        return "".join(w)

    base, other, lone = rnd(100), rnd(100), rnd(100)
    with_n = mutate(base, [12], to_n=True)
    probes = [base, with_n, other, lone]
    anchors = {0: [0, 1, 2, 19, 20, 21, 40, 47, 79, 80],     # adjacent, overlapping, both ends
               1: [0, 5, 13, 30, 31, 60],                    # anchors 0 and 5 hold the probe's N
               2: [3, 40, 41, 42, 43, 80],
               3: [37]}
    entries = sorted((p, a) for p, al in anchors.items() for a in al)
    copies = []
    a0 = anchors[0]
    for mask in range(1 << len(a0)):
        if mask % 7 not in (0, 3):                            # a spread of the 1,024 patterns
            continue
        # break exactly the anchors of `mask` where that is possible with a mismatch of their own
        pos = []
        for j, a in enumerate(a0):
            if mask >> j & 1:
                pos.append(a + int(rng.integers(0, 20)))
        pos = sorted(set(pos))[:5]
        copies.append(mutate(base, pos))
    for q in ([], [25], [25, 70], [0], [99], [39, 40], [59, 60, 61]):
        copies.append(mutate(base, q))
        copies.append(mutate(other, q))
        copies.append(mutate(lone, q))
    copies.append(mutate(base, [22], to_n=True))              # N in the target inside anchors 19-21 and 20
    copies.append(mutate(base, [12], to_n=True))              # the same N as probe 1 has
    copies.append(mutate(base, [12, 90], to_n=True))
    copies.append(mutate(with_n, [33]))
    filler = lambda: rnd(int(rng.integers(1, 70)))
    seq = filler().join(copies)
    pad = rnd(2048 * 3 - len(seq) % 2048 - 37)                # the next copies straddle a tile boundary
    long_seq = seq + pad + base + rnd(11) + mutate(base, [5, 85]) + other + rnd(30)
    genomes = [[long_seq], [base], [base[:60] + rnd(40) + base], [rnd(20) + other], [mutate(base, [99]) + rnd(9)],
               [lone[1:] + "A"], [lone]]
    pr, un, st, en = oracle.make_sets(probes, entries, 20, genomes, 5, 100, 0, 10)
    exp = rows_as_tuples(pr, un, st, en)
    assert len(exp) > 60
    for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL):
        assert _scan_rows(ctx, probes, genomes, 5, 100, 0, 10, mode, entries=entries, k=20) == exp, mode
    os.environ["CATCHHIP_SEED_RANDOM_KEEP_ALL"] = "1"
    try:
        assert _scan_rows(ctx, probes, genomes, 5, 100, 0, 10, engine.SCAN_SEED, entries=entries, k=20) == exp
    finally:
        del os.environ["CATCHHIP_SEED_RANDOM_KEEP_ALL"]
    # the filter does drop matches: seeds verified with and without it
    st_f = _seed_scan_stats(ctx, probes, genomes, entries, 20, 5, 10)
    os.environ["CATCHHIP_SEED_RANDOM_KEEP_ALL"] = "1"
    try:
        st_u = _seed_scan_stats(ctx, probes, genomes, entries, 20, 5, 10)
    finally:
        del os.environ["CATCHHIP_SEED_RANDOM_KEEP_ALL"]
    assert st_f["hits"] == st_u["hits"] and 0 < st_f["seeds"] < 0.5 * st_u["seeds"], (st_f, st_u)


def test_scan_fast_no_n_two_planes(ctx, oracle):
    engine = _engine()
    genomes = small_species(seed=5, with_n=False)
    probes = candidates(genomes, 100, 50)
    exp = _oracle_rows(oracle, probes, genomes, 2, 100, 0, 50)
    assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 50, engine.SCAN_FAST) == exp
    assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 50, engine.SCAN_SEED) == exp


@pytest.mark.parametrize("L,stride,m,thres,island,ext,seed", [
    (75, 25, 2, 60, 0, 0, 11),      # lcf_thres < L  -> random anchors
    (100, 50, 5, 100, 0, 50, 12),   # pigeonhole k < 20 -> random anchors
    (75, 25, 2, 75, 30, 0, None),   # island of exact match
    (100, 50, 3, 80, 25, 10, 13),
    (75, 25, 1, 40, 0, 3, 14),
    (100, 50, 6, 100, 0, 20, 15),   # random anchors, full-length threshold, more mismatches
    (60, 30, 4, 60, 0, 0, 16),
])
def test_scan_general_matches_oracle(ctx, oracle, L, stride, m, thres, island,
                                     ext, seed):
    genomes = small_species(seed=21)
    probes = candidates(genomes, L, stride)
    if seed is not None:
        np.random.seed(seed)
    exp = _oracle_rows(oracle, probes, genomes, m, thres, island, ext)
    if seed is not None:
        np.random.seed(seed)
    got = _scan_rows(ctx, probes, genomes, m, thres, island, ext)
    assert got == exp
    if thres == L and island == 0:
        # full-length threshold: the seed scan takes any anchor table (here the
        # reference's random anchors) and must agree with the seed join
        engine = _engine()
        for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL):
            if seed is not None:
                np.random.seed(seed)
            assert _scan_rows(ctx, probes, genomes, m, thres, island, ext, mode) == exp


@pytest.mark.parametrize("copies", [40, 700, 9000])
def test_scan_repeats_fill_large_buckets(ctx, oracle, copies):
    """A unit repeated `copies` times: the probes inside the unit hit every
    copy, so their row-build buckets exceed what one wavefront (512 hits) and
    one workgroup (8192) sort -- the wave, workgroup and radix-sort builds must
    all give the reference's rows, in every scan mode."""
    engine = _engine()
    rng = random.Random(copies)
    def rs(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    unit = rs(150)
    g0 = "".join(unit + rs(30) for _ in range(copies))
    genomes = [[g0], [rs(400) + unit + rs(300)]]
    probes = candidates([[unit + rs(50)], [g0[:2000]]], 100, 25)
    exp = _oracle_rows(oracle, probes, genomes, 2, 100, 0, 20)
    assert max(np.bincount([r[0] for r in exp])) >= min(copies, 2)
    for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL, engine.SCAN_FAST):
        assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 20, mode) == exp
    if copies == 700:
        # tolerant-bp accounting goes through the same bucket build
        p_mod = _probe_mod()
        k, uniq, owner, ep, eo = p_mod.anchor_table(probes, 2, 100)
        t = engine.Targets(ctx, genomes)
        p = engine.Probes(ctx, uniq, owner, ep, eo, k)
        out = np.zeros(len(uniq), dtype=np.int64)
        engine.tolerant_bp(ctx, p, t, 2, 100, 0, out)
        rows = _scan_rows(ctx, probes, [[s] for g in genomes for s in g], 2, 100, 0, 0)
        want = np.zeros(len(probes), dtype=np.int64)
        for sid, _, a, b in rows:
            want[sid] += b - a
        own = np.array(owner)
        assert np.array_equal(out, want[own])
        p.close(); t.close()


def test_scan_multi_chromosome_and_short_sequences(ctx, oracle):
    """Genome coordinates across chromosomes (set_cover_filter.py:429-453),
    sequences shorter than the probe and than k, empty sequences."""
    rng = random.Random(3)
    def rs(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    base = rs(400)
    genomes = [[base[:150], base[150:], rs(30)], [base[10:300]], [rs(8), ""],
               [base[100:160]]]
    probes = candidates([[base]], 50, 10)
    for m, thres in ((1, 50), (2, 30)):
        np.random.seed(1)
        exp = _oracle_rows(oracle, probes, genomes, m, thres, 0, 7, min_k=10)
        np.random.seed(1)
        got = _scan_rows(ctx, probes, genomes, m, thres, 0, 7, min_k=10)
        assert got == exp


def test_scan_arbitrary_alphabet(ctx, oracle):
    """Character equality on any byte alphabet (the reference's toy tests use
    A-Z; lower case differs from upper case)."""
    rng = random.Random(9)
    alpha = "ABCDEFGHIJKLMNOPQRSTUVWXYZacgt"
    seq = "".join(rng.choice(alpha) for _ in range(600))
    genomes = [[seq], [seq[100:400].lower() + seq[400:]]]
    probes = [seq[i:i + 20] for i in range(0, 580, 7)]
    exp = _oracle_rows(oracle, probes, genomes, 1, 20, 0, 2, min_k=5)
    got = _scan_rows(ctx, probes, genomes, 1, 20, 0, 2, min_k=5)
    assert got == exp


def test_scan_reference_test_vectors(ctx):
    """The reference's own scan known answers (catch/tests/test_probe.py),
    recorded as data."""
    recs = [c for c in load_golden("scan") if c["merge"]]
    assert len(recs) >= 20
    for c in recs:
        got = _scan_rows(ctx, c["probes"], [[c["sequence"]]], c["mismatches"],
                         c["lcf_thres"], c["island"], 0,
                         entries=c["entries"], k=c["k"])
        exp = sorted((int(p), 0, s, e) for p, v in c["out"].items()
                     for s, e in v)
        assert got == exp, (c["probes"], c["sequence"][:60])


def _occurrences(text, pat):
    n, at = 0, text.find(pat)
    while at >= 0:
        n += 1
        at = text.find(pat, at + 1)
    return n


def test_extension_replays_the_reference_lcs_and_lcf_vectors(ctx):
    """a7 / a8 on the DEVICE, vector by vector: every recorded answer of the
    reference's k_lcf_around_anchor (its own tests' cases + 3,000 random ones,
    tests/golden/lcs_anchor.json.gz) and of its lcf cover function
    (lcf_cover.json.gz) that can be posed as a scan of one window -- probe and
    window aligned at 0, the anchor k-mer the probe's only table entry and
    found nowhere else in the window -- goes through catchhip_cover_scan's
    extension kernel and must come back as recorded (catch/utils/
    longest_common_substring.py:59-159, catch/probe.py:1328-1344)."""
    g = load_golden("lcs_anchor")
    done = 0
    for c in g["from_reference_tests"] + g["random"]:
        a, b, s0, e0, k = c["a"], c["b"], c["anchor_start"], c["anchor_end"], c["k"]
        if len(a) != len(b) or e0 - s0 < 1 or a[s0:e0] != b[s0:e0] or _occurrences(b, a[s0:e0]) != 1:
            continue
        length, start = c["out"]
        got = _scan_rows(ctx, [a], [[b]], k, 1, 0, 0, entries=[(0, s0)], k=e0 - s0)
        assert got == [(0, 0, start, start + length)], c
        done += 1
    assert done >= 2400
    done = 0
    for c in load_golden("lcf_cover"):
        pr, sq, s0, e0 = c["probe_seq"], c["sequence"], c["kmer_start"], c["kmer_end"]
        if (c["full_probe_len"] != len(pr) or c["full_sequence_len"] != len(sq) or len(pr) > len(sq)
                or pr[s0:e0] != sq[s0:e0] or _occurrences(sq, pr[s0:e0]) != 1):
            continue
        got = _scan_rows(ctx, [pr], [[sq]], c["mismatches"], c["lcf_thres"], c["island"], 0,
                         entries=[(0, s0)], k=e0 - s0)
        exp = [] if c["out"] is None else [(0, 0, c["out"][0], c["out"][1])]
        assert got == exp, c
        done += 1
    assert done >= 8


def test_cover_ranges_unmerged(ctx, oracle):
    """catchhip_cover_ranges = find_probe_covers_in_sequence(merge_overlapping=
    False): the reference's unmerged known answers, and the oracle on repeats
    (overlapping ranges of one probe stay apart, duplicates collapse)."""
    engine = _engine()
    recs = load_golden("coverage_analysis")["scans_unmerged"]
    assert len(recs) >= 50
    for c in recs:
        got = _scan_rows(ctx, c["probes"], [[c["sequence"]]], c["mismatches"],
                         c["lcf_thres"], c["island"], 0,
                         entries=c["entries"], k=c["k"], merge=False)
        exp = sorted((int(p), 0, s, e) for p, v in c["out"].items()
                     for s, e in v)
        assert got == exp, (c["probes"], c["sequence"][:60])
    rng = random.Random(17)
    unit = "".join(rng.choice("ACGT") for _ in range(60))
    seq = unit * 12 + "".join(rng.choice("ACGT") for _ in range(200)) + unit * 3
    probes = candidates([[seq]], 50, 10)
    for m, thres, mode in ((1, 50, engine.SCAN_AUTO), (2, 35, engine.SCAN_AUTO),
                           (1, 50, engine.SCAN_GENERAL), (1, 50, engine.SCAN_FAST)):
        np.random.seed(3)
        k, entries = oracle.anchor_table(probes, m, thres, min_k=10, k=10)
        uniq, owner = oracle._unique_last(probes)
        cov = oracle.scan_sequence(seq, uniq, entries, k, m, thres, 0, merge=False)
        exp = sorted((int(owner[p]), 0, max(0, a - 5), min(len(seq), b + 5))
                     for p, v in cov.items() for a, b in v)
        exp = sorted(set(exp))
        np.random.seed(3)
        got = _scan_rows(ctx, probes, [[seq]], m, thres, 0, 5, mode, min_k=10,
                         merge=False)
        assert got == exp, (m, thres, mode)
        merged = _scan_rows(ctx, probes, [[seq]], m, thres, 0, 5, mode, min_k=10)
        assert len(merged) < len(got)


def test_scan_empty_inputs(ctx):
    engine = _engine()
    assert _scan_rows(ctx, [], [["ACGT" * 30]], 1, 10) == []
    assert _scan_rows(ctx, ["ACGTACGTAC"], [], 0, 10, min_k=5) == []
    assert _scan_rows(ctx, ["ACGTACGTAC"], [[""]], 0, 10, min_k=5) == []
    with pytest.raises(ValueError):
        t = engine.Targets(ctx, [["AC"]])
        p = engine.Probes(ctx, ["ACGTACGTAC"], [0], [0], [0], 5)
        engine.Rows.scan(ctx, p, t, 2, 60, 0, 0, engine.SCAN_FAST)


# ---------------------------------------------------------------- K2
def _partial_solver(monkeypatch, solver):
    """Which solver takes instances with universe_p < 1: the frontier rounds of
    the row-parallel kernels with the universe test (default), or the
    persistent-workgroup solver (eager re-count; the lazy-evaluation variant of
    round 3 was a measured dead end and is gone)."""
    if solver != "frontier":
        monkeypatch.setenv("CATCHHIP_PARTIAL_SEQUENTIAL", "1")


@pytest.mark.parametrize("solver", ["frontier", "eager"])
def test_greedy_reference_test_vectors(ctx, monkeypatch, solver):
    """set_cover.approx_multiuniverse known answers
    (catch/utils/tests/test_set_cover.py), unit-cost instances; partial
    coverage through each of the three solvers that take it."""
    engine = _engine()
    _partial_solver(monkeypatch, solver)
    recs = load_golden("setcover")
    n = 0
    for c in recs:
        if c["costs"] is not None and any(x != 1.0 for x in c["costs"]):
            continue
        r = np.array(c["rows"], dtype=np.int64).reshape(-1, 4)
        U = c["num_universes"]
        glen = np.zeros(U, dtype=np.int64)
        for u in range(U):
            sel = r[:, 1] == u
            glen[u] = r[sel, 3].max() if sel.any() else 0
        rows = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = rows.greedy(c["num_sets"], c["ranks"], c["universe_p"])
        rows.close()
        assert sorted(got) == c["out"], c
        n += 1
    assert n >= 20


@pytest.mark.parametrize("solver", ["frontier", "eager"])
def test_greedy_random_instances_match_oracle(ctx, oracle, monkeypatch, solver):
    engine = _engine()
    _partial_solver(monkeypatch, solver)
    rng = np.random.Generator(np.random.PCG64(123))
    for trial in range(30):
        P = int(rng.integers(1, 60))
        U = int(rng.integers(1, 6))
        glen = rng.integers(50, 400, size=U)
        rows = []
        for s in range(P):
            for u in range(U):
                if rng.random() < 0.6:
                    ivs, pos = [], int(rng.integers(0, 30))
                    for _ in range(int(rng.integers(1, 4))):
                        ln = int(rng.integers(1, 40))
                        if pos + ln > glen[u]:
                            break
                        ivs.append((pos, pos + ln))
                        pos += ln + int(rng.integers(1, 50))
                    rows += [(s, u, a, b) for a, b in ivs]
        if not rows:
            continue
        r = np.array(sorted(rows), dtype=np.int64)
        ranks = rng.integers(0, 3, size=P) if trial % 2 else None
        up = [float(x) for x in rng.choice([1.0, 0.9, 0.5, 0.25, 0.0], size=U)] \
            if trial % 3 else None
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P,
                                          U, None, up, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, up)
        dev.close()
        # same picks in the same (sequential) order, whichever solver ran
        assert got == exp, trial


@pytest.mark.parametrize("how", ["by rows", "round robin", "by rows, 2 workgroups per CU", "by rows, 16 tiles at least"])
def test_flat_solver_tiles_dealt_to_xcds(ctx, oracle, monkeypatch, how):
    """The row-parallel solver's tiles on the XCDs (round 6): ~250 contiguous tiles of very different row counts --
    a dense half and a sparse half of the coordinate space, some tiles empty -- dealt by rows (the default: largest
    tile first, to the XCD with the fewest rows so far, at most 32 tiles per XCD), dealt round robin (tile t on XCD
    t mod 8, as until round 6), with other grid sizes and tile counts: always the oracle's picks in its order, with
    and without ranks, at full and at partial coverage."""
    engine = _engine()
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0")
    monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "12")          # (raised by the library until there are < 256 tiles)
    if how == "round robin":
        monkeypatch.setenv("CATCHHIP_FLAT_TILES_ROUND_ROBIN", "1")
    if "2 workgroups" in how:
        monkeypatch.setenv("CATCHHIP_FLAT_WG_PER_CU", "2")
    if "16 tiles" in how:
        monkeypatch.setenv("CATCHHIP_FLAT_MIN_TILES", "16")
    rng = np.random.Generator(np.random.PCG64(20260930))
    for trial in range(3):
        U = 40
        glen = rng.integers(20000, 60000, size=U)
        P = int(rng.integers(1500, 3000))
        rows = []
        for s in range(P):
            # sets of the dense half cover many universes of the first 20, the others one or two of the last 20;
            # universes 30-33 are covered by nobody but one set each (nearly empty tiles)
            dense = s % 3 != 0
            us = rng.choice(20, size=int(rng.integers(4, 12)), replace=False) if dense else 20 + rng.choice(10, size=int(rng.integers(1, 3)), replace=False)
            for u in sorted(int(x) for x in us):
                pos = int(rng.integers(0, glen[u] - 300))
                ln = int(rng.integers(30, 257))
                rows.append((s, u, pos, pos + ln))
        for u in range(30, 34):
            rows.append((int(rng.integers(0, P)), u, 100, 180))
        r = np.array(sorted(set(rows)), dtype=np.int64)
        ranks = rng.integers(0, 3, size=P) if trial == 1 else None
        up = [float(rng.choice([1.0, 0.9, 0.5])) for _ in range(U)] if trial == 2 else None
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, U, None, up, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, up)
        cn = ctx.counters()
        dev.close()
        assert cn["flat_rows_streamed"] > 0
        assert got == exp, (how, trial)


@pytest.mark.parametrize("flat", [False, True, "lds", "contiguous", "contiguous-lds"])
def test_greedy_batched_rounds_restore_sequential_order(ctx, oracle, monkeypatch, flat):
    """Larger full-coverage instances (many locally maximal sets per round,
    with and without ranks): the frontier solver -- set-parallel fused kernels
    and, forced here on these small instances, the row-parallel kernels large
    instances take -- must return the oracle's sequential pick order, and so
    must the one-pick-per-iteration solver.  The row-parallel kernels run with
    striped and with contiguous tiles, and ("lds" variants, named for the
    round-3 cache they replaced) with the E_dirty statistics collected -- the
    changed-word bits the apply launch then marks and the count launch reads."""
    engine = _engine()
    monkeypatch.setenv("CATCHHIP_FLAT_MIN_ROWS", "0" if flat else str(1 << 40))
    if flat in ("lds", "contiguous-lds"):
        monkeypatch.setenv("CATCHHIP_FLAT_COUNT_DIRTY", "1")
    if flat in ("contiguous", "contiguous-lds"):
        monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "16")
    rng = np.random.Generator(np.random.PCG64(321))
    for trial in range(6):
        P = int(rng.integers(300, 2500))
        U = int(rng.integers(1, 12))
        glen = rng.integers(2000, 9000, size=U)
        rows = []
        for s in range(P):
            for u in range(U):
                if rng.random() < 0.5:
                    pos = int(rng.integers(0, glen[u] - 300))
                    for _ in range(int(rng.integers(1, 3))):
                        ln = int(rng.integers(1, 257))
                        if pos + ln > glen[u]:
                            break
                        rows.append((s, u, pos, pos + ln))
                        pos += ln + int(rng.integers(1, 200))
        r = np.array(sorted(rows), dtype=np.int64)
        ranks = rng.integers(0, 4, size=P) if trial % 2 else None
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P,
                                          U, None, None, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, None)
        cn = ctx.counters()
        rounds = cn["greedy_iters"]
        if flat:
            assert 0 < cn["flat_rows_recounted"] <= cn["flat_rows_streamed"]
        else:
            assert cn["flat_rows_streamed"] == 0
        os.environ["CATCHHIP_GREEDY_SEQUENTIAL"] = "1"
        try:
            got_seq = dev.greedy(P, ranks, None)
        finally:
            del os.environ["CATCHHIP_GREEDY_SEQUENTIAL"]
        dev.close()
        assert got == exp, trial
        assert got_seq == exp, trial
        assert rounds < len(exp)      # really batched


def test_sequential_solver_partial_cover_many_universes(ctx, oracle, monkeypatch):
    """The persistent-workgroup solver on sets that touch thousands of universes,
    with partial coverage (min(left, count) binds at the end of every universe),
    ranks, and rows longer than five bitmap words (which the frontier rounds do
    not take under partial coverage): the oracle's picks in its order."""
    engine = _engine()
    _partial_solver(monkeypatch, "eager")
    rng = np.random.Generator(np.random.PCG64(2024))
    for trial in range(3):
        P, U = 40, 4500 + 700 * trial
        glen = rng.integers(300, 700, size=U)
        rows = []
        for s in range(P):
            dens = 1.0 if s < 3 else rng.uniform(0.05, 0.6)
            for u in np.nonzero(rng.random(U) < dens)[0]:
                pos = int(rng.integers(0, glen[u] - 60))
                ln = int(rng.integers(20, 400 if s % 5 == 0 else 60))
                rows.append((s, int(u), pos, min(pos + ln, int(glen[u]))))
        r = np.array(sorted(rows), dtype=np.int64)
        ranks = rng.integers(0, 2, size=P) if trial == 1 else None
        up = [float(x) for x in rng.choice([1.0, 0.9, 0.5], size=U)]
        exp = oracle.lazy_greedy(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, glen, up, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, up)
        cn = ctx.counters()
        dev.close()
        assert got == exp, trial
        assert cn["rows_recounted"] >= len(exp)


@pytest.mark.parametrize("tiles", ["striped", "contiguous"])
def test_partial_cover_frontier_rounds_match_oracle(ctx, oracle, monkeypatch, tiles):
    """universe_p < 1 through the frontier rounds of the row-parallel kernels
    (per-row min(need, count), complex sets through gr_fixup, the universe test
    of gr_apply with the thresholds of gr_usel, finished universes dropping
    out): instances shaped like a design -- many universes of similar genomes,
    sets with one row in most universes and now and then two in one -- with
    p in {0.9, 0.5, mixed incl. 1.0 and 0}, with and without ranks.  The picks
    and their ORDER are the oracle's."""
    engine = _engine()
    if tiles == "contiguous":
        monkeypatch.setenv("CATCHHIP_FLAT_TILE_SHIFT", "16")
        monkeypatch.setenv("CATCHHIP_FLAT_COUNT_DIRTY", "1")
    rng = np.random.Generator(np.random.PCG64(4242))
    for trial in range(6):
        U = int(rng.integers(20, 90))
        base_len = int(rng.integers(1500, 5000))
        glen = base_len + rng.integers(-40, 40, size=U)
        P = int(base_len // 25)
        rows = []
        for s in range(P):
            centre = int(rng.integers(0, base_len - 260))
            hit = rng.random(U) < rng.uniform(0.2, 0.9)
            for u in np.nonzero(hit)[0]:
                pos = min(max(0, centre + int(rng.integers(-15, 15))), int(glen[u]) - 257)
                ln = int(rng.integers(100, 257))
                rows.append((s, int(u), pos, pos + ln))
                if rng.random() < 0.04 and pos + ln + 40 + 120 < glen[u]:      # a second row in the same universe
                    rows.append((s, int(u), pos + ln + 40, pos + ln + 40 + int(rng.integers(30, 120))))
        r = np.array(sorted(set(rows)), dtype=np.int64)
        ranks = rng.integers(0, 3, size=P) if trial % 3 == 2 else None
        up = ([0.9] * U if trial % 3 == 0 else [0.5] * U if trial % 3 == 1 else
              [float(x) for x in rng.choice([1.0, 0.9, 0.7, 0.0], size=U)])
        exp = oracle.lazy_greedy(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, glen, up, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, up)
        cn = ctx.counters()
        dev.close()
        assert got == exp, (trial, len(got), len(exp))
        assert cn["flat_rows_streamed"] > 0                    # the row-parallel kernels ran
        # every round makes at least one pick (the set with the largest key passes the universe test)
        assert cn["greedy_iters"] <= len(exp) + 2, (trial, cn["greedy_iters"], len(exp))


@pytest.mark.parametrize("force_long", [False, True])
def test_greedy_long_rows_take_the_frontier_path(ctx, oracle, monkeypatch, force_long):
    """Rows of more than 257 bases (up to 40 bitmap words) go through the
    lane-per-word round kernels (gfl_*), in both set widths (16 lanes: few rows
    per set, 64 lanes: many), still in rounds and still the oracle's order;
    forced on short rows they must agree with the lane-per-row kernels."""
    engine = _engine()
    if force_long:
        monkeypatch.setenv("CATCHHIP_GF_LONG", "1")
    rng = np.random.Generator(np.random.PCG64(777 + force_long))
    for trial in range(6):
        P = int(rng.integers(200, 1500))
        U = int(rng.integers(1, 5)) if trial % 2 else int(rng.integers(40, 90))
        glen = rng.integers(4000, 12000, size=U)
        maxlen = 250 if force_long else int(rng.choice([300, 600, 2500]))
        rows = []
        for s in range(P):
            for u in range(U):
                if rng.random() < (0.5 if U < 10 else 0.7):
                    pos = int(rng.integers(0, glen[u] - maxlen - 1))
                    for _ in range(int(rng.integers(1, 3))):
                        ln = int(rng.integers(1, maxlen + 1))
                        if pos + ln > glen[u]:
                            break
                        rows.append((s, u, pos, pos + ln))
                        pos += ln + int(rng.integers(1, 200))
        r = np.array(sorted(rows), dtype=np.int64)
        ranks = rng.integers(0, 3, size=P) if trial % 3 == 0 else None
        exp = oracle.lazy_greedy(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, glen,
                                 None, ranks)
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        got = dev.greedy(P, ranks, None)
        rounds = ctx.counters()["greedy_iters"]
        dev.close()
        assert got == exp, trial
        assert rounds < len(exp), (rounds, len(exp))      # rounds, not one pick per iteration
        if not force_long:
            assert int((r[:, 3] - r[:, 2]).max()) > 257


# ---------------------------------------------------------------- SCF
def _run_filter(c):
    from catch_amd import genome, probe
    from catch_amd.filter import set_cover_filter as scf
    import tempfile, os
    paths = []
    if c["avoided_sequences"]:
        fd, path = tempfile.mkstemp(suffix=".fasta")
        with os.fdopen(fd, "w") as f:
            for i, s in enumerate(c["avoided_sequences"]):
                f.write(">a%d\n%s\n" % (i, s))
        paths.append(path)
    f = scf.SetCoverFilter(
        mismatches=c["mismatches"], lcf_thres=c["lcf_thres"],
        island_of_exact_match=c["island"],
        mismatches_tolerant=c["mismatches_tolerant"],
        lcf_thres_tolerant=c["lcf_thres_tolerant"],
        island_of_exact_match_tolerant=c["island_tolerant"],
        identify=c["identify"], avoided_genomes=paths, coverage=c["coverage"],
        cover_extension=c["cover_extension"],
        kmer_probe_map_k=c["kmer_probe_map_k"])
    probes = [[probe.Probe.from_str(s) for s in g] for g in c["probes"]]
    genomes = [[genome.Genome.from_one_seq(g[0]) if len(g) == 1 else
                genome.Genome(list(g), chrs=dict((str(i), s) for i, s in enumerate(g)))
                for g in grp] for grp in c["genomes"]]
    if "np_random_state" in c:
        np.random.set_state(np_state_from_json(c["np_random_state"]))
    out = f.filter(probes, genomes, input_is_grouped=True)
    for p in paths:
        os.remove(p)
    # identity: outputs are the very input objects
    for g_out, g_in in zip(out, probes):
        ids = set(id(p) for p in g_in)
        assert all(id(p) in ids for p in g_out)
    return [sorted(p.seq_str for p in g) for g in out]


@pytest.mark.parametrize("name", ["scf_reference_tests", "scf_synthetic"])
def test_set_cover_filter_golden(ctx, name):
    """SetCoverFilter.filter() through the plugin surface: selected probe sets
    identical to the reference's on the same inputs."""
    recs = load_golden(name)
    assert len(recs) >= 5
    for c in recs:
        assert _run_filter(c) == c["out"], (name, c.get("name"))


def test_set_cover_filter_matches_oracle_medium(ctx, oracle):
    """30-genome two-species input (S2 at scale 0.3): picks equal the oracle's."""
    from catch_amd.utils import synthetic
    groups = synthetic.dataset("S2", scale=0.3)
    probes = [candidates(g, 100, 50) for g in groups]
    exp = oracle.set_cover_filter(probes, groups, 2, 100, coverage=1.0,
                                  cover_extension=50)
    c = dict(mismatches=2, lcf_thres=100, island=0, mismatches_tolerant=2,
             lcf_thres_tolerant=100, island_tolerant=0, identify=False,
             avoided_sequences=[], coverage=1.0, cover_extension=50,
             kmer_probe_map_k=20, probes=probes, genomes=groups)
    got = _run_filter(c)
    assert got == [sorted(probes[gi][i] for i in ids) for gi, ids in enumerate(exp)]


def test_full_size_properties(ctx):
    """BASELINE config 2 at full size (S2, ~1.56 Mbp): checks that do not need
    the oracle -- the two independent device scans agree row for row, the
    chosen probes cover every universe completely (coverage 1.0), no chosen
    probe is redundant at the moment it was picked, and the run is
    deterministic."""
    engine, probe = _engine(), _probe_mod()
    from catch_amd.utils import synthetic
    groups = synthetic.dataset("S2")
    for genomes in groups:
        cand = candidates(genomes, 100, 50)
        k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
        t = engine.Targets(ctx, genomes)
        p = engine.Probes(ctx, uniq, owner, ep, eo, k)
        rf = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50, engine.SCAN_FAST)
        rg = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50, engine.SCAN_GENERAL)
        a, b = rf.fetch(), rg.fetch()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        rs = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50, engine.SCAN_SEED)
        assert all(np.array_equal(x, y) for x, y in zip(a, rs.fetch()))
        rs.close()
        picks = rf.greedy(len(cand))
        assert picks == rf.greedy(len(cand))
        assert len(set(picks)) == len(picks)
        sid, un, st, en = a
        glen = np.array([sum(len(s) for s in g) for g in genomes])
        base = np.concatenate([[0], np.cumsum(glen)])
        tot = int(base[-1])
        def cover(mask):
            d = np.zeros(tot + 1, dtype=np.int64)
            np.add.at(d, base[un[mask]] + st[mask], 1)
            np.add.at(d, base[un[mask]] + en[mask], -1)
            return np.cumsum(d)[:-1] > 0
        all_cov = cover(np.ones(sid.size, dtype=bool))
        sel_cov = cover(np.isin(sid, picks))
        assert np.array_equal(all_cov, sel_cov)
        # dropping the last pick must leave something uncovered
        less = cover(np.isin(sid, picks[:-1]))
        assert less.sum() < sel_cov.sum()
        rf.close(); rg.close(); p.close(); t.close()


# ---------------------------------------------------------------- K3
def test_ndf_hamming_golden(ctx):
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    g = load_golden("ndf_hamming")
    recs = g["from_reference_tests"] + g["synthetic"]
    assert len(recs) >= 3
    for c in recs:
        f = ndf.NearDuplicateFilterWithHammingDistance(c["dist_thres"], c["dim"])
        f.k = c["k"]
        f.reporting_prob = c["reporting_prob"]
        f._draw_positions = lambda c=c: c["positions"]
        inp = [probe.Probe.from_str(s) for s in c["probes"]]
        out = f.filter(inp)
        assert sorted(p.seq_str for p in out) == c["out"]
        if "seed" in c:   # positions drawn from `random` like the reference
            random.seed(c["seed"])
            f2 = ndf.NearDuplicateFilterWithHammingDistance(c["dist_thres"], c["dim"])
            assert f2._draw_positions() == c["positions"]


def test_ndf_hamming_matches_oracle_large(ctx, oracle):
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(31))
    sp = synthetic.make_species(rng, [6000], 40, 4, 0.03, 0.01, with_n=True)
    strs = candidates(sp, 100, 25, dedup=False)
    random.seed(99)
    pos = oracle.lsh_draw_positions(oracle.lsh_num_tables(3, 100, 20), 20, 100)
    exp = oracle.ndf_hamming(strs, 3, pos)
    f = ndf.NearDuplicateFilterWithHammingDistance(3, 100)
    random.seed(99)
    out = f.filter([probe.Probe.from_str(s) for s in strs])
    assert [p.seq_str for p in out] == exp
    assert len(exp) < len(set(strs))


# ---------------------------------------------------------------- RCCL path
def test_greedy_rccl_solver_single_rank_matches(ctx, oracle):
    """A context with a (one-rank) communicator solves a whole instance like
    any other context: the same picks in the same order as the oracle and as
    a context without one."""
    engine = _engine()
    c2 = engine.Context(0)
    with pytest.raises(ValueError):
        c2.comm_selftest()                    # no communicator yet
    c2.comm_init(engine.Context.comm_unique_id(), 1, 0)
    c2.comm_selftest()                        # a checked SUM all-reduce through the pinned RCCL (1 rank: sum == 1)
    c2.comm_selftest(3)
    rng = np.random.Generator(np.random.PCG64(321))
    for trial in range(6):
        P, U = int(rng.integers(5, 80)), int(rng.integers(1, 5))
        glen = rng.integers(80, 500, size=U)
        rows = []
        for s in range(P):
            for u in range(U):
                if rng.random() < 0.7:
                    a = int(rng.integers(0, glen[u] - 40))
                    rows.append((s, u, a, a + int(rng.integers(1, 40))))
        r = np.array(sorted(rows), dtype=np.int64)
        ranks = rng.integers(0, 2, size=P) if trial % 2 else None
        up = [0.8] * U if trial % 3 == 0 else None
        exp = oracle.approx_multiuniverse(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P, U,
                                          None, up, ranks)
        dev = engine.Rows.from_host(c2, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        assert dev.greedy(P, ranks, up) == exp
        dev.close()
        dev = engine.Rows.from_host(ctx, r[:, 0], r[:, 1], r[:, 2], r[:, 3], glen)
        assert dev.greedy(P, ranks, up) == exp
        dev.close()
    c2.close()


def _sharded_picks(engine, ctx, probes, genomes, bounds, n_sets, ranks, exchange_of, universe_p=None):
    """Universe-sharded solve: one targets / rows / shard triple per genome
    range, driven by the product's round loop."""
    from catch_amd import parallel
    held, shards = [], []
    try:
        for v in range(len(bounds) - 1):
            t = engine.Targets(ctx, genomes[bounds[v]:bounds[v + 1]])
            held.append(t)
            rows = engine.Rows.scan(ctx, probes, t, 2, 100, 0, 50)
            held.append(rows)
            up = None if universe_p is None else universe_p[bounds[v]:bounds[v + 1]]
            # partial-ness is the INSTANCE's: a shard whose own universes all want full cover is
            # still built as a partial shard -- the same kernels and round shape on every rank
            part = universe_p is not None and any(p < 1.0 for p in universe_p)
            shards.append(engine.Shard(rows, n_sets, ranks, up if part else None, instance_partial=part))
            assert shards[-1].partial_instance == part
        return parallel.sharded_solve(shards, exchange_of(shards))
    finally:
        for h in shards + held[::-1]:
            h.close()


@pytest.mark.parametrize("partial", [0, 1])
@pytest.mark.parametrize("with_ranks", [False, True])
def test_universe_sharded_solver_equals_unsharded(ctx, oracle, with_ranks, partial):
    """One group cut into 1, 2, 3 and 5 universe ranges (split_universes), each
    scanned and held by its own shard, solved in rounds with the two
    all-reduces per round (here: between shards of this process): the picks
    and their order equal the unsharded solver's and the oracle's.
    partial = 0: full coverage, and the one refusal; 1: partial coverage."""
    from catch_amd import parallel
    engine, probe = _engine(), _probe_mod()
    rng = np.random.Generator(np.random.PCG64(99))
    from catch_amd.utils import synthetic
    genomes = synthetic.make_species(rng, [6000], 23, 3, 0.06, 0.012)
    cand = candidates(genomes, 100, 50)
    k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
    p = engine.Probes(ctx, uniq, owner, ep, eo, k)
    t = engine.Targets(ctx, genomes)
    rows = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50)
    ranks = rng.integers(0, 3, size=len(cand)) if with_ranks else None
    want = rows.greedy(len(cand), ranks)
    sid, un, st, en = rows.fetch()
    exp = oracle.lazy_greedy(sid, un, st, en, len(cand), [len(g[0]) for g in genomes],
                             None, ranks)
    assert want == exp and len(want) > 20
    rows.close(); t.close()
    lens = [sum(len(s) for s in g) for g in genomes]
    if not partial:
        for world in (1, 2, 3, 5):
            bounds = parallel.split_universes(lens, world)
            assert bounds[0] == 0 and bounds[-1] == len(genomes) and len(bounds) == world + 1
            got = _sharded_picks(engine, ctx, p, genomes, bounds, len(cand), ranks,
                                 lambda sh: (lambda w: engine.shards_allreduce_local(sh, w)))
            assert got == want, world
        # a rank without genomes (more ranks than genomes can feed) still takes part
        got = _sharded_picks(engine, ctx, p, genomes, [0, 0, 10, 23, 23], len(cand), ranks,
                             lambda sh: (lambda w: engine.shards_allreduce_local(sh, w)))
        assert got == want
        # the one refusal: rows longer than 257 bases (100-base probes, cover extension 80) -- the caller solves the group
        # whole
        t = engine.Targets(ctx, genomes)
        rows = engine.Rows.scan(ctx, p, t, 2, 100, 0, 80)
        with pytest.raises(ValueError, match="solved unsharded"):
            engine.Shard(rows, len(cand), ranks)
        with pytest.raises(ValueError, match="solved unsharded"):
            engine.Shard(rows, len(cand), ranks, [0.9] * len(genomes))
        rows.close(); t.close()
    else:
        # partial coverage (round 4): need[u] and the acceptance thresholds of a universe on
        # the rank that owns it, the candidates' verdicts exchanged with the lost marks -- the unsharded picks, in order;
        # uniform and mixed fractions (a shard whose own universes all want full cover still takes part in the third step)
        for up in ([0.9] * len(genomes), [1.0] * 12 + [0.6] * (len(genomes) - 12), [0.35, 1.0] * (len(genomes) // 2) + [0.8]):
            t = engine.Targets(ctx, genomes)
            rows = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50)
            want_p = rows.greedy(len(cand), ranks, up)
            sid, un, st, en = rows.fetch()
            exp_p = oracle.lazy_greedy(sid, un, st, en, len(cand), [len(g[0]) for g in genomes], up, ranks)
            rows.close(); t.close()
            assert want_p == exp_p and 0 < len(want_p) < len(want)
            for bounds in (parallel.split_universes(lens, 2), parallel.split_universes(lens, 3), [0, 0, 10, 23, 23]):
                got = _sharded_picks(engine, ctx, p, genomes, bounds, len(cand), ranks,
                                     lambda sh: (lambda w: engine.shards_allreduce_local(sh, w)), up)
                assert got == want_p, (up[:3], bounds)
    p.close()


def test_universe_sharded_solver_over_rccl_single_rank(oracle):
    """The same round loop with the exchanges going through RCCL
    (catchhip_shard_allreduce) on a one-rank communicator; the exchange is
    packed (only the sets alive at the last apply travel): its sizes never
    grow, and what travels last is next to nothing."""
    engine, probe = _engine(), _probe_mod()
    c2 = engine.Context(0)
    c2.comm_init(engine.Context.comm_unique_id(), 1, 0)
    genomes = small_species(seed=17, n=9, length=4000)
    cand = candidates(genomes, 100, 50)
    k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
    p = engine.Probes(c2, uniq, owner, ep, eo, k)
    sel = oracle.set_cover_filter([cand], [genomes], 2, 100, coverage=1.0,
                                  cover_extension=50, return_intermediate=True)[1][0]["picks"]
    shapes = []

    def exchange_over_rccl(sh):
        def ex(w):
            shapes.append((w, sh[0]._exchange_shape()[w]))
            for x in sh:
                x.allreduce(w)
        return ex
    got = _sharded_picks(engine, c2, p, genomes, [0, len(genomes)], len(cand), None, exchange_over_rccl)
    assert got == sel
    gains = [n for w, n in shapes if w == 0]
    marks = [n for w, n in shapes if w == 1]
    assert gains[0] == len(cand) + 2 and marks[0] == len(cand) and len(gains) == len(marks)
    assert all(a >= b for a, b in zip(gains, gains[1:])) and all(a >= b for a, b in zip(marks, marks[1:]))
    assert gains[-1] < gains[0] // 4 and all(g == m + 2 for g, m in zip(gains, marks))
    p.close()
    c2.close()


@pytest.mark.parametrize("partial", [0, 1])
def test_round_loop_under_the_c_abi_equals_the_interpreters_loop(ctx, oracle, partial):
    """catchhip_shard_solve (round 6: the whole round loop of a sharded instance in one call, several rounds queued
    per host read-back, exchange buffers at the capacity of the last read-back) == parallel.sharded_solve's loop in
    the interpreter (the step functions: one read-back per round, in apply) == the unsharded picks == the oracle, in
    pick order: 1, 2, 3 and 5 universe ranges exchanging among themselves (transport "local"), 1 / 3 / 16 rounds per
    read-back, with and without ranks, full and partial coverage (uniform and mixed fractions), a shard without
    genomes; and over RCCL on a one-rank communicator (transport "rccl").  partial = 0: full coverage, 1: partial."""
    from catch_amd import parallel
    from catch_amd.utils import synthetic
    engine, probe = _engine(), _probe_mod()
    rng = np.random.Generator(np.random.PCG64(199))
    genomes = synthetic.make_species(rng, [6000], 21, 3, 0.06, 0.012)
    cand = candidates(genomes, 100, 50)
    k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
    p = engine.Probes(ctx, uniq, owner, ep, eo, k)
    lens = [sum(len(s) for s in g) for g in genomes]
    glen = [len(g[0]) for g in genomes]

    def solve(c, probes, bounds, ranks, up, native, rounds_per_sync=4):
        held, shards = [], []
        try:
            for v in range(len(bounds) - 1):
                t = engine.Targets(c, genomes[bounds[v]:bounds[v + 1]])
                held.append(t)
                rows = engine.Rows.scan(c, probes, t, 2, 100, 0, 50)
                held.append(rows)
                part = up is not None and any(q < 1.0 for q in up)
                shards.append(engine.Shard(rows, len(cand), ranks, up[bounds[v]:bounds[v + 1]] if part else None,
                                           instance_partial=part))
            if native is None:
                return parallel.sharded_solve(shards, lambda w: engine.shards_allreduce_local(shards, w))
            return engine.shards_solve(shards, native, rounds_per_sync)
        finally:
            for h in shards + held[::-1]:
                h.close()

    for with_ranks in (False, True):
        ranks = rng.integers(0, 3, size=len(cand)) if with_ranks else None
        for up in ([[0.9] * len(genomes), [0.35, 1.0] * (len(genomes) // 2) + [0.8]] if partial else [None]):
            t = engine.Targets(ctx, genomes)
            rows = engine.Rows.scan(ctx, p, t, 2, 100, 0, 50)
            want = rows.greedy(len(cand), ranks, up)
            sid, un, st, en = rows.fetch()
            assert want == oracle.lazy_greedy(sid, un, st, en, len(cand), glen, up, ranks) and len(want) > 10
            rows.close(); t.close()
            for bounds in ([0, len(genomes)], parallel.split_universes(lens, 2), parallel.split_universes(lens, 3),
                           parallel.split_universes(lens, 5), [0, 0, 9, 21, 21]):
                assert solve(ctx, p, bounds, ranks, up, None) == want
                for rps in (1, 3, 16):
                    assert solve(ctx, p, bounds, ranks, up, "local", rps) == want, (with_ranks, up and up[:2], bounds, rps)
    p.close()
    # transport "rccl": a one-rank communicator on a context of its own
    c2 = engine.Context(0)
    c2.comm_init(engine.Context.comm_unique_id(), 1, 0)
    p2 = engine.Probes(c2, uniq, owner, ep, eo, k)
    t = engine.Targets(c2, genomes)
    rows = engine.Rows.scan(c2, p2, t, 2, 100, 0, 50)
    sid, un, st, en = rows.fetch()
    want = oracle.lazy_greedy(sid, un, st, en, len(cand), glen, None, None)
    rows.close(); t.close()
    if not partial:
        for rps in (1, 4):
            assert solve(c2, p2, [0, len(genomes)], None, None, "rccl", rps) == want
    else:
        up = [0.9] * len(genomes)
        assert solve(c2, p2, [0, len(genomes)], None, up, "rccl", 4) == oracle.lazy_greedy(sid, un, st, en, len(cand), glen, up, None)
    p2.close()
    c2.close()


def _torchrun(nranks, script_args, env, ok):
    """torch.distributed.run on a port that was free a moment ago (found by binding and closing a socket, so somebody
    else can take it before the launcher's store does).  One run of the suite in ~15 on the GPU box lost this launch
    within seconds (output not captured; 42 launches in a loop afterwards all passed), so a run that ends within a
    minute without the expected output is launched again on another port, twice at most -- a failure of the product
    fails three times."""
    import socket
    import subprocess
    import time
    r = None
    for attempt in range(3):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                            "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
                            "--master-port", str(port)] + list(script_args),
                           env=env, capture_output=True, text=True, timeout=600)
        if ok(r.stdout) or time.time() - t0 > 60:
            break
    return r


@pytest.mark.parametrize("nranks", [2, 3])
def test_plugin_over_several_ranks_selects_what_one_rank_selects(nranks):
    """torch.distributed.run with 2 and 3 ranks (all on this box's one GPU, so
    the exchanges go through gloo instead of RCCL): SetCoverFilter with one
    group sharded by universes and the others spread whole, pigeonhole and
    random anchors -- every rank returns the oracle's selection."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CATCHHIP_EXCHANGE="gloo", CATCHHIP_SHARD_MIN_BASES="1",
               MASTER_ADDR="127.0.0.1")
    r = _torchrun(nranks, [os.path.join(here, "multirank_plugin_check.py")], env, lambda out: "MULTIRANK_PLUGIN_OK" in out)
    assert "MULTIRANK_PLUGIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_bench_preflight_over_two_ranks():
    """`bench.py --gpus 2 --preflight` (both ranks on this box's one GPU, so RCCL
    refuses and the ranks agree on the gloo exchange): one step of the S2
    workload per rank, every rank's line of diagnostics present -- its groups,
    pack / scan / solve times, the exchange in use and which RCCL copy the
    library is pinned to (the file opened by path, whatever torch mapped)."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", CATCHHIP_SHARD_MIN_BASES="1")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = _torchrun(2, [os.path.join(repo, "bench.py"), "--gpus", "2", "--workload", "S2", "--preflight"], env,
                  lambda out: any(ln.startswith("{") for ln in out.splitlines()))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and "cpu_baseline" not in d
    pf = d["preflight"]
    assert [p["rank"] for p in pf] == [0, 1]
    assert all("librccl" in p["rccl"] and "/opt/rocm" in p["rccl"] for p in pf)
    assert all(p["step_s"] > 0 and p["pack_h2d_s"] > 0 for p in pf)
    assert sorted(g for p in pf for g in p["groups"]) + sorted(pf[0]["sharded_groups"]) != []
    assert d["rccl"] and "version" in d["rccl"]


# ---------------------------------------------------------------- other configs
@pytest.mark.parametrize("name,scale", [("S3", 0.02), ("S4", 0.01)])
def test_scaled_baseline_configs_match_oracle(ctx, oracle, name, scale):
    """BASELINE configs 3 and 4 at reduced scale: 800 single-segment genomes
    in one group (S3) and 20 groups of very different sizes (S4); selected
    probe sets identical to the oracle's."""
    from catch_amd import genome, probe
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.utils import synthetic
    groups = synthetic.dataset(name, scale=scale)
    cands = [candidates(g, 100, 50) for g in groups]
    exp = oracle.set_cover_filter(cands, groups, 2, 100, coverage=1.0,
                                  cover_extension=50)
    f = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    probes = [[probe.Probe.from_str(s) for s in c] for c in cands]
    gen = [[genome.Genome.from_one_seq(g[0]) for g in grp] for grp in groups]
    out = f.filter(probes, gen, input_is_grouped=True)
    got = [sorted(p.seq_str for p in g) for g in out]
    assert got == [sorted(cands[i][j] for j in ids) for i, ids in enumerate(exp)]


def test_config3_pipeline_ndf_then_scf_matches_oracle(ctx, oracle):
    """config 3 shape: --filter-with-lsh-hamming 2 before the set cover."""
    from catch_amd import genome, probe
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithHammingDistance
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.utils import synthetic
    groups = synthetic.dataset("S3", scale=0.01)
    strs = candidates(groups[0], 100, 50, dedup=False)
    random.seed(7)
    pos = oracle.lsh_draw_positions(oracle.lsh_num_tables(2, 100, 20), 20, 100)
    kept = oracle.ndf_hamming(strs, 2, pos)
    exp = oracle.set_cover_filter([kept], groups, 2, 100, coverage=1.0, cover_extension=50)
    random.seed(7)
    ndf = NearDuplicateFilterWithHammingDistance(2, 100)
    out1 = ndf.filter([probe.Probe.from_str(s) for s in strs])
    assert [p.seq_str for p in out1] == kept
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    gen = [[genome.Genome.from_one_seq(g[0]) for g in groups[0]]]
    out2 = scf.filter([out1], gen, input_is_grouped=True)
    assert sorted(p.seq_str for p in out2[0]) == sorted(kept[i] for i in exp[0])


# ---------------------------------------------------------------- full sizes
def _full_size(key):
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "full_size_picks.json")) as f:
        return json.load(f)[key]


def _digest(ids):
    import hashlib
    a = np.sort(np.asarray(ids, dtype=np.int64))
    return hashlib.sha256(a.astype("<i8").tobytes()).hexdigest()


def _digest_in_order(ids):
    import hashlib
    return hashlib.sha256(np.asarray(ids, dtype="<i8").tobytes()).hexdigest()


@pytest.mark.parametrize("name", ["S4", "S4i"])
def test_full_size_config4_matches_oracle_digests(ctx, name):
    """BASELINE configs[3] at FULL size (S4: 20,755 genomes in 20 groups, 592
    Mbp, 8.9 M candidates, 519 M cover rows; S4i: the same generator with
    insertions and deletions between clades and strains, 20,169 genomes, 501
    Mbp, 9.3 M candidates, 465 M rows): per group the number of
    candidates, the number of picks and the sha256 of the sorted pick ids equal
    what the pinned CPU oracle computed in the authoring container
    (tests/golden/make_full_size.py; the oracle needs ~20 minutes there) -- and
    so does the sha256 of the ids in PICK ORDER; the same for `-c 0.9` (partial
    coverage) on the same rows, in fewer than an eighth as many rounds as picks."""
    from catch_amd import probe
    from catch_amd.utils import synthetic
    engine = _engine()
    gold = {g["group"]: g for g in _full_size(name)["groups"]}
    groups = synthetic.dataset(name)
    assert len(groups) == len(gold) == 20
    for gi, genomes in enumerate(groups):
        t = engine.Targets(ctx, genomes)
        c = engine.Candidates(ctx, t, 100, 50)
        k, ep, eo = probe.anchor_entries_equal_length(c.n, 100, 2, 100)
        p = c.probes(k, ep, eo)
        ids, nrows = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n)
        # the same group under -c 0.9 (partial coverage: frontier rounds with the universe test)
        ids09, nrows09 = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n,
                                                universe_p=[0.9] * len(genomes))
        rounds09 = ctx.counters()["greedy_iters"]
        p.close(); c.close(); t.close()
        g = gold[gi]
        assert (c.n, nrows, len(ids)) == (g["n_candidates"], g["n_rows"], g["n_picks"]), gi
        assert _digest(ids) == g["picks_sha256"], gi
        assert _digest_in_order(ids) == g["picks_in_order_sha256"], gi      # the sequential pick ORDER
        assert (nrows09, len(ids09)) == (g["n_rows"], g["n_picks_c09"]), gi
        assert _digest(ids09) == g["picks_c09_sha256"], gi
        assert _digest_in_order(ids09) == g["picks_c09_in_order_sha256"], gi
        assert rounds09 < len(ids09) // 8, (gi, rounds09, len(ids09))


def test_full_size_config3_matches_oracle_digests(ctx):
    """BASELINE configs[2] at FULL size (S3: 40,000 influenza-like segment
    records, 68 Mbp, --filter-with-lsh-hamming 2 then the set cover): the
    near-duplicate filter keeps exactly the oracle's candidates (sha256 of the
    kept strings in inclusion order) and the set cover picks the oracle's ids."""
    import hashlib
    from catch_amd import probe
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithHammingDistance
    from catch_amd.utils import synthetic
    engine = _engine()
    g = _full_size("S3")["groups"][0]
    genomes = synthetic.dataset("S3")[0]
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, 100, 50)
    assert c.ncandidates == g["n_windows"]
    random.seed(7)
    ndf = NearDuplicateFilterWithHammingDistance(2, 100)
    ndf._apply_to_candidates(c)
    assert c.n == g["n_candidates"]
    # the kept candidates, in the filter's inclusion order, as strings
    pos = c.positions()
    seqs = [s for gg in genomes for s in gg]
    which = np.searchsorted(t.seq_off, pos, side="right") - 1
    local = pos - t.seq_off[which]
    kept = [seqs[q][o:o + 100] for q, o in zip(which.tolist(), local.tolist())]
    assert hashlib.sha256("\n".join(kept).encode()).hexdigest() == g["kept_sha256"]
    k, ep, eo = probe.anchor_entries_equal_length(c.n, 100, 2, 100)
    p = c.probes(k, ep, eo)
    ids, nrows = engine.setcover_filter(ctx, p, t, 2, 100, 0, 50, c.n)
    p.close(); c.close(); t.close()
    assert (nrows, len(ids)) == (g["n_rows"], g["n_picks"])
    assert _digest(ids) == g["picks_sha256"]
    assert _digest_in_order(ids) == g["picks_in_order_sha256"]


def _config5_scales():
    """The scales of S5 that tests/golden/full_size_picks.json pins (x 0.1 = 390 Mbp joins when its oracle run --
    make_full_size.py S5:0.1, hours of CPU -- has been committed)."""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_size_picks.json")) as f:
        keys = json.load(f).keys()
    return sorted(float(k.split(":")[1]) for k in keys if k.startswith("S5:"))


@pytest.mark.parametrize("scale", _config5_scales())
def test_full_size_config5_design_large_matches_oracle_digest(ctx, tmp_path, capsys, scale):
    """BASELINE configs[4] at real scales (S5 x 0.01: 2,132 genomes, 48 Mbp,
    2,598 fragments -> 1,130 clusters, 826 k candidates after the MinHash
    near-duplicate filter; round 5: x 0.02 = 3,939 genomes, 84 Mbp -> 1,392
    clusters, 348 k probes; x 0.05 = 10,172 genomes, 195 Mbp, 11,757 fragments ->
    1,663 clusters, 1.69 M candidates after the filter, 415,548 probes):
    `design_large` defaults end to end (-m 5 random anchors, -e 50, cluster 0.15
    from 50-kb fragments, MinHash filter 0.6, set cover per cluster) writes
    exactly the probes the oracle's chain of the same steps selects
    (tests/golden/make_full_size.py S5:<scale>: 12, 31 and 87 minutes of CPU; round 6:
    x 0.1 = 20,066 genomes, 386 Mbp, 22,921 fragments -> 1,903 clusters, 2.29 M
    candidates after the filter, 504,324 probes: 193 minutes)."""
    import hashlib
    from catch_amd import design
    from catch_amd.utils import synthetic, seq_io
    g = _full_size("S5:%g" % scale)["design"]
    genomes = synthetic.dataset("S5", scale=scale)[0]
    assert len(genomes) == g["genomes"]
    fn = tmp_path / "s5.fasta"
    with open(fn, "w") as f:
        for i, gen in enumerate(genomes):
            for j, s in enumerate(gen):
                f.write(">g%d_%d\n%s\n" % (i, j, s))
    out = tmp_path / "probes.fasta"
    args = design.parse_args([str(fn), "-o", str(out),
                              "--cluster-and-design-separately-method", "simple"],
                             args_type="large")
    assert (args.mismatches, args.cover_extension, args.filter_with_lsh_minhash,
            args.cluster_and_design_separately, args.cluster_from_fragments) == (5, 50, 0.6, 0.15, 50000)
    random.seed(21)
    np.random.seed(22)
    pb = design.main(args)
    capsys.readouterr()
    # (the records one by one, not read_fasta's dict: a probe is named by the last 10 hex digits of its SHA-224 as in
    # catch/probe.py:301-321, and among the 504,324 probes of x 0.1 two share a name -- a dict keyed by name loses one)
    got = sorted(set(seq_io.iterate_fasta(str(out), replace_degenerate=False)))
    assert len(got) == g["n_probes"] == len(set(p.seq_str for p in pb.final_probes))
    assert hashlib.sha256("\n".join(got).encode()).hexdigest() == g["probes_sha256"]


def _np_cover_check(set_id, univ, start, end, genome_len, picks, p=None):
    """numpy restatement of catchhip_rows_cover_check (small instances)."""
    off = np.concatenate([[0], np.cumsum(genome_len)])
    U = np.zeros(int(off[-1]), dtype=bool)
    for u, s0, e0 in zip(univ, start, end):
        U[off[u] + s0: off[u] + e0] = True
    C = np.zeros_like(U)
    nogain = 0
    for s in picks:
        fresh = 0
        for r in np.nonzero(set_id == s)[0]:
            seg = slice(int(off[univ[r]] + start[r]), int(off[univ[r]] + end[r]))
            fresh += int((~C[seg]).sum())
            C[seg] = True
        nogain += fresh == 0
    short = 0
    for u in range(len(genome_len)):
        n = int(U[off[u]:off[u + 1]].sum())
        pu = 1.0 if p is None else p[u]
        need = n - int(n - pu * n)
        short += int((C & U)[off[u]:off[u + 1]].sum()) < need
    return nogain, short, int(U.sum()), int((C & U).sum())


def test_cover_check_kernels_equal_a_numpy_replay(ctx):
    """catchhip_rows_cover_check (csrc/check.hip: the picks replayed per universe in pick order over a covered-
    positions bitmap; shares no code with the solvers) against a numpy replay: solved instances pass with every
    counter at zero; a dropped pick leaves universes short; a pick moved behind the sets that cover all of it is
    reported as a pick without gain; repeated / out-of-range ids are counted."""
    engine = _engine()
    rng = np.random.Generator(np.random.PCG64(77))
    for trial in range(8):
        U = int(rng.integers(3, 30))
        glen = rng.integers(300, 3000, size=U)
        P = int(rng.integers(40, 400))
        rows = []
        for s in range(P):
            for u in rng.choice(U, size=int(rng.integers(1, min(U, 6) + 1)), replace=False):
                a = int(rng.integers(0, glen[u] - 60))
                rows.append((s, int(u), a, a + int(rng.integers(20, 257))))
        rows = sorted(set((s, u, a, min(e, int(glen[u]))) for s, u, a, e in rows))
        # one row per (set, universe) start: merge nothing, the table only has to be sorted
        sid = np.array([r[0] for r in rows], np.int32); un = np.array([r[1] for r in rows], np.int32)
        st = np.array([r[2] for r in rows], np.int64); en = np.array([r[3] for r in rows], np.int64)
        R = engine.Rows.from_host(ctx, sid, un, st, en, glen)
        p = None if trial % 2 == 0 else rng.choice([1.0, 0.9, 0.5], size=U)
        ids = R.greedy(P, universe_p=p)
        got = R.cover_check(P, ids, p)
        want = _np_cover_check(sid, un, st, en, glen, ids, p)
        assert (got["picks_without_gain"], got["universes_short"], got["universe_bases"], got["covered_bases"]) == want
        assert got["picks_without_gain"] == 0 and got["universes_short"] == 0 and got["bad_pick_ids"] == 0
        if len(ids) > 1:
            # the first pick covers something nobody else needs to: without it a universe stays short (p = 1)
            bad = R.cover_check(P, ids[1:], p)
            want = _np_cover_check(sid, un, st, en, glen, ids[1:], p)
            assert (bad["picks_without_gain"], bad["universes_short"]) == want[:2]
            if p is None:
                assert bad["universes_short"] >= 1
            # a set replayed twice in spirit: the last pick first and again last -> counted as repeated
            rep = R.cover_check(P, list(ids) + [ids[0]], p)
            assert rep["bad_pick_ids"] == 1
            # under full coverage everything is covered in the end: one more set has nothing left to gain
            rest = sorted(set(sid.tolist()) - set(ids))
            if p is None and rest:
                m = R.cover_check(P, list(ids) + [rest[0]], None)
                assert (m["picks_without_gain"], m["universes_short"], m["bad_pick_ids"]) == (1, 0, 0)
        assert R.cover_check(P, [P + 3], p)["bad_pick_ids"] == 1
        R.close()


def test_property_checks_at_scale_config5(ctx):
    """BASELINE configs[4] through the design_large chain at S5 x 0.25 (47,514 genomes, 0.9 Gbases, 20 M candidate
    windows, 640 k probes): no oracle can solve this, so every set-cover instance the plugin solves is checked by
    the independent replay kernels (engine.collect_solution_checks -> catchhip_rows_cover_check on a second scan):
    every pick covered something new at its turn, every universe is covered to its requirement."""
    from catch_amd import engine as eng, genome
    from catch_amd.filter import near_duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.utils import synthetic
    genomes = synthetic.dataset("S5", scale=0.25)[0]
    gobjs = [[genome.Genome.from_one_seq(g[0]) for g in genomes]]
    random.seed(21)
    np.random.seed(22)
    ndf = near_duplicate_filter.NearDuplicateFilterWithMinHash(0.6)
    scf = set_cover_filter.SetCoverFilter(mismatches=5, lcf_thres=100, coverage=1.0, cover_extension=50,
                                          kmer_probe_map_k=20)
    pd = probe_designer.ProbeDesigner(gobjs, [ndf, scf], probe_length=100, probe_stride=50, cluster_threshold=0.15,
                                      cluster_merge_after=scf, cluster_method="choose", cluster_fragment_length=50000)
    clusters = pd._cluster_genomes()
    mode = pd._device_front_end_mode(clusters, ndf, scf)
    run = scf._filter_genomes_device if mode == "per group" else scf._filter_genomes_device_union
    checks = []
    eng.collect_solution_checks(checks)
    try:
        chosen = run(clusters, 100, 50, None, ndf)
    finally:
        eng.collect_solution_checks(None)
    assert sum(len(c) for c in chosen) > 500000
    assert len(checks) >= 1 and sum(c["picks"] for c in checks) > 500000
    assert all(c["picks_without_gain"] == 0 and c["universes_short"] == 0 and c["bad_pick_ids"] == 0 for c in checks)
    assert all(c["covered_bases"] == c["universe_bases"] for c in checks)      # -c 1.0


def test_clustered_design_over_fragment_views_equals_sliced_fragments(ctx, monkeypatch):
    """Round 6: the clusters of a clustered design as VIEWS of the genomes' own storage (engine.FragmentTable,
    probe_designer.ClusteredFragments: no str and no Genome per fragment) == the same design with every fragment sliced
    out and wrapped (CATCHHIP_CLUSTER_SLICE_FRAGMENTS, the path of rounds 1-5): same clusters, same fragments, same
    selected probes in the same order, through the union front end and through a generic consumer that iterates the
    clusters as lists of Genomes; short last fragments, sequences below the skip length and one-fragment genomes in."""
    import random
    from catch_amd import genome
    from catch_amd.filter import near_duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.utils import synthetic
    monkeypatch.setenv("CATCHHIP_TEST_HOOKS", "1")
    genomes = synthetic.dataset("S5", scale=0.01)[0]
    rng = np.random.RandomState(11)
    extra = ["".join(rng.choice(list("ACGT"), size=n)) for n in (150, 700, 50001, 99999, 120)]
    gobjs = [[genome.Genome.from_one_seq(g[0]) for g in genomes] + [genome.Genome.from_one_seq(s) for s in extra]]

    def design(slice_fragments, frag_len, skip):
        if slice_fragments:
            monkeypatch.setenv("CATCHHIP_CLUSTER_SLICE_FRAGMENTS", "1")
        else:
            monkeypatch.delenv("CATCHHIP_CLUSTER_SLICE_FRAGMENTS", raising=False)
        random.seed(21)
        np.random.seed(22)
        ndf = near_duplicate_filter.NearDuplicateFilterWithMinHash(0.6)
        scf = set_cover_filter.SetCoverFilter(mismatches=5, lcf_thres=100, coverage=1.0, cover_extension=50,
                                              kmer_probe_map_k=20)
        pd = probe_designer.ProbeDesigner(gobjs, [ndf, scf], probe_length=100, probe_stride=50, cluster_threshold=0.15,
                                          cluster_merge_after=scf, cluster_method="simple",
                                          cluster_fragment_length=frag_len, seq_length_to_skip=skip)
        clusters = pd._cluster_genomes()
        assert isinstance(clusters, probe_designer.ClusteredFragments) == (not slice_fragments)
        mode = pd._device_front_end_mode(clusters, ndf, scf)
        assert mode == "union"
        chosen = scf._filter_genomes_device_union(clusters, 100, 50, skip, ndf)
        return [[g.seqs[0] for g in cl] for cl in clusters], chosen

    for frag_len, skip in ((50000, None), (20000, 130)):
        want_clusters, want = design(True, frag_len, skip)
        got_clusters, got = design(False, frag_len, skip)
        assert got_clusters == want_clusters
        assert got == want and sum(len(c) for c in got) > 1000


def test_ndf_then_scf_chains_equal_the_live_reference(ctx):
    """Near-duplicate filter -> set cover filter, recorded from the LIVE
    reference under PYTHONHASHSEED=0 (tests/golden/ndf_scf_chains.json): the
    reference's filter returns `list(to_include)`, a set of probes, and the set
    cover numbers its candidates in that order.  Both front ends -- strings on
    the host, candidates on the device -- must hand the set cover filter the
    kept probes in exactly that order (emulated: catchhip_pyset_order) and
    select the reference's probes."""
    import hashlib
    import json
    from catch_amd import genome
    from catch_amd.filter import candidate_probes
    from catch_amd.filter.near_duplicate_filter import (NearDuplicateFilterWithHammingDistance,
                                                        NearDuplicateFilterWithMinHash)
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.utils import synthetic
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndf_scf_chains.json")) as f:
        runs = json.load(f)["runs"]

    def sha(strs):
        return hashlib.sha256("\n".join(strs).encode()).hexdigest()
    assert len(runs) >= 4
    for r in runs:
        genomes = synthetic.dataset(r["dataset"], scale=r["scale"])[r["group"]]
        gobjs = [genome.Genome(list(g), chrs=dict(("c%d" % i, s) for i, s in enumerate(g))) if len(g) > 1
                 else genome.Genome.from_one_seq(g[0]) for g in genomes]

        def make():
            random.seed(r["seed"])
            np.random.seed(r["seed"] + 1)
            ndf = (NearDuplicateFilterWithHammingDistance(r["threshold"], 100) if r["filter"] == "hamming"
                   else NearDuplicateFilterWithMinHash(r["threshold"]))
            return ndf, SetCoverFilter(mismatches=r["mismatches"], lcf_thres=100, coverage=1.0, cover_extension=50)
        # strings on the host
        ndf, scf = make()
        cands = candidate_probes.candidate_strings_from_sequences([s for g in genomes for s in g], 100, 50)
        kept = ndf._filter_strs(cands)
        assert len(kept) == r["kept"] and sha(kept) == r["kept_in_order_sha256"], r
        ids = scf._filter_strs([kept], [gobjs], assume_unique=True)[0]
        picks = sorted(kept[i] for i in ids)
        assert len(picks) == r["picks"] and sha(picks) == r["picks_sorted_sha256"], r
        # candidates on the device
        ndf, scf = make()
        out = scf._filter_genomes_device([gobjs], 100, 50, None, ndf)[0]
        assert sha(sorted(out)) == r["picks_sorted_sha256"], r


@pytest.mark.parametrize("n", [1, 4, 5, 6, 19, 20, 77, 1000, 49999, 50001, 78643, 78644, 157286, 400000])
def test_set_iteration_order_on_the_device(ctx, n):
    """catchhip_pyset_order_device (all insertions of a table generation at once,
    atomicMin on (rank, index) words) == the sequential emulation, at sizes on
    both sides of every rebuild rule (8 slots rebuilt at 5 keys; x4 up to
    50,000 keys, x2 beyond; a rebuild triggered by the very last key) -- and,
    where the interpreter can, == list(set) of ints with those hashes."""
    from catch_amd import engine
    rng = np.random.RandomState(n)
    for kind in ("random", "clustered"):
        if kind == "random":
            h = rng.randint(-2**62, 2**62, size=n, dtype=np.int64)
        else:       # long collision chains: few distinct low bits, displaced keys displacing others
            h = (rng.randint(0, 64, size=n).astype(np.int64) + (np.arange(n, dtype=np.int64) << 24))
        want = engine.pyset_order(h)
        got = ctx.pyset_order(h)
        assert np.array_equal(got, want), (n, kind)
    if n <= 50001:
        keys = [int(x) for x in rng.permutation(4 * n)[:n] + 1]     # hash(i) == i for small positive ints
        s = set()
        for k in keys:
            s.add(k)
        order = ctx.pyset_order(np.asarray(keys, dtype=np.int64))
        assert [keys[i] for i in order] == list(s)


def test_selection_equals_live_reference_runs(ctx):
    """The inputs the LIVE reference was run on in the authoring container
    (tools/time_reference.py: S1, S2 in full, S3 and S4 scaled down to what the
    Python reference finishes in minutes): the GPU filter selects exactly the
    probes catch.filter.set_cover_filter.SetCoverFilter selected there
    (sha256 of the sorted selected strings, tests/golden/reference_runs.json)."""
    import hashlib
    import json
    from catch_amd import genome
    from catch_amd.filter import candidate_probes
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.utils import synthetic
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "reference_runs.json")) as f:
        runs = json.load(f)["runs"]
    assert len(runs) >= 6
    for r in runs:
        groups = synthetic.dataset(r["input"], scale=r["scale"])
        cands = [list(dict.fromkeys(candidate_probes.candidate_strings_from_sequences(
            [s for g in grp for s in g], 100, 50))) for grp in groups]
        assert sum(map(len, cands)) == r["P"]
        gen = [[genome.Genome(list(g), chrs=dict(("c%d" % i, s) for i, s in enumerate(g))) if len(g) > 1 else genome.Genome.from_one_seq(g[0])
                for g in grp] for grp in groups]
        f = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
        ids = f._filter_strs(cands, gen, assume_unique=True)
        sel = [sorted(c[i] for i in g) for c, g in zip(cands, ids)]
        dig = hashlib.sha256("\n".join(",".join(g) for g in sel).encode()).hexdigest()
        assert sum(map(len, sel)) == r["probes_out"], (r["input"], r["scale"])
        assert dig == r["picks_sha256"], (r["input"], r["scale"])


def test_selection_equals_live_reference_on_real_ebola_genomes(ctx):
    """Real sequences: the first 30 / 100 records of the Ebola FASTA of the reference's own tests
    (tests/golden/ebola_zaire_100.fasta.gz: real composition, low-complexity runs, indels, N runs).
    The GPU filter selects exactly what the LIVE reference selected (tests/golden/real_runs.json,
    made by tests/golden/make_real_golden.py): pigeonhole anchors at -pl 100 and -pl 75, random
    anchors + truncated alignments (-l 60, np.random seeded as there), partial coverage."""
    import hashlib
    import json
    from catch_amd import genome
    from catch_amd.filter import candidate_probes
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.utils import seq_io
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "real_runs.json")) as f:
        d = json.load(f)
    genomes_all = seq_io.read_genomes_from_fasta(os.path.join(here, d["fasta"]))
    assert len(d["runs"]) >= 4
    for r in d["runs"]:
        gen = genomes_all[:r["records"]]
        pl = r["probe_length"]
        cands = list(dict.fromkeys(candidate_probes.candidate_strings_from_sequences(
            [s for g in gen for s in g.seqs], pl, pl // 2)))
        assert len(cands) == r["P"]
        if r["np_random_seed"] is not None:
            np.random.seed(r["np_random_seed"])
        f = SetCoverFilter(mismatches=r["mismatches"], lcf_thres=r["lcf_thres"], coverage=r["coverage"],
                           cover_extension=r["cover_extension"])
        ids = f._filter_strs([cands], [gen], assume_unique=True)[0]
        sel = sorted(cands[i] for i in ids)
        assert len(sel) == r["probes_out"], r
        assert hashlib.sha256(",".join(sel).encode()).hexdigest() == r["picks_sha256"], r


# ---------------------------------------------------------------- front end
def test_design_cli_end_to_end(ctx, oracle, tmp_path, capsys):
    """python -m catch_amd.design on two FASTA datasets: the written probe set
    equals candidates -> dedup -> oracle set cover on the same files."""
    from catch_amd import design
    from catch_amd.utils import synthetic, seq_io
    rng = np.random.Generator(np.random.PCG64(44))
    groups = [synthetic.make_species(rng, [2500], 5, 2, 0.05, 0.01),
              synthetic.make_species(rng, [1800], 4, 2, 0.04, 0.02)]
    files = []
    for i, grp in enumerate(groups):
        fn = tmp_path / ("d%d.fasta" % i)
        fn.write_text("".join(">g%d\n%s\n" % (j, g[0].lower() if j == 0 else g[0])
                              for j, g in enumerate(grp)))
        files.append(str(fn))
    out = tmp_path / "probes.fasta"
    pb = design.main(design.parse_args(files + ["-pl", "75", "-ps", "25", "-m", "2",
                                                "-e", "30", "-o", str(out)]))
    printed = int(capsys.readouterr().out.strip().splitlines()[-1])
    cands = [candidates(g, 75, 25) for g in groups]
    exp = oracle.set_cover_filter(cands, groups, 2, 75, coverage=1.0, cover_extension=30)
    want = set(cands[i][j] for i, ids in enumerate(exp) for j in ids)
    got = set(seq_io.read_fasta(str(out)).values())
    assert got == want and printed == len(want) == len(pb.final_probes)


def test_fused_filter_many_groups_matches_separate_calls(ctx, oracle):
    """catchhip_setcover_filter / _many (scan + solve in one call, independent
    groups on their own streams) give the picks of the two-call path and of the
    oracle, with and without ranks / partial coverage."""
    engine, probe = _engine(), _probe_mod()
    ctxs = [ctx, engine.Context(ctx.device), engine.Context(ctx.device)]
    specs, want = [], []
    keep = []
    for gi, c in enumerate(ctxs):
        genomes = small_species(seed=40 + gi, n=4 + gi, length=2500 + 500 * gi)
        cand = candidates(genomes, 100, 50)
        k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
        t = engine.Targets(c, genomes)
        p = engine.Probes(c, uniq, owner, ep, eo, k)
        ranks = None if gi != 1 else [i % 3 for i in range(len(cand))]
        up = None if gi != 2 else [0.9] * len(genomes)
        specs.append((c, p, t, len(cand), ranks, up))
        rows = engine.Rows.scan(c, p, t, 2, 100, 0, 30)
        want.append((rows.greedy(len(cand), ranks, up), rows.n))
        rows.close()
        keep.append((p, t))
    got = engine.setcover_filter_many(specs, 2, 100, 0, 30)
    assert got == want
    for _ in range(3):   # repeated use of the per-context caches
        assert engine.setcover_filter_many(specs, 2, 100, 0, 30) == want
    one = engine.setcover_filter(ctxs[1], specs[1][1], specs[1][2], 2, 100, 0, 30,
                                 specs[1][3], specs[1][4], specs[1][5])
    assert one == want[1]
    with pytest.raises(ValueError):
        engine.setcover_filter_many([specs[0], specs[0]], 2, 100, 0, 30)
    for p, t in keep:
        p.close(); t.close()
    for c in ctxs[1:]:
        c.close()


def test_seed_work_list_overflow_retries(ctx, oracle, monkeypatch):
    """A seed work list that is too small is detected on the device and the
    scan re-runs with the exact size (same rows).  The work list is the
    seed-list scan's (CATCHHIP_SEED_LIST: the key-grouped join, which these
    pigeonhole probes take otherwise, has none and never reads the capacity);
    capacity_events() says that the re-run happened
    (tests/test_capacity_paths.py has the other capacities)."""
    engine = _engine()
    genomes = small_species(seed=8)
    probes = candidates(genomes, 100, 50)
    exp = _oracle_rows(oracle, probes, genomes, 2, 100, 0, 50)
    monkeypatch.setenv("CATCHHIP_SEED_LIST", "1")
    assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 50, engine.SCAN_SEED) == exp
    assert ctx.capacity_events()["seed_list_rerun"] == 0
    monkeypatch.setenv("CATCHHIP_SEED_CAP", "100")
    assert _scan_rows(ctx, probes, genomes, 2, 100, 0, 50, engine.SCAN_SEED) == exp
    assert ctx.counters()["seed_hits"] > 100
    assert ctx.counters()["join_hit_positions"] == 0
    assert ctx.capacity_events()["seed_list_rerun"] == 1


def test_fused_filter_falls_back_when_rows_are_long(ctx, oracle):
    """cover_extension = 100 makes rows 300 bases long: the sync-free fused
    path notices on the device that they exceed the 5-word rows of its round
    kernels and the group is redone through the synchronous calls, which pick
    the lane-per-word kernels."""
    engine, probe = _engine(), _probe_mod()
    genomes = small_species(seed=61, n=5)
    cand = candidates(genomes, 100, 50)
    k, uniq, owner, ep, eo = probe.anchor_table(cand, 2, 100)
    t = engine.Targets(ctx, genomes)
    p = engine.Probes(ctx, uniq, owner, ep, eo, k)
    rows = engine.Rows.scan(ctx, p, t, 2, 100, 0, 100)
    want = (rows.greedy(len(cand)), rows.n)
    _, _, st, en = rows.fetch()
    assert int((en - st).max()) > 257
    rows.close()
    assert engine.setcover_filter(ctx, p, t, 2, 100, 0, 100, len(cand)) == want
    sel = oracle.set_cover_filter([cand], [genomes], 2, 100, coverage=1.0,
                                  cover_extension=100)
    assert sorted(want[0]) == sorted(sel[0])
    p.close(); t.close()


def test_ndf_minhash_golden(ctx):
    """MinHash near-duplicate filter against vectors recorded from the
    reference (run under PYTHONHASHSEED=0): its own unit tests' cases and
    seeded synthetic candidates."""
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    g = load_golden("ndf_minhash")
    recs = g["from_reference_tests"] + g["synthetic"]
    assert len(recs) >= 6
    for c in recs:
        f = ndf.NearDuplicateFilterWithMinHash(c["dist_thres"], c["kmer_size"])
        f.k = c["k"]
        f.reporting_prob = c["reporting_prob"]
        assert f.num_tables() == len(c["params"])
        f._draw_params = lambda c=c: c["params"]
        inp = [probe.Probe.from_str(s) for s in c["probes"]]
        out = f.filter(inp)
        assert sorted(p.seq_str for p in out) == c["out"]
        if "seed" in c:   # (a, b) drawn from `random` like the reference
            random.seed(c["seed"])
            f2 = ndf.NearDuplicateFilterWithMinHash(c["dist_thres"], c["kmer_size"])
            assert [[list(ab) for ab in t] for t in f2._draw_params()] == c["params"]


def test_ndf_minhash_matches_oracle_large(ctx, oracle):
    """More probes, unequal lengths, duplicates (multiplicity order), N runs."""
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    genomes = small_species(seed=91, n=10, length=6000, d1=0.05, d2=0.02)
    strs = candidates(genomes, 100, 25, dedup=False)
    strs += [s[:80] for s in strs[:200]] + strs[:300]
    for d, ks, seed in ((0.6, 10, 5), (0.35, 12, 6)):
        random.seed(seed)
        f = ndf.NearDuplicateFilterWithMinHash(d, ks)
        params = f._draw_params()
        f._draw_params = lambda params=params: params
        got = sorted(p.seq_str for p in f.filter([probe.Probe.from_str(s) for s in strs]))
        want = sorted(oracle.ndf_minhash(strs, d, params, ks))
        assert got == want
        assert len(got) < len(set(strs))


def test_coverage_analyzer_golden(ctx, oracle, tmp_path):
    """catch_amd.coverage_analysis.Analyzer against the results recorded from
    the reference's Analyzer (its own tests + seeded synthetic runs): cover
    ranges per genome and strand, bases covered, average depth, sequences
    mapped per probe, and the table strings."""
    from catch_amd import coverage_analysis as ca
    from catch_amd import genome, probe
    g = load_golden("coverage_analysis")
    recs = g["from_reference_tests"] + g["synthetic"]
    assert len(recs) >= 10
    for c in recs:
        gens = [[genome.Genome.from_one_seq(s[0]) if len(s) == 1 else
                 genome.Genome.from_chrs(dict(("c%d" % i, x) for i, x in enumerate(s)))
                 for s in grp] for grp in c["genomes"]]
        ps = [probe.Probe.from_str(s) for s in c["probes"]]
        if "np_seed" in c:
            np.random.seed(c["np_seed"])
        a = ca.Analyzer(ps, c["mismatches"], c["lcf_thres"], gens,
                        cover_extension=c["cover_extension"],
                        kmer_probe_map_k=c["kmer_probe_map_k"], rc_too=c["rc_too"])
        a.run()
        strands = (False, True) if c["rc_too"] else (False,)
        for i, grp in enumerate(c["genomes"]):
            for j in range(len(grp)):
                for r, rc in enumerate(strands):
                    assert sorted(map(list, a.target_covers[i][j][rc])) == \
                        c["target_covers"][i][j][r]
                    assert a.bp_covered[i][j][rc] == c["bp_covered"][i][j][r]
                    assert list(a.average_coverage[i][j][rc]) == \
                        c["average_coverage"][i][j][r]
        assert [a.probe_map_counts[p] for p in ps] == c["probe_map_counts"]
        # (the reference tests name their groups; the names were not recorded)
        assert [row[1:] for row in a._make_data_matrix_string()] == \
            [row[1:] for row in c["table"]]
    a.write_data_matrix_as_tsv(str(tmp_path / "a.tsv"))
    a.write_sliding_window_coverage(str(tmp_path / "s.tsv"))
    a.write_probe_map_counts(str(tmp_path / "c.tsv"))
    assert (tmp_path / "a.tsv").read_text().startswith("Genome\tNum bases covered")
    # sliding coverage against a direct count on the ranges
    cov = a.target_covers[0][0][False]
    n = gens[0][0].size()
    depth = np.zeros(n, dtype=np.int64)
    for s0, e0 in cov:
        depth[s0:e0] += 1
    sl = a.sliding_coverage[0][0][False]
    assert sl[25.0] == np.average(depth[0:50])


@pytest.mark.parametrize("first", ["dup", "hamming", "minhash"])
def test_string_pipeline_equals_object_pipeline(ctx, first):
    """ProbeDesigner's string pipeline (no Probe object per candidate) selects
    what the filter-by-filter pipeline on Probe objects selects, for every
    first filter bin/design.py can put before the set cover filter."""
    from catch_amd import genome
    from catch_amd.filter import (duplicate_filter, near_duplicate_filter,
                                  probe_designer, set_cover_filter)
    rng = np.random.Generator(np.random.PCG64(71))
    from catch_amd.utils import synthetic
    groups = [[genome.Genome.from_one_seq(g[0]) for g in
               synthetic.make_species(rng, [3000], 5, 2, 0.04, 0.01)],
              [genome.Genome.from_one_seq(g[0]) for g in
               synthetic.make_species(rng, [2200], 4, 2, 0.05, 0.02)]]

    def filters():
        f0 = {"dup": duplicate_filter.DuplicateFilter,
              "hamming": lambda: near_duplicate_filter.NearDuplicateFilterWithHammingDistance(2, 100),
              "minhash": lambda: near_duplicate_filter.NearDuplicateFilterWithMinHash(0.5)}[first]()
        return [f0, set_cover_filter.SetCoverFilter(mismatches=3, lcf_thres=100,
                                                    cover_extension=20)]
    random.seed(9)
    a = probe_designer.ProbeDesigner(groups, filters(), 100, 50)
    a.design()                                   # string pipeline
    random.seed(9)
    b = probe_designer.ProbeDesigner(groups, filters(), 100, 50)
    cands, probes = b._design_for_genomes(groups, b.filters)   # object pipeline
    want = list(dict.fromkeys(p for g in probes for p in g))
    assert sorted(p.seq_str for p in a.final_probes) == sorted(p.seq_str for p in want)
    assert [p.seq_str for p in a.candidate_probes] == [p.seq_str for g in cands for p in g]


@pytest.mark.parametrize("first", ["dup", "hamming", "minhash"])
@pytest.mark.parametrize("m", [2, 5])
def test_prefetched_groups_select_what_inline_groups_select(ctx, monkeypatch, first, m):
    """The device front end with the NEXT groups packed and uploaded on the
    upload context while the current chunk computes (objects change hands via
    catchhip_*_rebind) == the same groups built one after the other on the
    compute context: same probes in the same order, with pigeonhole (-m 2) and
    random (-m 5: np.random) anchors, and with LSH filters that draw from
    `random` group after group.  Seven groups, so that chunks of one (large
    groups alone) and of several (small ones in flight together) both occur."""
    from catch_amd import genome
    from catch_amd.filter import near_duplicate_filter, set_cover_filter
    from catch_amd.utils import synthetic
    monkeypatch.setenv("CATCHHIP_BIG_GROUP_BASES", "20000")
    rng = np.random.Generator(np.random.PCG64(1234 + m))
    groups = [[genome.Genome.from_one_seq(g[0]) for g in
               synthetic.make_species(rng, [int(ln)], n, 2, 0.04, 0.01)]
              for ln, n in ((9000, 6), (2500, 3), (2600, 4), (15000, 3), (2400, 2), (3000, 3), (2800, 5))]

    def run(depth):
        monkeypatch.setenv("CATCHHIP_PREFETCH_DEPTH", str(depth))
        random.seed(5)
        np.random.seed(6)
        ndf = {"dup": lambda: None,
               "hamming": lambda: near_duplicate_filter.NearDuplicateFilterWithHammingDistance(2, 100),
               "minhash": lambda: near_duplicate_filter.NearDuplicateFilterWithMinHash(0.5)}[first]()
        scf = set_cover_filter.SetCoverFilter(mismatches=m, lcf_thres=100, cover_extension=25)
        out = scf._filter_genomes_device(groups, 100, 50, None, ndf)
        tm = scf.last_timings
        ids = None
        if first == "dup":
            np.random.seed(6)            # the same random anchors (-m 5) as the call above
            ids = scf._filter_genomes_device(groups, 100, 50, None, ndf, return_ids=True)
        return out, ids, tm

    inline, ids0, t0 = run(0)
    ahead, ids2, t2 = run(2)
    deep, ids5, t5 = run(5)
    assert inline == ahead == deep
    assert ids0 == ids2 == ids5
    assert all(len(g) > 0 for g in inline)
    if ids0 is not None:
        assert [len(g) for g in ids0] == [len(g) for g in inline]
    assert t0["picks"] == t2["picks"] == t5["picks"] and t0["probe_bp_units"] == t2["probe_bp_units"] > 0


def test_ndf_hamming_counts_its_pairs(ctx):
    """catchhip_ctx_last_ndf_counters: probes, tables, pairs compared (SURVEY
    8(d) K3's C) and edges of the last Hamming filter."""
    engine = _engine()
    from catch_amd.utils import lsh
    rng = np.random.Generator(np.random.PCG64(99))
    base = rng.integers(0, 4, size=100)
    strs = []
    for i in range(400):
        v = base.copy()
        for j in rng.integers(0, 100, size=int(rng.integers(0, 4))):
            v[j] = (v[j] + 1) & 3
        strs.append("".join("ACGT"[c] for c in v))
    strs = list(dict.fromkeys(strs))
    random.seed(3)
    pos = np.array([sorted(random.sample(range(100), 20)) for _ in range(5)], dtype=np.int32)
    keep = ctx.ndf_hamming(strs, 100, pos, 2)
    cn = ctx.ndf_counters()
    assert cn["probes"] == len(strs) and cn["tables"] == 5
    assert cn["pairs_compared"] >= cn["edges"] > 0
    assert 0 < int(keep.sum()) < len(strs)


# ---------------------------------------------------------------- clustering pre-step
def test_signatures_golden(ctx):
    """MinHash signatures (md5 of every k-mer, N smallest) == the reference's
    (lsh.MinHashFamily.make_h, recorded), incl. sequences with fewer than N
    k-mers."""
    engine = _engine()
    g = load_golden("cluster")
    recs = g["from_reference_tests"]["minhash"] + g["synthetic"]
    assert len(recs) >= 8
    for c in recs:
        s = engine.Signatures(ctx, c["seqs"], c["k"], c["N"], c["a"], c["b"])
        got = s.fetch()
        s.close()
        assert got.tolist() == c["signatures"]


def test_signatures_and_distances_match_oracle(ctx, oracle):
    """Random sequences of ragged lengths (down to the k-mer size), any
    characters, several (k, N): signatures, the row walk and the condensed
    float32 matrix against the CPU restatement."""
    engine = _engine()
    rnd = random.Random(17)
    for k, N, nseq, maxlen in [(12, 100, 40, 900), (1, 5, 9, 30), (3, 64, 30, 200), (16, 1, 25, 300),
                               (31, 300, 12, 1500), (55, 1024, 6, 1400), (12, 100, 7, 40), (20, 257, 21, 500)]:
        root = "".join(rnd.choice("ACGT") for _ in range(maxlen))
        seqs = []
        for i in range(nseq):
            ln = rnd.randrange(k, maxlen + 1)
            st = rnd.randrange(0, maxlen - ln + 1)
            s = list(root[st:st + ln])
            for _ in range(rnd.choice([0, 0, 1, 3, 10, 40])):
                s[rnd.randrange(ln)] = rnd.choice("ACGTNacgtRY-")
            seqs.append("".join(s))
        seqs[0] = seqs[-1]                      # identical pair
        a, b = rnd.randint(1, 2 ** 31 - 1), rnd.randint(0, 2 ** 31 - 1)
        if k == 1:
            a, b = 2 ** 31 - 1, 2 ** 31 - 1     # extremes of the draw
        sigs = engine.Signatures(ctx, seqs, k, N, a, b)
        got = sigs.fetch()
        want = [oracle.minhash_signature(s, k, N, a, b) for s in seqs]
        assert got.tolist() == [list(w) for w in want]
        for j in (0, nseq // 2, nseq - 1):
            row = sigs.common_row(j)
            for q in range(nseq):
                inter, union = oracle.signature_common(want[j], want[q], N)
                assert union == N
                assert int(row[q]) == inter
        lut = (1.0 - np.arange(N + 1, dtype=np.float64) / float(N)).astype(np.float32)
        cond = sigs.condensed(lut)
        ref = oracle.condensed_dist_matrix(
            nseq, lambda i, j: oracle.estimate_jaccard_dist(want[i], want[j], N))
        assert cond.dtype == np.float32 and np.array_equal(cond, ref)
        sigs.close()
    e = engine.Signatures(ctx, [], 12, 100, 1, 0)
    assert e.fetch().shape == (0, 100)
    e.close()
    with pytest.raises(Exception):
        engine.Signatures(ctx, ["ACGT"], 12, 100, 1, 0)     # shorter than k


def test_signatures_of_long_sequences(ctx, oracle):
    """One 300-kb and many 5-kb sequences: radix select over long hash arrays,
    tiles crossing sequence ends."""
    engine = _engine()
    rng = np.random.Generator(np.random.PCG64(3))
    seqs = ["".join("ACGT"[x] for x in rng.integers(0, 4, size=300_000))]
    seqs += ["".join("ACGT"[x] for x in rng.integers(0, 4, size=int(n)))
             for n in rng.integers(1000, 5000, size=60)]
    seqs.append("AC" * 20_000)                  # two distinct 12-mers, heavy multiplicity
    a, b = 123456789, 987654321
    sigs = engine.Signatures(ctx, seqs, 12, 100, a, b)
    got = sigs.fetch()
    sigs.close()
    for i in (0, 1, 30, 60, 61):
        assert got[i].tolist() == list(oracle.minhash_signature(seqs[i], 12, 100, a, b))


def test_cluster_neighbor_lists_equal_full_rows(ctx, monkeypatch):
    """The connected-components search fed by device-made neighbour lists
    (catchhip_sigs_neighbors, used while the set difference is known to iterate
    in ascending order) == the search on full distance rows, on S5-shaped
    fragments (many singletons, a few clusters of hundreds)."""
    from catch_amd.utils import cluster, synthetic
    genomes = synthetic.dataset("S5", scale=0.004)[0]
    seqs = dict(enumerate(s for g in genomes for s in g))
    assert len(seqs) > 300
    random.seed(5)
    fast = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    monkeypatch.setenv("CATCHHIP_CLUSTER_ROWS_ONLY", "1")
    random.seed(5)
    rows = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    assert fast == rows
    assert 1 < len(fast) < len(seqs)


def test_cluster_neighbor_lists_many_and_one_by_one(ctx, monkeypatch):
    """catchhip_sigs_graph (all lists in one pass) == catchhip_sigs_neighbors_many
    (the lists of up to 32 vertices per launch)
    == catchhip_sigs_neighbors vertex by vertex == the full rows; and the search
    that asks for the stack's top along with the explored vertex == the search
    that asks one by one, on an input large enough for the tail of the search
    (differences that are copies of `remaining`, ranked once per component)."""
    from catch_amd.utils import cluster, lsh, synthetic
    genomes = synthetic.dataset("S5", scale=0.02)[0]
    seqs = dict(enumerate(s for g in genomes for s in g))
    random.seed(6)
    fam = lsh.MinHashFamily(12, N=100)
    sigs = fam.signatures(list(seqs.values()))
    try:
        rng = np.random.RandomState(3)
        for nq in (1, 2, 31, 32):
            js = rng.choice(sigs.n, size=nq, replace=False)
            many = sigs.neighbors_many(js, 20)
            for j, (idx, com) in zip(js, many):
                i1, c1 = sigs.neighbors(int(j), 20)
                assert np.array_equal(idx, i1) and np.array_equal(com, c1)
                row = sigs.common_row(int(j)).astype(np.int64)
                assert np.array_equal(idx, np.nonzero(row >= 20)[0]) and np.array_equal(com, row[idx])
        # the whole graph in one pass (catchhip_sigs_graph): every row == the vertex's own list without itself
        ptr, gidx, gcom = sigs.graph(20)
        assert ptr[0] == 0 and ptr[-1] == gidx.size and np.all(np.diff(ptr) >= 0)
        for j in list(rng.choice(sigs.n, size=40, replace=False)) + [0, sigs.n - 1]:
            i1, c1 = sigs.neighbors(int(j), 20)
            keep = i1 != j
            assert np.array_equal(gidx[ptr[j]:ptr[j + 1]], i1[keep]) and np.array_equal(gcom[ptr[j]:ptr[j + 1]], c1[keep])
        # symmetric, and no more edges than it has room for when asked to give up early
        deg = np.diff(ptr)
        src = np.repeat(np.arange(sigs.n), deg)
        fwd = set(zip(src[:5000].tolist(), gidx[:5000].tolist()))
        assert all((gidx[a + int(np.searchsorted(gidx[a:b], q))] == q) for q, k in fwd for a, b in [(ptr[k], ptr[k + 1])])
        sigs.GRAPH_MAX_EDGES = max(int(gidx.size) // 2, 1)
        assert sigs.graph(20) is None
        del sigs.GRAPH_MAX_EDGES
    finally:
        sigs.close()
    before = dict(cluster._path_counts)
    random.seed(5)
    graph = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    took = {k: cluster._path_counts[k] - before[k] for k in before}
    assert took["graphs"] == 1 and took["copy rank"] > 100 and took["list calls"] == 0, took
    # ... the same graph walked by the interpreter instead of catchhip_dfs_*: same components, same cases
    monkeypatch.setenv("CATCHHIP_CLUSTER_PYTHON_SEARCH", "1")
    before = dict(cluster._path_counts)
    random.seed(5)
    graph_py = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    took_py = {k: cluster._path_counts[k] - before[k] for k in before}
    assert graph_py == graph and took_py == took, (took_py, took)
    monkeypatch.delenv("CATCHHIP_CLUSTER_PYTHON_SEARCH")
    monkeypatch.setenv("CATCHHIP_CLUSTER_NO_GRAPH", "1")
    before = dict(cluster._path_counts)
    random.seed(5)
    many = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    took = {k: cluster._path_counts[k] - before[k] for k in before}
    assert took["copy rank"] > 100 and took["list calls"] < (took["ascending"] + took["copy rank"]) // 2, took
    assert graph == many
    monkeypatch.setenv("CATCHHIP_CLUSTER_ONE_BY_ONE", "1")
    random.seed(5)
    one = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    monkeypatch.setenv("CATCHHIP_CLUSTER_ROWS_ONLY", "1")
    random.seed(5)
    rows = cluster.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    assert many == one == rows


def test_minhash_filter_lazy_resolution_equals_all_pairs(ctx, monkeypatch):
    """The MinHash filter's lazy resolution (a cursor per table and slot over
    the higher-priority mates of its run; only kept and undecided mates are
    ever compared) keeps exactly the probes the all-pairs edge list + rounds
    keep (CATCHHIP_MH_ALL_PAIRS=1), on candidates with long runs of
    near-identical probes (strains of one species) next to unrelated ones,
    with and without groups."""
    from catch_amd import engine
    from catch_amd.filter import candidate_probes
    from catch_amd.utils import synthetic
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithMinHash
    groups = synthetic.dataset("S5m", scale=0.02)[0]
    seqs = [s for g in groups for s in g]
    cands = list(dict.fromkeys(candidate_probes.candidate_strings_from_sequences(seqs, 100, 50)))
    assert len(cands) > 20000
    out = {}
    for mode in ("lazy", "polling rounds", "all pairs"):
        if mode == "polling rounds":       # round 3's form of the lazy resolution (every unexhausted cursor listed every round)
            monkeypatch.setenv("CATCHHIP_NDF_POLL_ROUNDS", "1")
        if mode == "all pairs":
            monkeypatch.delenv("CATCHHIP_NDF_POLL_ROUNDS")
            monkeypatch.setenv("CATCHHIP_MH_ALL_PAIRS", "1")
        random.seed(41)
        ndf = NearDuplicateFilterWithMinHash(0.6)
        kept = ndf._filter_strs(cands)
        random.seed(41)
        ndf = NearDuplicateFilterWithMinHash(0.6)
        third = len(cands) // 3
        many = ndf._filter_strs_many([cands[:third], cands[third:2 * third], cands[2 * third:]])
        out[mode] = (kept, many, ctx.ndf_counters()["pairs_compared"])
    assert out["lazy"][0] == out["all pairs"][0] and out["lazy"][1] == out["all pairs"][1]
    assert out["lazy"][0] == out["polling rounds"][0] and out["lazy"][1] == out["polling rounds"][1]
    assert 0 < len(out["lazy"][0]) < len(cands)
    assert out["lazy"][2] < out["all pairs"][2]      # and with far fewer comparisons
    # the Hamming family likewise (CATCHHIP_NDF_ALL_PAIRS=1), several tables
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithHammingDistance
    monkeypatch.delenv("CATCHHIP_MH_ALL_PAIRS")
    ham = {}
    for mode in ("lazy", "polling rounds", "all pairs"):
        if mode == "polling rounds":
            monkeypatch.setenv("CATCHHIP_NDF_POLL_ROUNDS", "1")
        if mode == "all pairs":
            monkeypatch.delenv("CATCHHIP_NDF_POLL_ROUNDS")
            monkeypatch.setenv("CATCHHIP_NDF_ALL_PAIRS", "1")
        res = []
        for thres in (2, 6):
            random.seed(43)
            res.append(NearDuplicateFilterWithHammingDistance(thres, 100)._filter_strs(cands))
            res.append(ctx.ndf_counters()["pairs_compared"])
        ham[mode] = res
    assert ham["lazy"][0] == ham["all pairs"][0] and ham["lazy"][2] == ham["all pairs"][2]
    assert ham["lazy"][0] == ham["polling rounds"][0] and ham["lazy"][2] == ham["polling rounds"][2]
    assert 0 < len(ham["lazy"][2]) < len(ham["lazy"][0]) <= len(cands)
    assert ham["lazy"][1] < ham["all pairs"][1] and ham["lazy"][3] < ham["all pairs"][3]


@pytest.mark.parametrize("hook", ["CATCHHIP_MH_NO_WAVE64", "CATCHHIP_NDF_NO_QUEUE", "CATCHHIP_NDF_NO_PROBE_PASS",
                                  "CATCHHIP_NDF_PROBE_ROUND0", "CATCHHIP_NDF_NO_PACKED_STATES"])
def test_near_duplicate_filter_pass_forms_agree(ctx, monkeypatch, hook):
    """Round 5's forms of the lazy resolution -- walks with the probe's k-mer codes staged in LDS, deferred walks
    drained from a queue, one wavefront per woken probe, the first slot of a run settled by the init launch, states
    packed 2 bits per probe -- keep exactly the probes the round-4 forms keep (each hook switches one of them off,
    CATCHHIP_NDF_PROBE_ROUND0 sends round 0 through the probe kernel too): both families, with and without groups,
    on strains of one species next to unrelated sequences, incl. probes with N (no 2-bit codes: 16-byte ids)."""
    from catch_amd.filter import candidate_probes
    from catch_amd.utils import synthetic
    from catch_amd.filter.near_duplicate_filter import (NearDuplicateFilterWithMinHash,
                                                        NearDuplicateFilterWithHammingDistance)
    groups = synthetic.dataset("S5m", scale=0.02)[0]
    seqs = [s for g in groups for s in g]
    cands = list(dict.fromkeys(candidate_probes.candidate_strings_from_sequences(seqs, 100, 50)))
    cands += [c[:37] + "N" + c[38:] for c in cands[:300]]          # single N: such windows are candidates in CATCH
    third = len(cands) // 3

    def run():
        random.seed(41)
        a = NearDuplicateFilterWithMinHash(0.6)._filter_strs(cands)
        random.seed(41)
        b = NearDuplicateFilterWithMinHash(0.6)._filter_strs_many([cands[:third], cands[third:2 * third], cands[2 * third:]])
        random.seed(43)
        c = NearDuplicateFilterWithHammingDistance(6, 100)._filter_strs(cands)
        return a, b, c
    want = run()
    monkeypatch.setenv(hook, "1")
    got = run()
    assert got == want and 0 < len(want[0]) < len(cands) and 0 < len(want[2]) < len(cands)


def test_fuzz_case_whose_wake_ups_only_drop(ctx):
    """tests/fuzz_parity.py seed 31188 (round 5): 5,608 candidates of near-identical small groups, 13 MinHash tables --
    after a compaction keeps probes whose last tables ran out, a round without a pass only DROPS probes (parked on
    the newly kept ones) and wakes nobody; the loop must go on (its first stuck-check stopped there)."""
    import fuzz_parity
    fuzz_parity.one_case(31188, ctx, kmer_size=10)       # (k-mers of 10: the size the seed drew when it was found)


@pytest.mark.parametrize("seed,kmer_size", [(28, 6), (2, 13), (7, 16)])
def test_fuzz_cases_at_the_other_minhash_kmer_sizes(ctx, seed, kmer_size):
    """tests/fuzz_parity.py draws the MinHash filter's k-mer size from 6, 8, 10, 13 and 16 (8 and 10 until round 6):
    one seed of each of the other sizes -- below a SipHash block, two id words, no 2-bit codes."""
    import fuzz_parity
    assert fuzz_parity.minhash_kmer_size(seed) == kmer_size
    saved = {name: os.environ.get(name) for name in fuzz_parity.SOLVER_ENV}
    try:
        assert fuzz_parity.one_case(seed, ctx)["minhash_kmer_size"] == kmer_size
    finally:                                    # (a case sets the switches of its solver variant: put back what was there)
        for name, value in saved.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


def test_cluster_with_minhash_signatures_golden(ctx):
    """cluster.cluster_with_minhash_signatures (signatures + distances on the
    device, search / linkage on the host) == the reference's clusters, same
    order, for both methods."""
    from catch_amd.utils import cluster
    g = load_golden("cluster")
    recs = [c for c in g["from_reference_tests"]["minhash"]] + g["synthetic"]
    for c in recs:
        if "seed" not in c:
            continue
        random.seed(c["seed"])
        seqs = dict(zip(c["names"], c["seqs"]))
        got = cluster.cluster_with_minhash_signatures(
            seqs, k=c["k"], N=c["N"], threshold=c["threshold"], cluster_method=c["method"])
        assert got == c["out"]
    # the reference's own test inputs (catch/utils/tests/test_cluster.py:193-226):
    # recorded (a, b) are replayed through the family
    from catch_amd.utils import lsh
    for c in g["from_reference_tests"]["minhash"]:
        fam = lsh.MinHashFamily(c["k"], N=c["N"])
        sigs = fam.signatures(c["seqs"], ab=(c["a"], c["b"]))
        thr = cluster._jaccard_dist_from_mash_dist(c["threshold"], c["k"])
        if c["method"] == "simple":
            cl = cluster._components_of_signatures(sigs, thr)
        else:
            lut = (1.0 - np.arange(c["N"] + 1, dtype=np.float64) / float(c["N"])).astype(np.float32)
            cl = cluster.cluster_hierarchically_from_dist_matrix(sigs.condensed(lut), thr)
        sigs.close()
        assert [[c["names"][i] for i in x] for x in cl] == c["out"]


def test_probe_designer_with_clustering_golden(ctx):
    """ProbeDesigner with cluster_threshold: the clustered genomes and the
    final probe set of the reference (DuplicateFilter + SetCoverFilter per
    cluster, merged after the set cover filter)."""
    from catch_amd.filter import duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.genome import Genome
    from collections import OrderedDict
    g = load_golden("cluster")
    assert len(g["designs"]) >= 4
    for c in g["designs"]:
        groups = [[Genome.from_chrs(OrderedDict(("c%d" % i, s) for i, s in enumerate(gn)))
                   if len(gn) > 1 else Genome.from_one_seq(gn[0]) for gn in grp]
                  for grp in c["genomes"]]
        for use_strings in (True, False):
            df = duplicate_filter.DuplicateFilter()
            f = set_cover_filter.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0,
                                                cover_extension=20)
            pd = probe_designer.ProbeDesigner(
                groups, [df, f], probe_length=100, probe_stride=50,
                seq_length_to_skip=c["seq_length_to_skip"], cluster_threshold=c["threshold"],
                cluster_merge_after=f, cluster_method=c["method"],
                cluster_fragment_length=c["fragment_length"])
            if not use_strings:
                pd._strings_path_ok = lambda filters: False
            random.seed(c["seed"])
            clustered = pd._cluster_genomes()
            assert [[x.seqs[0] for x in cl] for cl in clustered] == c["clustered"]
            random.seed(c["seed"])
            pd.design()
            assert sorted(p.seq_str for p in pd.final_probes) == c["final"]
            assert len(pd.candidate_probes) == c["n_candidates"]


# ---------------------------------------------------------------- adapter filter
def _first_seen_device(ctx, uniq, entries, k, seqs, m, thres, island, ent_rank, mode=0):
    engine = _engine()
    ep = np.array([e[0] for e in entries], dtype=np.int32)
    eo = np.array([e[1] for e in entries], dtype=np.int32)
    t = engine.Targets(ctx, [[s] for s in seqs])
    p = engine.Probes(ctx, uniq, np.arange(len(uniq), dtype=np.int32), ep, eo, k)
    rows = engine.Rows.scan_first_seen(ctx, p, t, m, thres, island, 0, mode,
                                       np.asarray(ent_rank, dtype=np.uint32))
    sid, univ, st, en = rows.fetch()
    key = rows.fetch_first_seen()
    rows.close(); p.close(); t.close()
    return sid, univ, st, en, key


@pytest.mark.parametrize("L,m,thres,island,min_k", [(100, 2, 100, 0, 20), (75, 2, 75, 0, 20), (100, 5, 100, 0, 20),
                                                     (100, 3, 80, 0, 20), (75, 2, 60, 25, 10), (60, 1, 60, 0, 20),
                                                     (224, 2, 224, 0, 20)])
def test_first_seen_keys_match_oracle(ctx, oracle, L, m, thres, island, min_k):
    """catchhip_cover_scan_first_seen: merged rows as catchhip_cover_scan, and
    for every (probe, sequence) the first accepted seed (position, caller's
    entry rank) of the reference's left-to-right scan -- seed path (pigeonhole
    and random anchors) and general path."""
    genomes = small_species(seed=5, n=5, length=2500, d1=0.03, d2=0.004)
    seqs = [g[0] for g in genomes]
    strs = candidates(genomes, L, 20)[::2]
    np.random.seed(3)
    k, entries, draws = oracle.anchor_table(strs, m, thres, min_k=min_k, k=min_k, with_draws=True)
    uniq, _ = oracle._unique_last(strs)
    rnd = random.Random(1)
    ent_rank = [rnd.randrange(0, 5) for _ in entries]      # ties on purpose
    # distinct ranks inside a k-mer's entry list, as the host guarantees
    seen = {}
    for j, (p, pos) in enumerate(entries):
        km = uniq[p][pos:pos + k]
        ent_rank[j] = seen.get(km, 0)
        seen[km] = ent_rank[j] + 1
    sid, univ, st, en, key = _first_seen_device(ctx, uniq, entries, k, seqs, m, thres, island, ent_rank)
    want_rows, want_key = [], {}
    for u, s in enumerate(seqs):
        cov = oracle.scan_sequence(s, uniq, entries, k, m, thres, island, merge=True)
        first = oracle.scan_first_seen(s, uniq, entries, k, m, thres, island, ent_rank)
        assert set(cov) == set(first)
        for p, ranges in cov.items():
            for a, b in ranges:
                want_rows.append((p, u, a, b))
            want_key[(p, u)] = (first[p][0] << 32) | ent_rank[first[p][1]]
    assert rows_as_tuples(sid, univ, st, en) == sorted(want_rows)
    assert len(want_rows) > 50
    for i in range(len(sid)):
        assert int(key[i]) == want_key[(int(sid[i]), int(univ[i]))]


class _Seed0Probe:
    """Probe whose hash is CPython's string hash under PYTHONHASHSEED=0
    (computed by the oracle's SipHash): with these the product reproduces the
    tie-breaks of the reference run that recorded the golden vectors."""

    def __init__(self, s, h):
        self.seq_str, self._h = s, h

    def __hash__(self):
        return self._h

    def __eq__(self, other):
        return self.seq_str == other.seq_str

    def with_prepended_str(self, s):
        return _Seed0Probe(s + self.seq_str, 0)

    def with_appended_str(self, s):
        return _Seed0Probe(self.seq_str + s, 0)


def test_adapter_filter_golden(ctx, oracle):
    """AdapterFilter votes and output == the reference's (its own tests + six
    synthetic designs with many equal-end ties, random and pigeonhole anchors,
    island, duplicate probes)."""
    import sys
    from catch_amd.filter.adapter_filter import AdapterFilter
    from catch_amd.genome import Genome
    g = load_golden("adapter_filter")
    same_python = g["python"].split(".")[:2] == sys.version.split()[0].split(".")[:2]
    for c in g["from_reference_tests"] + g["synthetic"]:
        probes = [_Seed0Probe(s, oracle.pyhash_seed0(s)) for s in c["probes"]]
        gens = [[Genome.from_one_seq(s) for s in c["sequences"]]]
        f = AdapterFilter(tuple(c["adapters"][0]), tuple(c["adapters"][1]), c["mismatches"], c["lcf_thres"],
                          island_of_exact_match=c.get("island", 0), kmer_probe_map_k=c["kmer_probe_map_k"])
        np.random.set_state(np_state_from_json(c["np_state"]))
        votes = f._make_votes_across_target_genomes(probes, gens)
        assert [a + b for a, b in votes] == [a + b for a, b in c["votes"]]
        if same_python:
            assert [list(v) for v in votes] == c["votes"]
            if "out" in c:
                np.random.set_state(np_state_from_json(c["np_state"]))
                out = f.filter(probes, gens)
                assert [p.seq_str for p in out] == c["out"]


def test_adapter_filter_matches_oracle_in_this_interpreter(ctx, oracle):
    """With ordinary Probe objects the ties follow this interpreter's own
    string hash -- what the reference would do in this very process."""
    from catch_amd import probe
    from catch_amd.filter.adapter_filter import AdapterFilter
    from catch_amd.genome import Genome
    genomes = small_species(seed=8, n=6, length=3000, d1=0.03, d2=0.005)
    seqs = [g[0] for g in genomes]
    for L, m, thres, kmap in ((100, 2, 100, 20), (100, 3, 70, 15)):
        strs = candidates(genomes, L, 25)[::2]
        strs = strs + strs[:5]
        f = AdapterFilter(("AC", "GT"), ("TT", "GG"), m, thres, kmer_probe_map_k=kmap)
        np.random.seed(4)
        got = f.filter([probe.Probe.from_str(s) for s in strs], [[Genome.from_one_seq(s) for s in seqs]])
        np.random.seed(4)
        want = oracle.adapter_filter(strs, seqs, ("AC", "GT"), ("TT", "GG"), m, thres, 0, kmap, hash_fn=hash)
        assert [p.seq_str for p in got] == want
        assert len({w[:2] for w in want}) == 2      # both adapters in use
    with pytest.raises(ValueError):
        AdapterFilter(("A",), ("C", "G"), 1, 10)
    with pytest.raises(NotImplementedError):
        AdapterFilter(("A", "C"), ("C", "G"), 1, 10, custom_cover_range_fn=("x.py", "f"))


def test_design_cli_with_clustering_and_adapters(ctx, oracle, tmp_path, capsys):
    """python -m catch_amd.design --cluster-and-design-separately ... --add-adapters:
    clusters == oracle clustering of the same sequences, probes == oracle set
    cover per cluster, adapters == oracle adapter votes over the clustered
    sequences (this interpreter's string hash on both sides)."""
    from catch_amd import design
    from catch_amd.utils import synthetic, seq_io
    rng = np.random.Generator(np.random.PCG64(45))
    groups = [synthetic.make_species(rng, [2600], 4, 2, 0.05, 0.01, with_n=False),
              synthetic.make_species(rng, [1900], 3, 1, 0.0, 0.02, with_n=False)]
    files = []
    for i, grp in enumerate(groups):
        fn = tmp_path / ("d%d.fasta" % i)
        fn.write_text("".join(">g%d\n%s\n" % (j, g[0]) for j, g in enumerate(grp)))
        files.append(str(fn))
    out = tmp_path / "probes.fasta"
    random.seed(9)
    pb = design.main(design.parse_args(files + [
        "-pl", "100", "-ps", "50", "-m", "2", "-e", "20", "-o", str(out),
        "--cluster-and-design-separately", "0.15", "--cluster-and-design-separately-method", "simple",
        "--add-adapters", "--adapter-a", "AAAA", "CCCC", "--adapter-b", "GGGG", "TTTT"]))
    capsys.readouterr()
    seqs = [g[0] for grp in groups for g in grp]
    random.seed(9)
    clusters = oracle.cluster_with_minhash_signatures(seqs, threshold=0.15, cluster_method="simple")
    assert len(clusters) == 2
    cl_genomes = [[[seqs[i]] for i in c] for c in clusters]
    cands = [candidates(g, 100, 50) for g in cl_genomes]
    exp = oracle.set_cover_filter(cands, cl_genomes, 2, 100, coverage=1.0, cover_extension=20)
    chosen = list(dict.fromkeys(cands[i][j] for i, ids in enumerate(exp) for j in ids))
    all_seqs = [s for c in cl_genomes for g in c for s in g]
    want = oracle.adapter_filter(chosen, all_seqs, ("AAAA", "CCCC"), ("GGGG", "TTTT"), 2, 100, 0, 20,
                                 hash_fn=hash)
    got = list(seq_io.read_fasta(str(out)).values())
    assert sorted(got) == sorted(want)
    assert len(pb.final_probes) == len(want)


def test_config5_pipeline_large_profile_matches_oracle(ctx, oracle, tmp_path, capsys):
    """config 5 shape (design_large defaults: -m 5 -e 50, cluster 0.15 from
    fragments, MinHash near-duplicate filter 0.6, then the set cover per
    cluster) == the oracle's chain of the same steps."""
    from catch_amd import design
    from catch_amd.utils import synthetic, seq_io
    rng = np.random.Generator(np.random.PCG64(46))
    sp = [synthetic.make_species(rng, [2600], 4, 2, 0.06, 0.01, with_n=False),
          synthetic.make_species(rng, [2100], 3, 1, 0.0, 0.02, with_n=False),
          synthetic.make_species(rng, [3300], 2, 1, 0.0, 0.03, with_n=False)]
    fn = tmp_path / "all.fasta"
    fn.write_text("".join(">s%d_%d\n%s\n" % (i, j, g[0]) for i, grp in enumerate(sp) for j, g in enumerate(grp)))
    out = tmp_path / "probes.fasta"
    args = design.parse_args([str(fn), "-o", str(out), "--cluster-from-fragments", "1000",
                              "--cluster-and-design-separately-method", "simple"], args_type="large")
    assert (args.mismatches, args.cover_extension, args.filter_with_lsh_minhash,
            args.cluster_and_design_separately) == (5, 50, 0.6, 0.15)
    random.seed(21)
    np.random.seed(22)
    pb = design.main(args)
    capsys.readouterr()
    frags = [f for grp in sp for g in grp for f in oracle.fragments_of(g[0], 1000)]
    random.seed(21)
    np.random.seed(22)
    clusters = oracle.cluster_with_minhash_signatures(frags, threshold=0.15, cluster_method="simple")
    assert 3 <= len(clusters) < len(frags)
    cl_genomes = [[[frags[i]] for i in c] for c in clusters]
    kept = []
    for g in cl_genomes:
        cands = candidates(g, 100, 50, dedup=False)
        params = oracle.minhash_draw_params(oracle.minhash_num_tables(0.6), 3)
        kept.append(oracle.ndf_minhash(cands, 0.6, params))
    exp = oracle.set_cover_filter(kept, cl_genomes, 5, 100, coverage=1.0, cover_extension=50)
    want = set(kept[i][j] for i, ids in enumerate(exp) for j in ids)
    got = set(seq_io.read_fasta(str(out)).values())
    assert got == want and len(pb.final_probes) == len(want) > 10


def test_ndf_minhash_many_groups_equals_per_group_calls(ctx, oracle):
    """catchhip_ndf_minhash_many (all clusters in one pass, hash functions per
    group) == one catchhip_ndf_minhash call per group == the oracle."""
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithMinHash
    groups = []
    for seed, n in ((1, 5), (2, 1), (3, 7), (4, 3)):
        g = small_species(seed=seed, n=n, length=1500, d1=0.05, d2=0.02, with_n=(seed % 2 == 0))
        groups.append(candidates(g, 100, 50, dedup=False))
    groups.insert(2, [])                       # an empty cluster
    groups.append(groups[0][:40])              # same probes in another group: no cross-talk
    f = NearDuplicateFilterWithMinHash(0.6)
    random.seed(77)
    many = f._filter_strs_many(groups)
    random.seed(77)
    single = [f._filter_strs(g) for g in groups]
    assert many == single
    random.seed(77)
    for g, got in zip(groups, many):
        params = oracle.minhash_draw_params(oracle.minhash_num_tables(0.6), 3)
        assert got == oracle.ndf_minhash(g, 0.6, params)
    assert any(0 < len(k) < len(g) for k, g in zip(many, groups))


@pytest.mark.parametrize("m,coverage,ext", [(2, 1.0, 50), (5, 1.0, 50), (3, 0.9, 0), (2, 1.0, 0)])
def test_union_of_groups_equals_per_group(ctx, oracle, monkeypatch, m, coverage, ext):
    """Many groups solved as one instance (catchhip_*_set_groups + one fused
    call) == one call per group == the oracle per group, picks in the same
    order; the groups are strains of the same species, so without the group
    filter probes would also cover other groups' genomes."""
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.genome import Genome
    sp = (small_species(seed=12, n=14, length=2200, d1=0.03, d2=0.01) +
          small_species(seed=13, n=10, length=1700, d1=0.04, d2=0.01, with_n=False))
    groups = [sp[i:i + 2] for i in range(0, len(sp), 2)]          # 12 groups of 2 genomes
    cands = [candidates(g, 100, 50) for g in groups]
    gens = [[Genome.from_one_seq(x[0]) for x in g] for g in groups]
    f = SetCoverFilter(mismatches=m, lcf_thres=100, coverage=coverage, cover_extension=ext)
    np.random.seed(31)
    union = f._filter_strs(cands, gens, assume_unique=True)
    monkeypatch.setenv("CATCHHIP_UNION_MIN_GROUPS", "999")
    np.random.seed(31)
    single = f._filter_strs(cands, gens, assume_unique=True)
    assert union == single
    np.random.seed(31)
    want = oracle.set_cover_filter(cands, groups, m, 100, coverage=coverage, cover_extension=ext)
    assert [sorted(u) for u in union] == [sorted(w) for w in want]
    assert sum(map(len, union)) > 50


# ---------------------------------------------------------------- device front end
def _rand_seq_with_n_runs(rnd, n):
    s = [rnd.choice("ACGT") for _ in range(n)]
    for _ in range(rnd.choice([0, 0, 1, 2, 5])):
        a = rnd.randrange(0, n)
        ln = rnd.choice([1, 1, 2, 3, 7, 40])
        s[a:a + ln] = "N" * min(ln, n - a)
    if rnd.random() < 0.2:
        s[:3] = "NNN"
    if rnd.random() < 0.2:
        s[-2:] = "NN"
    return "".join(s)


@pytest.mark.parametrize("bits", ["0", "3", "9"])
def test_device_candidates_with_hash_collisions(ctx, monkeypatch, bits):
    """The de-duplication stays exact when different windows share a hash
    (CATCHHIP_CAND_HASH_BITS keeps 0 / 3 / 9 bits of it): unique list,
    multiplicities (through the Hamming filter's priority order) and groups."""
    from catch_amd.filter import candidate_probes, near_duplicate_filter as ndf
    engine = _engine()
    monkeypatch.setenv("CATCHHIP_CAND_HASH_BITS", bits)
    base = small_species(seed=51, n=4, length=700, d1=0.03, d2=0.01)
    genomes = base + [base[2], base[0]]
    L, stride = 60, 20
    strs = candidates(genomes, L, stride, dedup=False)
    flat = "".join(s for g in genomes for s in g)
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, L, stride)
    assert [flat[p:p + L] for p in c.positions().tolist()] == list(dict.fromkeys(strs))
    f = ndf.NearDuplicateFilterWithHammingDistance(1, L)
    random.seed(2)
    want = f._filter_strs(strs)
    random.seed(2)
    f._apply_to_candidates(c)
    assert [flat[p:p + L] for p in c.positions().tolist()] == want
    c.close()
    # grouped: the same genomes as three groups of two
    t.set_groups([0, 0, 1, 1, 2, 2])
    c = engine.Candidates(ctx, t, L, stride)
    want_g, want_grp = [], []
    for gi in range(3):
        u = list(dict.fromkeys(candidates(genomes[2 * gi:2 * gi + 2], L, stride, dedup=False)))
        want_g += u
        want_grp += [gi] * len(u)
    assert [flat[p:p + L] for p in c.positions().tolist()] == want_g
    assert c.groups().tolist() == want_grp
    c.close(); t.close()


@pytest.mark.parametrize("L,stride", [(100, 50), (75, 25), (60, 60), (80, 33), (20, 7)])
def test_device_candidates_match_host_front_end(ctx, L, stride):
    """catchhip_candidates_create == candidate_strings_from_sequences over the
    genomes + dict.fromkeys (the reference's candidate order and duplicate
    filter), incl. N runs, tails, flanking windows and repeated genomes."""
    from catch_amd.filter import candidate_probes
    engine = _engine()
    rnd = random.Random(L * 1000 + stride)
    g = load_golden("candidate_probes")
    genomes = [[s] for s in g[0]["seqs"]]
    for _ in range(25):
        n = rnd.randrange(L, 900)
        genomes.append([_rand_seq_with_n_runs(rnd, n) for _ in range(rnd.choice([1, 1, 2]))])
    genomes.append(list(genomes[3]))           # a genome given twice: all its windows are duplicates
    genomes.append(["ACGT" * 60])              # internal repeats
    genomes.append(["N" * (L + 5)])            # nothing but N
    genomes.append(["A" * L])                  # exactly one window
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, L, stride)
    want_all = []
    for gen in genomes:
        want_all += candidate_probes.candidate_strings_from_sequences(list(gen), L, stride)
    want = list(dict.fromkeys(want_all))
    assert c.ncandidates == len(want_all) and c.n == len(want)
    pos = c.positions()
    flat = "".join(s for gen in genomes for s in gen)
    assert [flat[p:p + L] for p in pos.tolist()] == want
    sub = np.array([0, c.n - 1, c.n // 2], dtype=np.int64)
    assert c.positions(sub).tolist() == pos[sub].tolist()
    c.close()
    # --small-seq-skip
    skip = 300
    c2 = engine.Candidates(ctx, t, L, stride, seq_length_to_skip=skip)
    want2 = []
    for gen in genomes:
        if any(len(s) > skip for s in gen):
            want2 += candidate_probes.candidate_strings_from_sequences(list(gen), L, stride,
                                                                        seq_length_to_skip=skip)
    assert c2.n == len(dict.fromkeys(want2)) and c2.ncandidates == len(want2)
    c2.close()
    t.close()
    t3 = engine.Targets(ctx, [["ACGT" * 50], ["ACG"]])
    with pytest.raises(ValueError):
        engine.Candidates(ctx, t3, L, stride)
    t3.close()


@pytest.mark.parametrize("m,thres", [(2, 100), (5, 100), (3, 80)])
def test_probes_from_device_candidates_scan_like_string_probes(ctx, m, thres):
    """A probes object gathered from the device's candidates behaves exactly
    like one built from the candidate strings (pigeonhole and given anchors)."""
    engine, probe = _engine(), _probe_mod()
    genomes = small_species(seed=21, n=5, length=2400, d1=0.04, d2=0.01)
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, 100, 50)
    strs = candidates(genomes, 100, 50)
    assert c.n == len(strs)
    np.random.seed(2)
    k, uniq, owner, ep, eo = probe.anchor_table(strs, m, thres, assume_unique=True)
    p_str = engine.Probes(ctx, uniq, owner, ep, eo, k)
    if m == 2:
        p_dev = c.probes(k)                    # pigeonhole table generated on the device
    else:
        p_dev = c.probes(k, ep, eo)
    outs = []
    for p in (p_str, p_dev):
        rows = engine.Rows.scan(ctx, p, t, m, thres, 0, 30)
        outs.append(rows_as_tuples(*rows.fetch()))
        rows.close()
    assert outs[0] == outs[1] and len(outs[0]) > 100
    ids0, _ = engine.setcover_filter(ctx, p_str, t, m, thres, 0, 30, len(strs))
    ids1, _ = engine.setcover_filter(ctx, p_dev, t, m, thres, 0, 30, len(strs))
    assert list(ids0) == list(ids1)
    if m != 2:
        # random anchors handed over as their np.random draws (the device sorts and de-duplicates them): the same
        # draws, the same table
        np.random.seed(2)
        k2, draws = probe.anchor_draws_equal_length(c.n, 100, m, thres)
        assert k2 == k and draws.dtype == np.uint8 and draws.shape == (c.n, 20)
        p_drw = c.probes_from_draws(k2, draws)
        rows = engine.Rows.scan(ctx, p_drw, t, m, thres, 0, 30)
        assert rows_as_tuples(*rows.fetch()) == outs[0]
        rows.close()
        ids2, _ = engine.setcover_filter(ctx, p_drw, t, m, thres, 0, 30, len(strs))
        assert list(ids2) == list(ids0)
        p_drw.close()
        with pytest.raises(ValueError):           # a position beyond the last k-mer of the probe
            c.probes_from_draws(k2, np.full((c.n, 20), 100 - k2 + 1, np.uint8))
    p_str.close(); p_dev.close(); c.close(); t.close()


@pytest.mark.parametrize("kind", ["hamming", "minhash"])
def test_device_candidates_near_duplicate_filter_matches_string_path(ctx, oracle, kind):
    """catchhip_candidates_ndf_* (multiplicities from the device's
    de-duplication, priority order, filter on device-resident rows) == the
    filter on the candidate strings == the oracle, kept candidates in the same
    order; genomes repeated so that multiplicities differ."""
    from catch_amd.filter import near_duplicate_filter as ndf
    engine = _engine()
    base = small_species(seed=31, n=6, length=2000, d1=0.04, d2=0.01)
    genomes = base + [base[1], base[1], base[4]] + small_species(seed=32, n=2, length=900, d1=0.0, d2=0.02)
    L, stride = 100, 25
    strs = candidates(genomes, L, stride, dedup=False)
    f = (ndf.NearDuplicateFilterWithHammingDistance(2, L) if kind == "hamming"
         else ndf.NearDuplicateFilterWithMinHash(0.5))
    random.seed(11)
    want = f._filter_strs(strs)
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, L, stride)
    random.seed(11)
    f._apply_to_candidates(c)
    pos = c.positions()
    flat = "".join(s for g in genomes for s in g)
    got = [flat[p:p + L] for p in pos.tolist()]
    assert got == want and 0 < len(want) < len(set(strs))
    random.seed(11)
    if kind == "hamming":
        positions = oracle.lsh_draw_positions(oracle.lsh_num_tables(2, L, 20), 20, L)
        assert want == oracle.ndf_hamming(strs, 2, positions)
    else:
        params = oracle.minhash_draw_params(oracle.minhash_num_tables(0.5), 3)
        assert want == oracle.ndf_minhash(strs, 0.5, params)
    with pytest.raises(ValueError):
        c.ndf_hamming([[0] * 20], 2)       # a second filter on the same candidates
    c.close(); t.close()


@pytest.mark.parametrize("first_kind", ["dup", "minhash", "hamming"])
def test_union_device_front_end_equals_string_path(ctx, monkeypatch, first_kind):
    """Many small groups with the front end on the device (grouped targets:
    duplicates removed per group, MinHash filter over all groups in one pass,
    union solve) == the string path.  The groups are strains of the same species
    and one genome sits in two groups, so identical windows occur in different
    groups and must stay separate candidates."""
    from catch_amd.filter import duplicate_filter, near_duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.genome import Genome
    sp = (small_species(seed=41, n=12, length=2100, d1=0.03, d2=0.01) +
          small_species(seed=42, n=8, length=1500, d1=0.05, d2=0.01, with_n=False))
    groups = [sp[i:i + 2] for i in range(0, len(sp), 2)]
    groups[3] = groups[3] + [groups[0][0]]          # the same genome in two groups
    genomes = [[Genome.from_one_seq(x[0]) for x in g] for g in groups]
    results = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        first = (duplicate_filter.DuplicateFilter() if first_kind == "dup"
                 else near_duplicate_filter.NearDuplicateFilterWithMinHash(0.5) if first_kind == "minhash"
                 else near_duplicate_filter.NearDuplicateFilterWithHammingDistance(2, 100))
        scf = set_cover_filter.SetCoverFilter(mismatches=3, lcf_thres=100, coverage=1.0, cover_extension=20)
        pd = probe_designer.ProbeDesigner(genomes, [first, scf], probe_length=100, probe_stride=50)
        if not host:
            assert pd._device_front_end_mode(genomes, first, scf) == "union"
        random.seed(5)
        np.random.seed(6)
        grouped = pd._design_on_strings(genomes, [first, scf])
        results.append([[p.seq_str for p in g] for g in grouped])
    assert results[0] == results[1]
    assert sum(map(len, results[0])) > 40 and all(len(g) > 0 for g in results[0])


def test_rows_stats_match_fetched_rows(ctx):
    """catchhip_rows_stats (coverage report without fetching the rows): summed
    range lengths, bases covered (union) per universe and universes per set ==
    the same numbers from the fetched table."""
    engine, probe = _engine(), _probe_mod()
    genomes = small_species(seed=61, n=7, length=1800, d1=0.04, d2=0.01)
    genomes.append(["ACGT" * 100, "T" * 150])          # two sequences: one universe each below
    seqs = [[s] for g in genomes for s in g]
    strs = candidates(genomes[:4], 100, 25)[::3]
    np.random.seed(3)
    k, uniq, owner, ep, eo = probe.anchor_table(strs, 3, 100, min_k=10, k=10)
    t = engine.Targets(ctx, seqs)
    p = engine.Probes(ctx, uniq, owner, ep, eo, k)
    for merge in (False, True):
        rows = engine.Rows.scan(ctx, p, t, 3, 100, 0, 15, engine.SCAN_AUTO, merge)
        sid, univ, st, en = rows.fetch()
        total, union, per_set = rows.stats(len(seqs), len(strs))
        rows.close()
        want_total = np.bincount(univ, weights=(en - st).astype(np.float64), minlength=len(seqs)).astype(np.int64)
        want_union = np.zeros(len(seqs), dtype=np.int64)
        for u in range(len(seqs)):
            cov = np.zeros(len(seqs[u][0]) + 1, dtype=np.int64)
            for a, b in zip(st[univ == u].tolist(), en[univ == u].tolist()):
                cov[a] += 1; cov[b] -= 1
            want_union[u] = int((np.cumsum(cov)[:-1] > 0).sum())
        pairs = np.unique(sid.astype(np.int64) * len(seqs) + univ)
        want_sets = np.bincount(pairs // len(seqs), minlength=len(strs))
        assert total.tolist() == want_total.tolist()
        assert union.tolist() == want_union.tolist()
        assert per_set.tolist() == want_sets.tolist() and per_set.sum() > 10
    p.close(); t.close()


@pytest.mark.gpu
def test_neighbour_graph_edge_cases(ctx):
    """catchhip_sigs_graph on one sequence, on unrelated sequences (no edges), on identical ones (a clique) and
    with a sequence count that is not a multiple of any tile; the clustering on top of each."""
    from catch_amd.utils import cluster, lsh
    rng = np.random.RandomState(11)

    def rand(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, size=n))
    base = rand(3000)
    cases = {"one": [rand(2000)],
             "unrelated": [rand(2000) for _ in range(70)],
             "clique": [base] * 67,
             "mixed": [base[:2500] + rand(40) for _ in range(33)] + [rand(1500) for _ in range(100)]}
    for name, seqs in cases.items():
        random.seed(9)
        sigs = lsh.MinHashFamily(12, N=100).signatures(seqs)
        try:
            ptr, gidx, gcom = sigs.graph(9)
            n = len(seqs)
            assert ptr.shape == (n + 1,) and ptr[0] == 0 and ptr[-1] == gidx.size == gcom.size
            for j in range(n):
                row = sigs.common_row(j).astype(np.int64)
                want = np.nonzero(row >= 9)[0]
                want = want[want != j]
                assert np.array_equal(gidx[ptr[j]:ptr[j + 1]], want), (name, j)
                assert np.array_equal(gcom[ptr[j]:ptr[j + 1]], row[want]), (name, j)
            if name in ("one", "unrelated"):
                assert gidx.size == 0
            if name == "clique":
                assert gidx.size == n * (n - 1) and set(gcom.tolist()) == {100}
        finally:
            sigs.close()
        random.seed(9)
        got = cluster.cluster_with_minhash_signatures(dict(enumerate(seqs)), threshold=0.15, cluster_method="simple")
        assert sorted(x for c in got for x in c) == list(range(len(seqs)))
        if name == "clique":
            assert len(got) == 1
        if name == "unrelated":
            assert len(got) == len(seqs)


@pytest.mark.gpu
def test_neighbour_lists_and_graph_of_a_large_clique(ctx, monkeypatch):
    """4,200 identical sequences and 30 unrelated ones behind them.  Every clique vertex has 4,200 entries in its
    neighbour list (itself included): more than the 4,096 that catchhip_sigs_neighbors copies back with the count,
    so the second copy runs; 32 lists in one call are 134,400 entries, more than the 16,384 of
    catchhip_sigs_neighbors_many's first copy (and more than the wrapper's first buffer: it grows and asks again);
    the graph has 4,200 x 4,199 = 17,635,800 ordered pairs, more than the 2^24 slots of catchhip_sigs_graph's first
    pass, so it counts, allocates n + 2 and runs again.  Every row is checked, not a sample."""
    from catch_amd import engine
    from catch_amd.utils import lsh
    rng = np.random.RandomState(4200)

    def rand(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, size=n))
    nc, nu = 4200, 30
    seqs = [rand(400)] * nc + [rand(400) for _ in range(nu)]
    n = nc + nu
    edges = nc * (nc - 1)
    assert edges > 1 << 24 and edges > 1024 * n and nc > 4096 and 32 * nc > 16384
    random.seed(9)
    sigs = lsh.MinHashFamily(12, N=100).signatures(seqs)
    try:
        ptr, gidx, gcom = sigs.graph(9)
        assert ptr.shape == (n + 1,) and gidx.size == gcom.size == edges
        assert np.array_equal(ptr, np.minimum(np.arange(n + 1), nc) * (nc - 1))        # the unrelated rows are empty
        others = np.arange(nc - 1, dtype=np.uint32)[None, :]
        want = others + (others >= np.arange(nc, dtype=np.uint32)[:, None])            # row j: 0 .. nc - 1 without j
        assert np.array_equal(gidx.reshape(nc, nc - 1), want)
        assert (gcom == 100).all()
        del want
        ends = (1, nc // 2, nc - 2)
        single = {}
        for j in ends:
            row = sigs.common_row(j).astype(np.int64)
            assert (row[:nc] == 100).all() and (row[nc:] < 9).all()
            idx, com = sigs.neighbors(j, 9)
            assert idx.size == nc > 4096 and np.array_equal(idx, np.arange(nc)) and (com == 100).all()
            single[j] = (idx, com)
        for j in (nc, n - 1):                                    # an unrelated vertex: itself
            idx, com = sigs.neighbors(j, 9)
            assert idx.tolist() == [j] and com.tolist() == [100]
        js = np.asarray(list(ends) + [5, nc - 1, 0] + list(range(100, 100 + 26 * 150, 150)))
        assert js.size == 32 == engine.Signatures.NEIGHBORS_MANY_MAX and js.max() < nc
        many = sigs.neighbors_many(js, 9)
        assert sum(idx.size for idx, _ in many) == 32 * nc > 16384
        for j, (idx, com) in zip(js.tolist(), many):
            assert np.array_equal(idx, np.arange(nc)) and (com == 100).all(), j
            if j in single:
                assert np.array_equal(idx, single[j][0]) and np.array_equal(com, single[j][1])
        mixed = sigs.neighbors_many([nc + 3, 7], 9)              # a short list in front of a long one
        assert mixed[0][0].tolist() == [nc + 3] and np.array_equal(mixed[1][0], np.arange(nc))
        print("clique of %d + %d unrelated: %d ordered pairs > 2^24 = %d (second graph pass); neighbour lists of %d "
              "entries > 4096; %d entries from one call for 32 vertices > 16384"
              % (nc, nu, gidx.size, 1 << 24, nc, 32 * nc))
        # more pairs than the caller lets the graph hold: no graph, below and above the first pass's room
        for limit in (1 << 20, edges - 1):
            monkeypatch.setattr(engine.Signatures, "GRAPH_MAX_EDGES", limit)
            assert sigs.graph(9) is None
        monkeypatch.setattr(engine.Signatures, "GRAPH_MAX_EDGES", edges)
        ptr2, gidx2, gcom2 = sigs.graph(9)
        assert np.array_equal(ptr2, ptr) and np.array_equal(gidx2, gidx) and np.array_equal(gcom2, gcom)
    finally:
        sigs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["hamming", "minhash"])
def test_union_chunks_in_pipeline_stages_select_what_chunks_one_by_one_select(ctx, monkeypatch, first):
    """The clustered design's union instances (several clusters per chunk, several chunks): the three-stage
    pipeline -- front end with the near-duplicate filter on one, two or three worker streams (its draws from
    `random` made for all chunks ahead), the anchors' np.random draws on a thread of their own, scan + solve on the
    caller's -- returns what the chunks one after the other on one stream return (-m 5: random anchors)."""
    from catch_amd import genome
    from catch_amd.filter import near_duplicate_filter, set_cover_filter
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(4321))
    clusters = [[genome.Genome.from_one_seq(g[0]) for g in synthetic.make_species(rng, [int(ln)], n, 2, 0.04, 0.01)]
                for ln, n in ((4000, 5), (2500, 3), (2600, 4), (6000, 3), (2400, 2), (3000, 3), (2800, 5), (2200, 6), (5000, 2))]

    def run(depth, workers):
        monkeypatch.setenv("CATCHHIP_PREFETCH_DEPTH", str(depth))
        monkeypatch.setenv("CATCHHIP_FRONT_END_WORKERS", str(workers))
        random.seed(15)
        np.random.seed(16)
        ndf = (near_duplicate_filter.NearDuplicateFilterWithHammingDistance(2, 100) if first == "hamming"
               else near_duplicate_filter.NearDuplicateFilterWithMinHash(0.5))
        scf = set_cover_filter.SetCoverFilter(mismatches=5, lcf_thres=100, cover_extension=25, kmer_probe_map_k=20)
        out = scf._filter_genomes_device_union(clusters, 100, 50, None, ndf, max_bases=40_000)
        return out, scf.last_timings["picks"]

    base, picks = run(0, 1)
    assert all(len(g) > 0 for g in base) and picks == sum(len(g) for g in base)
    for depth, workers in ((1, 1), (2, 1), (2, 2), (2, 3)):
        got, p2 = run(depth, workers)
        assert got == base and p2 == picks, (depth, workers)
