"""Extending an existing probe set: catchhip_rows_subtract, SetCoverFilter(fixed_probes=...) and
`design --extend-probes`.

The fixed probes count as sets picked before the first round of the reference's greedy loop
(catch/utils/set_cover.py:362-550).  _plain_extend_greedy below restates that over Python sets; the product
builds a reduced instance instead (rows minus the fixed coverage, adjusted coverage fractions) and runs the
unchanged solvers on it."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EBOLA = os.path.join(GOLDEN, "ebola_zaire_100.fasta.gz")


# ------------------------------------------------------------------ host models
def _normalise(ranges):
    out = []
    for s, t in sorted(ranges):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], t)
        else:
            out.append([s, t])
    return [tuple(x) for x in out]


def _np_subtract(rows, covered, glen):
    """NumPy interval subtraction.  rows / covered = (set, universe, start, end) arrays, coordinates inside the
    universe; glen = universe lengths.  Every row cut into its maximal runs that no covered row touches, in row
    order: the global runs of free bases that meet the row, clipped to it."""
    si, un, st, en = (np.asarray(a, dtype=np.int64) for a in rows)
    _cs, cu, cst, cen = (np.asarray(a, dtype=np.int64) for a in covered)
    off = np.concatenate([[0], np.cumsum(np.asarray(glen, dtype=np.int64))])
    total = int(off[-1])
    d = np.zeros(total + 1, dtype=np.int64)
    np.add.at(d, off[cu] + cst, 1)
    np.add.at(d, off[cu] + cen, -1)
    free = np.cumsum(d[:total]) == 0
    edge = np.diff(np.concatenate([[0], free.astype(np.int8), [0]]))
    run_s, run_e = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    gs, ge = off[un] + st, off[un] + en
    k0 = np.searchsorted(run_e, gs, side="right")
    k1 = np.searchsorted(run_s, ge, side="left")
    cnt = np.maximum(k1 - k0, 0)
    row = np.repeat(np.arange(si.size), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(k0, cnt)
    ps, pe = np.maximum(run_s[k], gs[row]), np.minimum(run_e[k], ge[row])
    return (si[row].astype(np.int32), un[row].astype(np.int32), ps - off[un[row]], pe - off[un[row]])


def _union_len(table, nuniv):
    """Bases of every universe covered by at least one row."""
    out = np.zeros(nuniv, dtype=np.int64)
    _s, un, st, en = table
    for u in range(nuniv):
        m = np.asarray(un) == u
        out[u] = sum(t - s for s, t in _normalise(zip(np.asarray(st)[m].tolist(), np.asarray(en)[m].tolist())))
    return out


def _plain_extend_greedy(sets, fixed, p, ranks):
    """catch/utils/set_cover.py:362-550 with the fixed probes' elements removed before the first pick.
    sets[i] = {universe: set of ints}, fixed = {universe: set of ints}, p[u], ranks[i].  Unit costs; among equal
    ratios the lowest id (the order in which the reference meets small-int set ids).  None: ranks exhausted."""
    nuniv = len(p)
    universes = {u: set(fixed.get(u, ())) for u in range(nuniv)}
    for by_u in sets:
        for u, s in by_u.items():
            universes[u] |= s
    can = {u: int(len(universes[u]) - p[u] * len(universes[u])) for u in universes}
    for u in universes:
        universes[u] -= fixed.get(u, set())
    left = {u: max(0, len(universes[u]) - can[u]) for u in universes}
    rank_vals = sorted(set(ranks))
    at, picks, remaining = 0, [], set(range(len(sets)))
    while any(v > 0 for v in left.values()):
        best, best_gain = None, 0
        for i in sorted(remaining):
            if ranks[i] != rank_vals[at]:
                continue
            gain = sum(min(left[u], len(s & universes[u])) for u, s in sets[i].items())
            if gain > best_gain:
                best, best_gain = i, gain
        if best is None:
            at += 1
            if at == len(rank_vals):
                return None
            continue
        picks.append(best)
        remaining.discard(best)
        for u, s in sets[best].items():
            universes[u] -= s
            left[u] = max(0, len(universes[u]) - can[u])
    return picks


def _random_ranges(rng, length, most):
    out = []
    for _ in range(int(rng.integers(0, most + 1))):
        a = int(rng.integers(0, length))
        out.append((a, int(rng.integers(a + 1, min(length, a + 40) + 1))))
    return _normalise(out)


def _instance(rng, max_sets=14, max_len=120):
    """(glen, rows table of the candidates, rows table of the fixed probes, the same two as Python sets)."""
    nuniv = int(rng.integers(1, 5))
    nsets = int(rng.integers(1, max_sets + 1))
    glen = [int(rng.integers(1, max_len + 1)) for _ in range(nuniv)]
    rows, sets = [], []
    for i in range(nsets):
        by_u = {}
        for u in range(nuniv):
            if rng.random() < 0.7:
                rr = _random_ranges(rng, glen[u], 4)
                if rr:
                    by_u[u] = set(x for s, t in rr for x in range(s, t))
                    rows += [(i, u, s, t) for s, t in rr]
        sets.append(by_u)
    cov, fixed = [], {}
    for j in range(int(rng.integers(0, 4))):
        for u in range(nuniv):
            if rng.random() < 0.6:
                rr = _random_ranges(rng, glen[u], 3)
                cov += [(j, u, s, t) for s, t in rr]
                fixed.setdefault(u, set()).update(x for s, t in rr for x in range(s, t))
    return glen, nsets, _table(rows), _table(cov), sets, fixed


def _table(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].copy(), a[:, 3].copy()


def _fractions(reduced, cov, glen, p):
    from catch_amd.filter.set_cover_filter import extension_fraction
    n2, c0 = _union_len(reduced, len(glen)), _union_len(cov, len(glen))
    return [extension_fraction(int(a), int(b), q) for a, b, q in zip(n2, c0, p)]


# ------------------------------------------------------------------ without a GPU
def test_extension_fraction_reproduces_the_number_that_may_stay_uncovered():
    """int(n2 - p' n2) == min(can, n2) with can = int(|U| - p |U|), |U| = n2 + |C0|; 0 <= p' <= 1; p' == 1.0
    exactly when can == 0 -- at random and at the edges (can = 0, can >= n2, n2 = 1, n2 = 2^32 - 2)."""
    from catch_amd.filter.set_cover_filter import extension_fraction
    rng = np.random.default_rng(11)
    top = (1 << 32) - 2
    cases = []
    for n2 in (0, 1, 2, 3, 100, 101, top - 1, top):
        for c0 in (0, 1, 7, 1000, 1 << 31):
            for p in (1.0, 0.9, 0.5, 0.0, 0.37, 1e-9, 1.0 - 1e-12):
                cases.append((n2, c0, p))
    for _ in range(20000):
        n2 = int(rng.integers(0, top + 1)) if rng.random() < 0.5 else int(rng.integers(0, 3000))
        c0 = int(rng.integers(0, top + 1)) if rng.random() < 0.5 else int(rng.integers(0, 3000))
        p = float(rng.choice([1.0, 0.9, 0.5, 0.37, 0.0])) if rng.random() < 0.5 else float(rng.random())
        cases.append((n2, c0, p))
    seen = set()
    for n2, c0, p in cases:
        n = n2 + c0
        can = int(n - p * n)
        q = extension_fraction(n2, c0, p)
        assert 0.0 <= q <= 1.0, (n2, c0, p)
        assert int(n2 - q * n2) == min(can, n2), (n2, c0, p, q)
        assert (q == 1.0) == (can == 0), (n2, c0, p, q)
        seen.add("zero" if can == 0 else "all" if can >= n2 else "some")
    assert seen == {"zero", "all", "some"}


def test_reduced_instance_picks_what_the_greedy_with_fixed_sets_picks(oracle):
    """The plain greedy with the fixed coverage removed first == the oracle's approx_multiuniverse on the
    NumPy-subtracted rows with the adjusted fractions, pick for pick."""
    rng = np.random.default_rng(2024)
    compared = partial = exhausted = 0
    for _ in range(400):
        glen, nsets, rows, cov, sets, fixed = _instance(rng)
        p = [float(rng.choice([1.0, 0.9, 0.5, 0.37, 0.0]))] * len(glen) if rng.random() < 0.5 else \
            [float(rng.choice([1.0, 0.9, 0.5, 0.37, 0.0])) for _ in glen]
        ranks = [int(rng.choice([0, 3])) for _ in range(nsets)] if rng.random() < 0.5 else [0] * nsets
        want = _plain_extend_greedy(sets, fixed, p, ranks)
        reduced = _np_subtract(rows, cov, glen)
        # (the subtraction itself, against the sets)
        got_sets = {}
        for i, u, s, t in zip(*reduced):
            got_sets.setdefault((int(i), int(u)), set()).update(range(int(s), int(t)))
        for i, by_u in enumerate(sets):
            for u, s in by_u.items():
                assert got_sets.get((i, u), set()) == s - fixed.get(u, set())
        q = _fractions(reduced, cov, glen, p)
        if want is None:
            exhausted += 1
            with pytest.raises(IndexError):
                oracle.approx_multiuniverse(*reduced, nsets, len(glen), universe_p=q, ranks=ranks)
            continue
        got = oracle.approx_multiuniverse(*reduced, nsets, len(glen), universe_p=q, ranks=ranks)
        assert got == want, (glen, p, ranks)
        compared += 1
        partial += any(x < 1.0 for x in p)
    assert compared >= 300 and partial >= 150


def test_symbol_is_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_subtract\s*\(", hdr)
    assert "catchhip_rows_subtract" in _lib.PROTOTYPES
    assert callable(engine.Rows.subtract)
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "subtract.hip" in mk


def test_filter_keeps_the_reference_signature_and_takes_fixed_probes():
    import inspect
    from catch_amd import probe
    from catch_amd.filter import set_cover_filter as scf
    names = list(inspect.signature(scf.SetCoverFilter.__init__).parameters)
    assert names[-1] == "fixed_probes" and names[-2] == "kmer_probe_map_use_native_dict"
    assert scf.SetCoverFilter(2, 100).fixed_probes == []
    assert scf.SetCoverFilter(2, 100, fixed_probes=[]).fixed_probes == []
    f = scf.SetCoverFilter(2, 100, fixed_probes=["ACGT", probe.Probe.from_str("GGCC")])
    assert f.fixed_probes == ["ACGT", "GGCC"]


def test_front_end_stays_on_the_host_with_fixed_probes():
    from catch_amd.filter import probe_designer, set_cover_filter as scf
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for fixed, want in ((None, "per group"), (["ACGT" * 25], None)):
        f = scf.SetCoverFilter(2, 100, fixed_probes=fixed)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == want


def test_command_line_refusals(tmp_path):
    from catch_amd import design
    fa = tmp_path / "t.fasta"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    probes = tmp_path / "p.fasta"
    probes.write_text(">p\n" + "ACGT" * 25 + "\n")
    empty = tmp_path / "empty.fasta"
    empty.write_text("")
    base = [str(fa), "-o", str(tmp_path / "o.fasta")]
    with pytest.raises(Exception, match="--skip-set-cover"):
        design.main(design.parse_args(base + ["--extend-probes", str(probes), "--skip-set-cover"]))
    with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):
        design.main(design.parse_args(base + ["--extend-probes", str(probes),
                                              "--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):     # design_large's default
        design.main(design.parse_args(base + ["--extend-probes", str(probes)], args_type="large"))
    with pytest.raises(Exception, match="--cluster-from-fragments to 0"):     # design_large with clustering alone off
        design.main(design.parse_args(base + ["--extend-probes", str(probes), "--cluster-and-design-separately", "0"],
                                      args_type="large"))
    with pytest.raises(Exception, match="holds no sequence"):
        design.main(design.parse_args(base + ["--extend-probes", str(empty)]))
    # what the message advises parses
    args = design.parse_args(base + ["--extend-probes", str(probes), "--cluster-and-design-separately", "0",
                                     "--cluster-from-fragments", "0"], args_type="large")
    assert not args.cluster_and_design_separately and not args.cluster_from_fragments
    assert not os.path.exists(str(tmp_path / "o.fasta"))


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel
    from catch_amd.filter import set_cover_filter as scf

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    f = scf.SetCoverFilter(2, 100, fixed_probes=["ACGT" * 25])
    with pytest.raises(NotImplementedError):
        f._filter_strs([["ACGT" * 25]], [[]])


# ------------------------------------------------------------------ kernel: rows minus covered
def _from_host(ctx, table, glen):
    from catch_amd import engine
    return engine.Rows.from_host(ctx, table[0], table[1], table[2], table[3], glen)


def _check_subtract(ctx, rows, cov, glen, tag):
    R, C = _from_host(ctx, rows, glen), _from_host(ctx, cov, glen)
    try:
        D = R.subtract(C)
        try:
            want = _np_subtract(rows, cov, glen)
            got = D.fetch()
            assert D.n == want[0].size, tag
            for g, w, name in zip(got, want, ("set", "universe", "start", "end")):
                assert np.array_equal(g, w), (tag, name)
            return got
        finally:
            D.close()
    finally:
        R.close()
        C.close()


def _hand_made_cases():
    """name -> (universe lengths, rows (set, universe, start, end), covered (universe, start, end): a set each)."""
    alt = [(0, s, s + 1) for s in range(11, 11 + 257, 2)]          # every other base of [10, 267) stays
    rng = np.random.default_rng(3)
    holes = sorted(set(int(x) for x in rng.integers(100, 5100, size=400)))
    return {
        "holes at a row's first and last base": ([300], [(0, 0, 10, 50)], [(0, 10, 11), (0, 49, 50)]),
        "a row fully covered vanishes": ([300], [(0, 0, 10, 50), (0, 0, 60, 70), (1, 0, 5, 8)],
                                         [(0, 10, 50), (0, 0, 5)]),
        "a row untouched": ([300], [(0, 0, 10, 50)], [(0, 100, 200)]),
        "cover ending at a row's start, cover touching its end": (
            [300], [(0, 0, 10, 50), (1, 0, 60, 70)], [(0, 0, 10), (0, 50, 55), (0, 70, 80), (0, 58, 60)]),
        "rows and holes across word boundaries": (
            [1000], [(0, 0, 60, 70), (0, 0, 100, 400), (1, 0, 63, 65), (2, 0, 0, 64), (2, 0, 128, 192),
                     (3, 0, 64, 129), (4, 0, 64, 128), (5, 0, 1, 1000)],
            [(0, 62, 66), (0, 127, 129), (0, 191, 257), (0, 319, 320), (0, 384, 385), (0, 640, 704)]),
        "257 bases under alternating cover: 129 pieces": ([400], [(0, 0, 10, 267)], alt),
        "5,000 bases with a few hundred holes": ([6000], [(0, 0, 100, 5100), (1, 0, 0, 6000)],
                                                 [(0, h, h + 1) for h in holes]),
        "cover to the end of a universe, a row from the start of the next": (
            [100, 100, 28], [(0, 0, 90, 100), (0, 1, 0, 10), (0, 1, 90, 100), (0, 2, 0, 28)],
            [(0, 95, 100), (1, 99, 100), (1, 5, 6)]),
        "the last word, total a multiple of 64": ([64, 128], [(0, 1, 100, 128), (1, 1, 64, 128)],
                                                  [(1, 120, 127), (1, 64, 65)]),
        "the last word, total no multiple of 64": ([64, 100], [(0, 1, 60, 100), (1, 1, 99, 100)],
                                                   [(1, 98, 99), (1, 63, 65)]),
        "the last base covered": ([64, 64], [(0, 1, 0, 64)], [(1, 63, 64)]),
        "empty covered": ([300], [(0, 0, 10, 50), (3, 0, 20, 30)], []),
        "empty rows": ([300], [], [(0, 10, 50)]),
        "both empty": ([300], [], []),
        "overlapping cover from several sets": (
            [300, 50], [(0, 0, 0, 300), (2, 1, 0, 50)],
            [(0, 10, 100), (0, 50, 150), (0, 200, 210), (0, 90, 205), (1, 10, 20), (1, 10, 20)]),
    }


@pytest.mark.gpu
def test_rows_subtract_hand_made_cases(ctx):
    cases = _hand_made_cases()
    for tag, (glen, rows, cov) in cases.items():
        got = _check_subtract(ctx, _table(rows), _table([(j,) + c for j, c in enumerate(cov)]), glen, tag)
        if tag.startswith("257 bases"):
            assert got[0].size == 129 and (got[3] - got[2] == 1).all()
        if tag == "a row fully covered vanishes":
            assert [tuple(int(x[i]) for x in got) for i in range(got[0].size)] == [(0, 0, 60, 70), (1, 0, 5, 8)]
        if tag == "empty covered":
            assert got[0].size == 2


def _big_table(rng, nsets, nuniv, per, gap_hi, len_hi, glen=None):
    g = rng.integers(1, gap_hi, size=(nsets, nuniv, per))
    ln = rng.integers(1, len_hi, size=(nsets, nuniv, per))
    en = np.cumsum(g + ln, axis=2)
    st = en - ln
    si = np.broadcast_to(np.arange(nsets)[:, None, None], st.shape)
    un = np.broadcast_to(np.arange(nuniv)[None, :, None], st.shape)
    if glen is None:
        glen = en.max(axis=(0, 2))
    keep = en <= np.asarray(glen)[None, :, None]
    return (si[keep].astype(np.int32), un[keep].astype(np.int32), st[keep], en[keep]), [int(x) for x in glen]


@pytest.mark.gpu
def test_rows_subtract_random_tables(ctx):
    rng = np.random.default_rng(77)
    pieces = 0
    for case in range(200):
        glen, _n, rows, cov, _sets, _fixed = _instance(rng, max_sets=20, max_len=300)
        pieces += _check_subtract(ctx, rows, cov, glen, case)[0].size
    assert pieces > 1000
    # ~300,000 rows, some longer than five words: the exclusive scan crosses its tile edges
    rows, glen = _big_table(rng, 600, 5, 100, 40, 400)
    cov, _ = _big_table(rng, 7, 5, 300, 120, 30, glen)
    assert 250_000 < rows[0].size < 350_000 and (rows[3] - rows[2]).max() > 320
    got = _check_subtract(ctx, rows, cov, glen, "large")
    assert got[0].size > rows[0].size


@pytest.mark.gpu
def test_rows_subtract_refuses_another_coordinate_space(ctx):
    from catch_amd import engine, probe
    rows = _table([(0, 0, 10, 50), (0, 1, 0, 5)])
    R = _from_host(ctx, rows, [100, 50])
    held = [R]
    try:
        for glen in ([100, 51], [150], [100, 50, 1], [50, 100]):
            C = _from_host(ctx, _table([(0, 0, 1, 2)]), glen)
            held.append(C)
            with pytest.raises(ValueError, match="coordinate space"):
                R.subtract(C)
        # unmerged ranges of a scan over other targets
        rng = np.random.default_rng(8)
        genome = "".join(rng.choice(list("ACGT"), size=400))
        strs = [genome[j:j + 60] for j in range(0, 340, 20)]
        k, uniq, owner, ep, eo = probe.anchor_table(strs, 1, 60, min_k=20, k=20)
        targets = engine.Targets(ctx, [[genome], [genome[50:300]]])
        held.append(targets)
        probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
        held.append(probes)
        ranges = engine.Rows.scan(ctx, probes, targets, 1, 60, 0, 0, merge=False)
        held.append(ranges)
        assert ranges.n > 0
        with pytest.raises(ValueError, match="coordinate space"):
            R.subtract(ranges)
        # rows of a scan with group numbers (a union of instances)
        gp, gt = engine.Probes(ctx, uniq, owner, ep, eo, k), engine.Targets(ctx, [[genome], [genome[50:300]]])
        held += [gp, gt]
        gp.set_groups(np.zeros(len(uniq), dtype=np.int32))
        gt.set_groups(np.zeros(2, dtype=np.int32))
        grouped = engine.Rows.scan(ctx, gp, gt, 1, 60, 0, 0)
        held.append(grouped)
        plain = engine.Rows.scan(ctx, probes, targets, 1, 60, 0, 0)
        held.append(plain)
        with pytest.raises(ValueError, match="group numbers"):
            grouped.subtract(plain)
        with pytest.raises(ValueError, match="group numbers"):
            plain.subtract(grouped)
        # ... and over the same universes they are a covered table like any other (overlapping, many set ids)
        glen = [400, 250]
        mine = _table([(0, 0, 0, 400), (1, 0, 7, 333), (1, 1, 0, 250)])
        R2 = _from_host(ctx, mine, glen)
        held.append(R2)
        D = R2.subtract(ranges)
        held.append(D)
        want = _np_subtract(mine, ranges.fetch(), glen)
        for g, w in zip(D.fetch(), want):
            assert np.array_equal(g, w)
    finally:
        for h in reversed(held):
            h.close()


# ------------------------------------------------------------------ rows level, end to end
@pytest.mark.gpu
def test_subtract_stats_fractions_greedy_equal_the_plain_greedy(ctx):
    from catch_amd.filter.set_cover_filter import extension_fraction
    rng = np.random.default_rng(909)
    compared = 0
    for case in range(60):
        glen, nsets, rows, cov, sets, fixed = _instance(rng)
        R, C = _from_host(ctx, rows, glen), _from_host(ctx, cov, glen)
        D = R.subtract(C)
        try:
            n2, c0 = D.stats(len(glen))[1], C.stats(len(glen))[1]
            for p in (1.0, 0.9, 0.5):
                for ranks in (None, [int(x) for x in rng.choice([0, 3], size=nsets)]):
                    want = _plain_extend_greedy(sets, fixed, [p] * len(glen), ranks or [0] * nsets)
                    q = [extension_fraction(int(a), int(b), p) for a, b in zip(n2, c0)]
                    up = None if all(x == 1.0 for x in q) else q
                    if want is None:
                        with pytest.raises(IndexError):
                            D.greedy(nsets, ranks, up)
                        continue
                    got = D.greedy(nsets, ranks, up)
                    assert got == want, (case, p, ranks)
                    chk = D.cover_check(nsets, got, up)
                    assert chk["universes_short"] == 0 and chk["picks_without_gain"] == 0 \
                        and chk["bad_pick_ids"] == 0, (case, p, chk)
                    compared += 1
        finally:
            for h in (D, R, C):
                h.close()
    assert compared >= 300


# ------------------------------------------------------------------ filter level
def _genomes(n):
    from catch_amd.utils import seq_io
    return seq_io.read_genomes_from_fasta(EBOLA)[:n]


def _candidates(genomes):
    from catch_amd.filter import candidate_probes
    out = []
    for g in genomes:
        out += candidate_probes.candidate_strings_from_sequences(list(g.seqs), 100, 50)
    return list(dict.fromkeys(out))


def _filter(e, coverage=1.0, **kw):
    from catch_amd.filter import set_cover_filter as scf
    return scf.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=coverage, cover_extension=e, **kw)


_designs = {}


def _design(e, coverage=1.0):
    """(genomes, candidates of the 10 genomes, the design of all 10, the design of the first 5), made once."""
    key = (e, coverage)
    if key not in _designs:
        g10 = _genomes(10)
        c10, c5 = _candidates(g10), _candidates(g10[:5])
        d10 = [c10[i] for i in _filter(e, coverage)._filter_strs([c10], [g10], assume_unique=True)[0]]
        d5 = [c5[i] for i in _filter(e, coverage)._filter_strs([c5], [g10[:5]], assume_unique=True)[0]]
        _designs[key] = (g10, c10, d10, d5)
    return _designs[key]


def _oracle_rows(oracle, strs, genomes, e):
    k, entries = oracle.anchor_table(strs, 2, 100, 20, 20)
    return oracle.make_sets(strs, entries, k, [list(g.seqs) for g in genomes], 2, 100, 0, e)


def _scan(ctx, strs, genomes, e):
    from catch_amd import engine, probe
    k, uniq, _owner, ep, eo = probe.anchor_table(strs, 2, 100, min_k=20, k=20)
    assert uniq == list(strs)
    targets = engine.Targets(ctx, [g.seqs for g in genomes])
    probes = engine.Probes(ctx, uniq, np.arange(len(uniq), dtype=np.int32), ep, eo, k)
    try:
        return engine.Rows.scan(ctx, probes, targets, 2, 100, 0, e).fetch()
    finally:
        probes.close()
        targets.close()


def _check_covers(ctx, fixed, cands, new_ids, genomes, e, coverage):
    """The fixed probes and the new ones, picked from the table of fixed + candidates, leave no universe short."""
    from catch_amd import engine
    glen = [g.size() for g in genomes]
    fr, cr = _scan(ctx, fixed, genomes, e), _scan(ctx, cands, genomes, e)
    both = tuple(np.concatenate([a, b + (len(fixed) if i == 0 else 0)]) for i, (a, b) in enumerate(zip(fr, cr)))
    T = engine.Rows.from_host(ctx, both[0], both[1], both[2], both[3], glen)
    try:
        picks = list(range(len(fixed))) + [len(fixed) + i for i in new_ids]
        chk = T.cover_check(len(fixed) + len(cands), picks, None if coverage == 1.0 else [coverage] * len(glen))
        assert chk["universes_short"] == 0 and chk["bad_pick_ids"] == 0, chk
    finally:
        T.close()


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_filter_without_fixed_probes_is_unchanged_and_a_full_design_needs_nothing(ctx, e):
    g10, c10, d10, d5 = _design(e)
    plain = _filter(e)._filter_strs([c10], [g10], assume_unique=True)
    assert _filter(e, fixed_probes=[])._filter_strs([c10], [g10], assume_unique=True) == plain
    assert [c10[i] for i in plain[0]] == d10 and len(d10) >= len(d5) > 0
    f = _filter(e, fixed_probes=d10)
    assert f._filter_strs([c10], [g10], assume_unique=True) == [[]]
    assert f.last_timings["picks"] == 0 and f.last_timings["rows_reduced"] == 0
    assert f.last_timings["rows_fixed"] > 0 and f.last_timings["subtract_ms"] > 0


def _oracle_extension(oracle, cands, fixed, genomes, e, coverage):
    """(what to select, rows of the reduced instance): the oracle's cover rows of candidates and fixed probes,
    NumPy subtraction, the adjusted fractions, the oracle's greedy."""
    from catch_amd.filter.set_cover_filter import extension_fraction
    glen = [g.size() for g in genomes]
    rows, cov = _oracle_rows(oracle, cands, genomes, e), _oracle_rows(oracle, fixed, genomes, e)
    reduced = _np_subtract(rows, cov, glen)
    n2, c0 = _union_len(reduced, len(glen)), _union_len(cov, len(glen))
    q = [extension_fraction(int(a), int(b), coverage) for a, b in zip(n2, c0)]
    return oracle.approx_multiuniverse(*reduced, len(cands), len(glen), universe_p=q), reduced[0].size


@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_extends_the_design_of_five_genomes_to_ten(ctx, oracle, e, coverage):
    g10, c10, d10, d5 = _design(e, coverage)
    f = _filter(e, coverage, fixed_probes=d5)
    new = f._filter_strs([c10], [g10], assume_unique=True)[0]
    want, nreduced = _oracle_extension(oracle, c10, d5, g10, e, coverage)
    assert new == want
    assert len(new) <= len(d10)
    print("e = %d, coverage %g: %d fixed probes, %d new, %d in a design from scratch"
          % (e, coverage, len(d5), len(new), len(d10)))
    assert f.last_timings["picks"] == len(new) and f.last_timings["rows_reduced"] == nreduced
    _check_covers(ctx, d5, c10, new, g10, e, coverage)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_fixed_probes_of_another_length_are_accepted(ctx, oracle, e):
    """75-base fixed probes beside 100-base candidates under -l 100: a probe shorter than the threshold covers
    with its full length (catch/probe.py:1297, :1332), so they take coverage away like any other."""
    g10, c10, d10, d5 = _design(e)
    short = list(dict.fromkeys(s[:75] for s in d5[:25]))
    got = _filter(e, fixed_probes=short)._filter_strs([c10], [g10], assume_unique=True)[0]
    want, _n = _oracle_extension(oracle, c10, short, g10, e, 1.0)
    assert got == want and 0 < len(got) <= len(d10)
    _check_covers(ctx, short, c10, got, g10, e, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_subtracted_scan_rows_carry_their_gain0(ctx, e):
    """Rows of a cover scan carry gain0 (per set the total length of its rows); the subtracted table carries the
    lengths of what is left, and is the NumPy subtraction of the two fetched tables."""
    from catch_amd import engine, probe
    g10, c10, _d10, d5 = _design(e)
    held = []
    try:
        targets = engine.Targets(ctx, [g.seqs for g in g10])
        held.append(targets)
        tables = []
        for strs in (c10, d5):
            k, uniq, owner, ep, eo = probe.anchor_table(strs, 2, 100, min_k=20, k=20, assume_unique=True)
            pr = engine.Probes(ctx, uniq, owner, ep, eo, k)
            held.append(pr)
            tables.append(engine.Rows.scan(ctx, pr, targets, 2, 100, 0, e))
            held.append(tables[-1])
        rows, fixed = tables
        reduced = rows.subtract(fixed)
        held.append(reduced)
        want = _np_subtract(rows.fetch(), fixed.fetch(), [g.size() for g in g10])
        got = reduced.fetch()
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        g0, gr = rows.fetch_gain0(len(c10)), reduced.fetch_gain0(len(c10))
        assert (g0 is None) == (gr is None)          # (the bucketed row build fills gain0; a radix build does not)
        print("e = %d: gain0 of the scan %s" % (e, "absent" if g0 is None else "present"))
        left = np.bincount(got[0], weights=got[3] - got[2], minlength=len(c10)).astype(np.int64)
        if gr is not None:
            assert np.array_equal(gr.astype(np.int64), left[:gr.size]) and not left[gr.size:].any()
            assert 0 < left.sum() < g0.astype(np.int64).sum()
        assert reduced.greedy(len(c10)) == _filter(e, fixed_probes=d5)._filter_strs(
            [c10], [g10], assume_unique=True)[0]
    finally:
        for h in reversed(held):
            h.close()


# ------------------------------------------------------------------ command line
def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">%s\n%s\n" % (name, s))
    return str(path)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_design_extend_probes_writes_the_new_probes(ctx, tmp_path, capsys, e):
    from catch_amd import design
    from catch_amd.utils import seq_io
    g10, c10, _d10, d5 = _design(e)
    new = _filter(e, fixed_probes=d5)._filter_strs([c10], [g10], assume_unique=True)[0]
    fa = _write_fasta(tmp_path / "ten.fasta", list(seq_io.read_fasta(EBOLA).items())[:10])
    old = _write_fasta(tmp_path / "d5.fasta", [("probe_%d" % i, s) for i, s in enumerate(d5)])
    out = str(tmp_path / "new.fasta")
    base = [fa, "-pl", "100", "-ps", "50", "-m", "2", "-e", str(e), "--extend-probes", old, "-o", out]
    capsys.readouterr()
    design.main(design.parse_args(base))
    assert capsys.readouterr().out.split() == [str(len(new))]
    assert list(seq_io.iterate_fasta(out)) == [c10[i] for i in new]
    tsv = str(tmp_path / "analysis.tsv")
    design.main(design.parse_args(base + ["--print-analysis", "--write-analysis-to-tsv", tsv]))
    text = capsys.readouterr().out
    assert "NUMBER OF PROBES: %d" % (len(d5) + len(new)) in text
    lines = open(tsv).read().splitlines()
    col = lines[0].split("\t").index("Frac bases covered")
    fracs = [float(ln.split("\t")[col]) for ln in lines[1:]]
    assert len(fracs) == 10 and all(x == 1.0 for x in fracs), fracs
