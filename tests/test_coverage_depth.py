"""Designing for a coverage depth: catchhip_rows_below_depth, SetCoverFilter(coverage_depth=D) and
`design --coverage-depth D`.

The design is a layered greedy: layer k covers, to the user's fraction, the bases that fewer than k of the picks so
far hold, with the candidates not picked yet.  _plain_depth_greedy below states that over Python sets with a
per-base depth counter; the product builds one reduced instance per layer (the unpicked sets' rows cut to the bases
below the layer's depth, restated coverage fractions) and runs the unchanged solvers on it."""
import inspect
import os
import re

import numpy as np
import pytest

from test_extend_probes import (EBOLA, REPO, _candidates, _from_host, _genomes, _instance, _np_subtract, _oracle_rows,
                                _table, _union_len, _write_fasta)

DEPTH = 3


# ------------------------------------------------------------------ host models
def _plain_depth_greedy(sets, depth, p, ranks):
    """The layered greedy over element sets.  sets[i] = {universe: set of ints}, p[u], ranks[i].  Layer k is
    catch/utils/set_cover.py:362-550 with the bases at depth >= k taken out before its first pick and the sets
    picked by earlier layers absent; unit costs, among equal ratios the lowest id.  Returns (picks per layer,
    per layer and universe (elements the solver sees, elements at depth >= k) before the layer's first pick)."""
    nuniv = len(p)
    count = [dict() for _ in range(nuniv)]           # base -> picked sets that hold it
    rank_vals = sorted(set(ranks))
    remaining = set(range(len(sets)))
    layers, sizes = [], []
    for k in range(1, depth + 1):
        fixed = {u: set(b for b, c in count[u].items() if c >= k) for u in range(nuniv)}
        universes = {u: set(fixed[u]) for u in range(nuniv)}
        for i in remaining:
            for u, s in sets[i].items():
                universes[u] |= s
        can = {u: int(len(universes[u]) - p[u] * len(universes[u])) for u in universes}
        for u in universes:
            universes[u] -= fixed[u]
        sizes.append([(len(universes[u]), len(fixed[u])) for u in range(nuniv)])
        left = {u: max(0, len(universes[u]) - can[u]) for u in universes}
        at, picks = 0, []
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
                assert at < len(rank_vals), "every element left lies in a set that is left"
                continue
            picks.append(best)
            remaining.discard(best)
            for u, s in sets[best].items():
                universes[u] -= s
                left[u] = max(0, len(universes[u]) - can[u])
                for b in s:
                    count[u][b] = count[u].get(b, 0) + 1
        layers.append(picks)
    return layers, sizes


def _np_below_depth(rows, nsets, picks, k, glen):
    """NumPy: (the rows of the sets not in picks cut into their maximal runs of bases that fewer than k picked sets
    hold, in row order; reached[u] = bases of universe u that k or more hold).  Rows as (set, universe, start, end),
    coordinates inside the universe."""
    si, un, st, en = (np.asarray(a, dtype=np.int64) for a in rows)
    off = np.concatenate([[0], np.cumsum(np.asarray(glen, dtype=np.int64))])
    total = int(off[-1])
    picked = np.zeros(max(nsets, 1), dtype=bool)
    picked[np.asarray(picks, dtype=np.int64)] = True
    m = picked[si]
    d = np.zeros(total + 1, dtype=np.int64)
    np.add.at(d, off[un[m]] + st[m], 1)
    np.add.at(d, off[un[m]] + en[m], -1)
    depth = np.cumsum(d[:total])
    done = depth >= k
    cs = np.concatenate([[0], np.cumsum(done)])
    reached = cs[off[1:]] - cs[off[:-1]]
    edge = np.diff(np.concatenate([[0], (~done).astype(np.int8), [0]]))
    run_s, run_e = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    si, un, st, en = si[~m], un[~m], st[~m], en[~m]
    gs, ge = off[un] + st, off[un] + en
    k0 = np.searchsorted(run_e, gs, side="right")
    k1 = np.searchsorted(run_s, ge, side="left")
    cnt = np.maximum(k1 - k0, 0)
    row = np.repeat(np.arange(si.size), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(k0, cnt)
    ps, pe = np.maximum(run_s[j], gs[row]), np.minimum(run_e[j], ge[row])
    table = (si[row].astype(np.int32), un[row].astype(np.int32), ps - off[un[row]], pe - off[un[row]])
    return table, reached.astype(np.int64), depth


def _oracle_depth_design(oracle, rows, nsets, glen, depth, p, ranks=None):
    """The layers through reduced instances on the host: NumPy below-depth, extension_fraction, the oracle's greedy.
    -> (picks per layer, per layer the (n2, reached, restated fractions) of layers 2.., rows per reduced table)."""
    from catch_amd.filter.set_cover_filter import extension_fraction
    ng = len(glen)
    layers, facts, nrows, picks = [], [], [], []
    for k in range(1, depth + 1):
        if k == 1:
            table, q = rows, list(p)
        else:
            table, reached, _d = _np_below_depth(rows, nsets, picks, k, glen)
            n2 = _union_len(table, ng)
            q = [extension_fraction(int(a), int(b), x) for a, b, x in zip(n2, reached, p)]
            facts.append((n2, reached, q))
            nrows.append(int(table[0].size))
        got = [] if table[0].size == 0 else \
            oracle.approx_multiuniverse(*table, nsets, ng, universe_p=q, ranks=ranks)
        layers.append(list(got))
        picks += list(got)
    return layers, facts, nrows


def _depth_and_candidates(rows, nsets, picks, glen):
    """Per base: how many of `picks` hold it, how many sets hold it at all."""
    _t, _r, depth = _np_below_depth(rows, nsets, picks, 1, glen)
    _t, _r, c = _np_below_depth(rows, nsets, list(range(nsets)), 1, glen)
    return depth, c


def _check_properties(layers, facts, rows, nsets, glen, p, d1):
    """Nesting, the depth guarantee at full coverage, the restated fractions."""
    assert layers[0] == d1                                     # layer 1 is the ordinary design ...
    for n2, reached, q in facts:
        for a, b, x, y in zip(n2, reached, p, q):
            n = int(a) + int(b)
            assert int(int(a) - y * int(a)) == min(int(n - x * n), int(a)), (a, b, x, y)
    allp = [i for layer in layers for i in layer]
    assert len(set(allp)) == len(allp)
    if all(x == 1.0 for x in p):
        depth, c = _depth_and_candidates(rows, nsets, allp, glen)
        assert (depth >= np.minimum(len(layers), c)).all()


def _cases_909():
    """The 60 instances, each at three fractions, without and with ranks (the random stream of
    test_subtract_stats_fractions_greedy_equal_the_plain_greedy)."""
    rng = np.random.default_rng(909)
    for case in range(60):
        glen, nsets, rows, _cov, sets, _fixed = _instance(rng)
        for p in (1.0, 0.9, 0.5):
            for ranks in (None, [int(x) for x in rng.choice([0, 3], size=nsets)]):
                yield case, glen, nsets, rows, sets, p, ranks


_plain_cache = {}


def _plain_909():
    """(case, p, ranked) -> the plain model's layers; computed once."""
    if not _plain_cache:
        for case, glen, nsets, _rows, sets, p, ranks in _cases_909():
            _plain_cache[(case, p, ranks is not None)] = _plain_depth_greedy(
                sets, DEPTH, [p] * len(glen), ranks or [0] * nsets)
    return _plain_cache


# ------------------------------------------------------------------ without a GPU
def test_layered_greedy_equals_the_reduced_instances_layer_by_layer(oracle):
    """The plain layered greedy == per layer the oracle's approx_multiuniverse on the NumPy below-depth rows with
    the restated fractions, pick for pick; and the three properties of the design: its first k layers are the design
    at depth k, at full coverage every base ends in min(D, candidates that hold it) picks, and the restated
    fraction leaves as many bases below the layer's depth as the user's fraction of the whole universe."""
    plain = _plain_909()
    combos = second = third = 0
    for case, glen, nsets, rows, sets, p, ranks in _cases_909():
        want, sizes = plain[(case, p, ranks is not None)]
        got, facts, _n = _oracle_depth_design(oracle, rows, nsets, glen, DEPTH, [p] * len(glen), ranks)
        assert got == want, (case, p, ranks)
        for (n2, reached, _q), per_u in zip(facts, sizes[1:]):     # the reduced instance is the model's state
            assert [(int(a), int(b)) for a, b in zip(n2, reached)] == per_u, (case, p)
        d1 = oracle.approx_multiuniverse(*rows, nsets, len(glen), universe_p=[p] * len(glen), ranks=ranks) \
            if rows[0].size else []
        _check_properties(got, facts, rows, nsets, glen, [p] * len(glen), list(d1))
        for k in (1, 2):                                           # ... and the first k layers the design at depth k
            assert _plain_depth_greedy(sets, k, [p] * len(glen), ranks or [0] * nsets)[0] == want[:k]
        combos += 1
        second += len(want[1]) > 0
        third += len(want[2]) > 0
    print("%d combinations, second layer not empty in %d, third in %d" % (combos, second, third))
    assert combos == 360 and second >= 200 and third >= 150


def test_symbol_is_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_below_depth\s*\(", hdr)
    assert "catchhip_rows_below_depth" in _lib.PROTOTYPES
    assert callable(engine.Rows.below_depth)
    assert list(inspect.signature(engine.Rows.below_depth).parameters) == ["self", "num_sets", "picks", "depth"]
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "depth.hip" in mk and "subtract.hip" in mk
    assert "#define CATCHHIP_ABI_VERSION 2\n" in hdr


def test_filter_keeps_the_reference_signature_and_takes_a_depth():
    from catch_amd.filter import set_cover_filter as scf
    # __init__ keeps the reference's arguments followed by fixed_probes (tests/test_extend_probes.py pins that
    # fixed_probes is its last); coverage_depth follows as a keyword of the call of the class
    names = list(inspect.signature(scf.SetCoverFilter.__init__).parameters)
    assert names[-2:] == ["kmer_probe_map_use_native_dict", "fixed_probes"]
    call = inspect.signature(scf.SetCoverFilter).parameters
    assert call["coverage_depth"].kind is inspect.Parameter.KEYWORD_ONLY and call["coverage_depth"].default == 1
    assert scf.SetCoverFilter(2, 100, 0, None, None, None, None, None, False, [], 1.0, 0, 20, False, None,
                              coverage_depth=2).coverage_depth == 2
    with pytest.raises(TypeError):
        scf.SetCoverFilter(2, 100, 0, None, None, None, None, None, False, [], 1.0, 0, 20, False, None, 2)
    assert scf.SetCoverFilter(2, 100).coverage_depth == 1
    f = scf.SetCoverFilter(2, 100, coverage_depth=3)
    assert f.coverage_depth == 3 and f.last_layer_sizes == []
    for bad in (0, -1, 1.5, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            scf.SetCoverFilter(2, 100, coverage_depth=bad)
    with pytest.raises(NotImplementedError):
        scf.SetCoverFilter(2, 100, fixed_probes=["ACGT" * 25], coverage_depth=2)
    assert scf.SetCoverFilter(2, 100, fixed_probes=["ACGT" * 25], coverage_depth=1).fixed_probes


def test_front_end_stays_on_the_host_above_depth_one():
    from catch_amd.filter import probe_designer, set_cover_filter as scf
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for depth, want in ((1, "per group"), (2, None), (3, None)):
        f = scf.SetCoverFilter(2, 100, coverage_depth=depth)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == want


def test_command_line_refusals(tmp_path):
    from catch_amd import design
    fa = tmp_path / "t.fasta"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    probes = tmp_path / "p.fasta"
    probes.write_text(">p\n" + "ACGT" * 25 + "\n")
    base = [str(fa), "-o", str(tmp_path / "o.fasta"), "--coverage-depth", "2"]
    assert design.parse_args([str(fa)]).coverage_depth == 1
    assert design.parse_args([str(fa)], args_type="large").coverage_depth == 1
    assert design.parse_args(base, args_type="large").coverage_depth == 2
    with pytest.raises(Exception, match="--extend-probes"):
        design.main(design.parse_args(base + ["--extend-probes", str(probes)]))
    with pytest.raises(Exception, match="--skip-set-cover"):
        design.main(design.parse_args(base + ["--skip-set-cover"]))
    with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):     # design_large's default
        design.main(design.parse_args(base, args_type="large"))
    with pytest.raises(Exception, match="--cluster-from-fragments to 0"):     # design_large with clustering alone off
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0"], args_type="large"))
    with pytest.raises(Exception, match="--coverage-depth must be at least 1"):
        design.main(design.parse_args([str(fa), "-o", str(tmp_path / "o.fasta"), "--coverage-depth", "0"]))
    with pytest.raises(SystemExit):                                           # not an integer
        design.parse_args([str(fa), "--coverage-depth", "1.5"])
    # what the messages advise parses
    args = design.parse_args(base + ["--cluster-and-design-separately", "0", "--cluster-from-fragments", "0"],
                             args_type="large")
    assert not args.cluster_and_design_separately and not args.cluster_from_fragments and args.coverage_depth == 2
    assert not os.path.exists(str(tmp_path / "o.fasta"))


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel
    from catch_amd.filter import set_cover_filter as scf

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    f = scf.SetCoverFilter(2, 100, coverage_depth=2)
    with pytest.raises(NotImplementedError):
        f._filter_strs([["ACGT" * 25]], [[]])


# ------------------------------------------------------------------ kernel: rows below a depth
def _check_below(ctx, rows, nsets, picks, k, glen, tag, R=None):
    own = R is None
    if own:
        R = _from_host(ctx, rows, glen)
    try:
        D, reached = R.below_depth(nsets, picks, k)
        try:
            want, want_reached, _d = _np_below_depth(rows, nsets, picks, k, glen)
            got = D.fetch()
            assert D.n == want[0].size, (tag, k, D.n, want[0].size)
            for g, w, name in zip(got, want, ("set", "universe", "start", "end")):
                assert np.array_equal(g, w), (tag, k, name)
            assert reached.dtype == np.int64 and np.array_equal(reached, want_reached), (tag, k, reached, want_reached)
            return got, reached
        finally:
            D.close()
    finally:
        if own:
            R.close()


def _rows_of(got):
    return [tuple(int(x[i]) for x in got) for i in range(got[0].size)]


def _hand_made_cases():
    """name -> (universe lengths, rows (set, universe, start, end), number of sets, picks, depths)."""
    alt = [(2 + j, 0, s, s + 1) for j, s in enumerate(range(11, 11 + 257, 2))]     # every other base of [10, 267)
    rng = np.random.default_rng(3)
    holes = sorted(set(int(x) for x in rng.integers(100, 5100, size=400)))
    return {
        "runs that start or end at bit 63 or 64 of a word": (
            [400], [(0, 0, 0, 400), (1, 0, 63, 64), (2, 0, 64, 65), (3, 0, 100, 127), (4, 0, 128, 191),
                    (5, 0, 191, 193), (6, 0, 255, 257), (7, 0, 300, 320), (8, 0, 60, 130)],
            9, [1, 2, 3, 4, 5, 6, 7], (1, 2)),
        "a run to a universe's last base, the next universe's first base reached too": (
            [100, 100, 28], [(0, 0, 90, 100), (0, 1, 0, 10), (1, 0, 80, 100), (1, 1, 0, 30), (2, 0, 0, 100),
                             (2, 1, 0, 100), (2, 2, 0, 28), (3, 1, 95, 100), (3, 2, 0, 5), (4, 1, 90, 100),
                             (4, 2, 0, 28)],
            5, [0, 1, 3], (1, 2, 3)),
        "a picked row that ends at total": (
            [64, 64], [(0, 1, 10, 64), (1, 0, 0, 64), (1, 1, 0, 64), (2, 1, 63, 64), (3, 1, 0, 64)],
            4, [0, 2], (1, 2, 3)),
        "a picked row that ends at total, total no multiple of 64": (
            [64, 37], [(0, 1, 30, 37), (1, 0, 60, 64), (1, 1, 0, 37), (2, 1, 36, 37)], 3, [0, 2], (1, 2, 3)),
        "three picked sets, depth 1-2-3-2-1": (
            [300], [(0, 0, 10, 110), (1, 0, 30, 90), (2, 0, 50, 70), (3, 0, 0, 300), (4, 0, 60, 65), (5, 0, 20, 55)],
            6, [0, 1, 2], (1, 2, 3, 4)),
        "depth greater than the number of picks": (
            [300], [(0, 0, 10, 110), (1, 0, 30, 90), (2, 0, 0, 300)], 3, [0, 1], (3, 7, 1000)),
        "no picks": ([300, 20], [(0, 0, 10, 50), (3, 0, 20, 30), (3, 1, 0, 20)], 4, [], (1, 2)),
        "all sets picked": ([300, 20], [(0, 0, 10, 50), (1, 0, 20, 30), (1, 1, 0, 20)], 2, [1, 0], (1, 2, 3)),
        "a set without rows picked, an empty table": ([300], [], 3, [1], (1,)),
        "257 bases under alternating picks: 129 pieces (all words loaded first)": (
            [400], [(0, 0, 10, 267)] + alt, 2 + len(alt), list(range(2, 2 + len(alt))), (1, 2)),
        "5,000 bases with a few hundred picked bases (the loop over words)": (
            [6000], [(0, 0, 100, 5100), (1, 0, 0, 6000)] + [(2 + j, 0, h, h + 1) for j, h in enumerate(holes)],
            2 + len(holes), list(range(2, 2 + len(holes))), (1, 2)),
        "a universe of one base, a row of one base": (
            [1, 50, 1], [(0, 0, 0, 1), (0, 1, 7, 8), (1, 0, 0, 1), (1, 1, 0, 50), (1, 2, 0, 1), (2, 2, 0, 1),
                         (3, 1, 7, 8)],
            4, [0, 2], (1, 2)),
        "one universe of one base": ([1], [(0, 0, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)], 3, [1], (1, 2)),
    }


@pytest.mark.gpu
def test_rows_below_depth_hand_made_cases(ctx):
    cases = _hand_made_cases()
    for tag, (glen, rows, nsets, picks, depths) in cases.items():
        table = _table(rows)
        for k in depths:
            got, reached = _check_below(ctx, table, nsets, picks, k, glen, tag)
            if tag.startswith("three picked sets"):
                three = {1: [(3, 0, 0, 10), (3, 0, 110, 300)],
                         2: [(3, 0, 0, 30), (3, 0, 90, 300), (5, 0, 20, 30)],
                         3: [(3, 0, 0, 50), (3, 0, 70, 300), (5, 0, 20, 50)],
                         4: [(3, 0, 0, 300), (4, 0, 60, 65), (5, 0, 20, 55)]}
                assert _rows_of(got) == three[k] and reached.tolist() == [{1: 100, 2: 60, 3: 20, 4: 0}[k]]
            if tag.startswith("depth greater"):
                assert _rows_of(got) == [(2, 0, 0, 300)] and reached.tolist() == [0]
            if tag == "no picks":
                assert _rows_of(got) == rows and not reached.any()
            if tag == "all sets picked":
                assert got[0].size == 0 and reached.tolist() == {1: [40, 20], 2: [10, 0], 3: [0, 0]}[k]
            if tag.startswith("257 bases") and k == 1:
                assert got[0].size == 129 and (got[3] - got[2] == 1).all() and reached.tolist() == [129]
            if tag.startswith("5,000 bases") and k == 1:
                assert got[0].size > 600
            if tag.startswith("a run to a universe's last base") and k == 1:
                # sets 0, 1, 3 reach [80, 100) of universe 0, [0, 30) and [95, 100) of 1, [0, 5) of 2
                assert reached.tolist() == [20, 35, 5]
                assert _rows_of(got) == [(2, 0, 0, 80), (2, 1, 30, 95), (2, 2, 5, 28), (4, 1, 90, 95), (4, 2, 5, 28)]


@pytest.mark.gpu
def test_rows_below_depth_refusals(ctx):
    R = _from_host(ctx, _table([(0, 0, 10, 50), (1, 0, 0, 5), (2, 1, 0, 9)]), [100, 50])
    try:
        for picks, depth, what in (([0], 0, "smallest depth"), ([0], -3, "smallest depth"),
                                   ([3], 1, "outside the set ids"), ([-1], 1, "outside the set ids"),
                                   ([0, 1, 0], 1, "given twice"), ([0, 1, 2, 1], 2, "picks of 3 sets")):
            with pytest.raises(ValueError, match=what):
                R.below_depth(3, picks, depth)
        D, reached = R.below_depth(3, [1, 2], 1)          # ... and the table serves the next call
        assert _rows_of(D.fetch()) == [(0, 0, 10, 50)] and reached.tolist() == [5, 9]
        D.close()
    finally:
        R.close()


def _big_table(rng, nsets, nuniv, per, gap_hi, len_hi):
    g = rng.integers(1, gap_hi, size=(nsets, nuniv, per))
    ln = rng.integers(1, len_hi, size=(nsets, nuniv, per))
    en = np.cumsum(g + ln, axis=2)
    st = en - ln
    si = np.broadcast_to(np.arange(nsets)[:, None, None], st.shape)
    un = np.broadcast_to(np.arange(nuniv)[None, :, None], st.shape)
    glen = en.max(axis=(0, 2))
    return (si.reshape(-1).astype(np.int32), un.reshape(-1).astype(np.int32), st.reshape(-1), en.reshape(-1)), \
        [int(x) for x in glen]


@pytest.mark.gpu
def test_rows_below_depth_random_tables(ctx):
    """A few thousand rows in up to 6 universes under random picks at depths 1 to 4, against NumPy; at depth 1 also
    against catchhip_rows_subtract: the unpicked sets' rows minus the picked sets' rows."""
    rng = np.random.default_rng(4242)
    cut = deep = 0
    for case in range(6):
        nsets, nuniv = int(rng.integers(20, 60)), int(rng.integers(1, 7))
        rows, glen = _big_table(rng, nsets, nuniv, int(rng.integers(4, 20)), 60, 330 if case % 2 else 120)
        assert 80 * nuniv <= rows[0].size < 8000
        R = _from_host(ctx, rows, glen)
        try:
            for frac in (0.1, 0.5, 0.9):
                picks = [int(x) for x in rng.permutation(nsets)[:max(1, int(frac * nsets))]]
                for k in (1, 2, 3, 4):
                    got, reached = _check_below(ctx, rows, nsets, picks, k, glen, (case, frac), R=R)
                    cut += got[0].size
                    deep += k >= 3 and int(reached.sum()) > 0
                m = np.isin(rows[0], picks)
                A = _from_host(ctx, tuple(a[~m] for a in rows), glen)
                B = _from_host(ctx, tuple(a[m] for a in rows), glen)
                S = A.subtract(B)
                D, _r = R.below_depth(nsets, picks, 1)
                try:
                    assert S.n == D.n
                    for a, b in zip(S.fetch(), D.fetch()):
                        assert np.array_equal(a, b)
                    want = _np_subtract(tuple(a[~m] for a in rows), tuple(a[m] for a in rows), glen)
                    for a, b in zip(D.fetch(), want):
                        assert np.array_equal(a, b)
                finally:
                    for h in (A, B, S, D):
                        h.close()
        finally:
            R.close()
    assert cut > 20000 and deep >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("edge", [2048 * 1024, 2048 * 2048])
def test_rows_below_depth_where_the_scan_takes_further_passes(ctx, edge):
    """A few hundred rows in a coordinate space just above 2,097,152 bases (the scan of the depth array runs its
    second level over more than half a tile of tile sums) and just above 2048^2 (its third level), with rows on
    both sides of, across and ending at the edge."""
    rng = np.random.default_rng(edge)
    total = edge + 700
    rows = []
    for i in range(40):
        starts = np.sort(rng.choice(total // 400 - 1, size=6, replace=False)) * 400
        rows += [(i, 0, int(s) + int(rng.integers(0, 100)), int(s) + int(rng.integers(150, 390))) for s in starts]
    near = [(40, edge - 300, edge), (40, edge + 1, edge + 300), (41, edge - 100, edge + 100),
            (42, edge - 1, edge + 1), (43, edge, edge + 64), (44, edge - 2048, edge + 690),
            (45, edge - 64, edge - 1), (46, edge - 200, edge + 650), (47, edge + 600, total),
            (48, 0, 3), (49, edge - 50, edge + 50)]
    rows += [(i, 0, s, t) for i, s, t in near]
    rows.sort()
    table = _table(rows)
    assert 200 < table[0].size < 400
    R = _from_host(ctx, table, [total])
    try:
        picks = list(range(0, 40, 2)) + [40, 41, 42, 44, 47]
        for k in (1, 2, 3):
            got, reached = _check_below(ctx, table, 50, picks, k, [total], edge, R=R)
            assert got[0].size > 0 and (k == 3 or reached[0] > 0)
    finally:
        R.close()


# ------------------------------------------------------------------ rows level, end to end
@pytest.mark.gpu
def test_device_layers_equal_the_plain_layered_greedy(ctx):
    """from_host, below_depth, stats, extension_fraction, greedy per layer == the plain model, pick for pick; every
    layer's picks pass cover_check on the layer's own table."""
    from catch_amd.filter.set_cover_filter import extension_fraction
    plain = _plain_909()
    combos = second = third = 0
    tables = {}
    try:
        for case, glen, nsets, rows, _sets, p, ranks in _cases_909():
            if case not in tables:
                for h in tables.values():
                    h.close()
                tables.clear()
                tables[case] = _from_host(ctx, rows, glen)
            R = tables[case]
            want, sizes = plain[(case, p, ranks is not None)]
            picks, got = [], []
            for k in range(1, DEPTH + 1):
                if k == 1:
                    T, up = R, (None if p == 1.0 else [p] * len(glen))
                else:
                    T, reached = R.below_depth(nsets, picks, k)
                    n2 = T.stats(len(glen))[1]
                    assert [(int(a), int(b)) for a, b in zip(n2, reached)] == sizes[k - 1], (case, p, k)
                    q = [extension_fraction(int(a), int(b), p) for a, b in zip(n2, reached)]
                    up = None if all(x == 1.0 for x in q) else q
                try:
                    layer = T.greedy(nsets, ranks, up) if T.n else []
                    if T.n:
                        chk = T.cover_check(nsets, layer, up)
                        assert chk["universes_short"] == 0 and chk["picks_without_gain"] == 0 \
                            and chk["bad_pick_ids"] == 0, (case, p, k, chk)
                finally:
                    if T is not R:
                        T.close()
                got.append(layer)
                picks += layer
            assert got == want, (case, p, ranks)
            combos += 1
            second += len(got[1]) > 0
            third += len(got[2]) > 0
    finally:
        for h in tables.values():
            h.close()
    print("%d combinations, second layer not empty in %d, third in %d" % (combos, second, third))
    assert combos == 360 and second >= 200 and third >= 150


# ------------------------------------------------------------------ filter level
def _filter(e, coverage=1.0, **kw):
    from catch_amd.filter import set_cover_filter as scf
    return scf.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=coverage, cover_extension=e, **kw)


_five = {}


def _ebola5():
    if not _five:
        g5 = _genomes(5)
        _five["g"], _five["c"] = g5, _candidates(g5)
    return _five["g"], _five["c"]


def _scan_rows(ctx, strs, genomes, e):
    from catch_amd import engine, probe
    k, uniq, owner, ep, eo = probe.anchor_table(strs, 2, 100, min_k=20, k=20, assume_unique=True)
    targets = engine.Targets(ctx, [g.seqs for g in genomes])
    probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
    return engine.Rows.scan(ctx, probes, targets, 2, 100, 0, e), probes, targets


@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_designs_three_layers_on_five_genomes(ctx, oracle, e, coverage):
    g5, c5 = _ebola5()
    glen = [g.size() for g in g5]
    f = _filter(e, coverage, coverage_depth=DEPTH)
    got = f._filter_strs([c5], [g5], assume_unique=True)
    assert len(got) == 1
    got = got[0]
    rows = _oracle_rows(oracle, c5, g5, e)
    layers, _facts, nrows = _oracle_depth_design(oracle, rows, len(c5), glen, DEPTH, [coverage] * len(glen))
    print("e = %d, coverage %g: %d candidates, %d rows, picks per layer %s (oracle model %s), depth_ms %.3f"
          % (e, coverage, len(c5), rows[0].size, " / ".join(str(x) for x in f.last_layer_sizes[0]),
             " / ".join(str(len(x)) for x in layers), f.last_timings["depth_ms"]))
    assert got == [i for layer in layers for i in layer]
    assert f.last_layer_sizes == [[len(x) for x in layers]]
    first = f.last_layer_sizes[0][0]
    assert first > 0 and f.last_layer_sizes[0][1] > 0 and f.last_layer_sizes[0][2] > 0
    assert got[:first] == _filter(e, coverage, coverage_depth=1)._filter_strs([c5], [g5], assume_unique=True)[0]
    assert got[:first] == _filter(e, coverage)._filter_strs([c5], [g5], assume_unique=True)[0]
    assert f.last_timings["depth_ms"] > 0 and f.last_timings["picks"] == len(got)
    assert f.last_timings["rows_reduced"] == sum(nrows) and f.last_timings["rows"] == rows[0].size
    if coverage == 1.0:
        scanned, probes, targets = _scan_rows(ctx, c5, g5, e)
        try:
            table = scanned.fetch()
        finally:
            for h in (scanned, probes, targets):
                h.close()
        depth, c = _depth_and_candidates(table, len(c5), got, glen)
        short = int(np.count_nonzero(c < DEPTH))
        print("    %d of %d bases lie in fewer than %d candidates; minimum depth %d"
              % (short, depth.size, DEPTH, int(depth.min())))
        assert (depth >= np.minimum(DEPTH, c)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_below_depth_of_scan_rows_carries_its_gain0(ctx, e):
    """Rows of a cover scan carry gain0 (per set the total length of its rows); the table below a depth carries the
    lengths of its pieces, nothing for the picked sets, and is the NumPy cut of the fetched table."""
    g5, c5 = _ebola5()
    glen = [g.size() for g in g5]
    scanned, probes, targets = _scan_rows(ctx, c5, g5, e)
    held = [targets, probes, scanned]
    try:
        table = scanned.fetch()
        picks = _filter(e)._filter_strs([c5], [g5], assume_unique=True)[0]
        g0 = scanned.fetch_gain0(len(c5))
        print("e = %d: gain0 of the scan %s" % (e, "absent" if g0 is None else "present"))
        for k, pk in ((1, picks), (2, picks), (2, picks[:len(picks) // 2]), (1, [])):
            D, reached = scanned.below_depth(len(c5), pk, k)
            held.append(D)
            want, want_reached, _d = _np_below_depth(table, len(c5), pk, k, glen)
            got = D.fetch()
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
            assert np.array_equal(reached, want_reached)
            gr = D.fetch_gain0(len(c5))
            assert (g0 is None) == (gr is None)
            left = np.bincount(got[0], weights=got[3] - got[2], minlength=len(c5)).astype(np.int64)
            if gr is not None:
                assert np.array_equal(gr.astype(np.int64), left[:gr.size]) and not left[gr.size:].any()
                assert not gr[np.asarray(pk, dtype=np.int64)].any()
                if len(pk) == 0:
                    assert np.array_equal(gr, g0)
            if k == 1 and len(pk):
                assert D.n == 0 or left.sum() < (table[3] - table[2]).sum()
    finally:
        for h in reversed(held):
            h.close()


# ------------------------------------------------------------------ command line
@pytest.mark.gpu
def test_design_coverage_depth_writes_the_layers_in_order(ctx, tmp_path, capsys):
    from catch_amd import design
    from catch_amd.utils import seq_io
    g3 = _genomes(3)
    c3 = _candidates(g3)
    f = _filter(0, coverage_depth=2)
    want = f._filter_strs([c3], [g3], assume_unique=True)[0]
    sizes = f.last_layer_sizes[0]
    assert len(sizes) == 2 and sizes[0] > 0 and sizes[1] > 0
    fa = _write_fasta(tmp_path / "three.fasta", list(seq_io.read_fasta(EBOLA).items())[:3])
    one, two = str(tmp_path / "one.fasta"), str(tmp_path / "two.fasta")
    base = [fa, "-pl", "100", "-ps", "50", "-m", "2", "-e", "0"]
    capsys.readouterr()
    design.main(design.parse_args(base + ["-o", one]))
    assert capsys.readouterr().out.split() == [str(sizes[0])]
    design.main(design.parse_args(base + ["--coverage-depth", "2", "-o", two]))
    assert capsys.readouterr().out.split() == [str(sizes[0] + sizes[1])]
    assert list(seq_io.iterate_fasta(two)) == [c3[i] for i in want]
    a, b = open(one, "rb").read(), open(two, "rb").read()
    assert len(a) > 0 and len(b) > len(a) and b[:len(a)] == a
