"""Pruning redundant picks: catchhip_rows_prune, engine.Rows.prune, SetCoverFilter(prune_redundant=True),
`design --prune-redundant` and `python -m catch_amd.prune_probes`.

The definition is a sequential walk: depth(b) = the picked sets with a row over base b plus the fixed rows over it;
the picks are examined from the last picked to the first, and one is removed if at its turn every base of its rows
has depth >= D + 1, which lowers those depths by 1.  _walk_sets below states that over Python sets (_walk is the same
over NumPy slices, for the large tables); the device reproduces it in parallel rounds, which _rounds models."""
import inspect
import os
import re
from collections import Counter

import numpy as np
import pytest

from test_coverage_depth import _big_table, _ebola5, _filter, _oracle_depth_design
from test_extend_probes import (EBOLA, REPO, _design, _from_host, _instance, _oracle_extension, _oracle_rows, _table,
                                _write_fasta)


# ------------------------------------------------------------------ host models
def _walk_sets(sets, picks, depth, fixed_rows=()):
    """The walk over element sets.  sets[i] = {universe: set of ints}; fixed_rows = (universe, start, end) triples,
    every one counts.  -> (kept in pick order, removed in examination order, depth per (universe, base) before and
    after, the picks removable before the first removal)."""
    count = Counter()
    for u, s, t in fixed_rows:
        for b in range(s, t):
            count[(u, b)] += 1
    for i in picks:
        for u, el in sets[i].items():
            for b in el:
                count[(u, b)] += 1
    before = Counter(count)
    removable = [i for i in picks if all(count[(u, b)] >= depth + 1 for u, el in sets[i].items() for b in el)]
    removed = []
    for i in reversed(picks):
        if all(count[(u, b)] >= depth + 1 for u, el in sets[i].items() for b in el):
            removed.append(i)
            for u, el in sets[i].items():
                for b in el:
                    count[(u, b)] -= 1
    gone = set(removed)
    return [i for i in picks if i not in gone], removed, before, count, removable


def _global_rows(rows, glen):
    """set id -> [(global start, global end)], the universes' offsets, total."""
    si, un, st, en = (np.asarray(a, dtype=np.int64) for a in rows)
    off = np.concatenate([[0], np.cumsum(np.asarray(glen, dtype=np.int64))])
    by_set = {}
    for i, a, b in zip(si.tolist(), (off[un] + st).tolist(), (off[un] + en).tolist()):
        by_set.setdefault(i, []).append((a, b))
    return by_set, off, int(off[-1])


def _depth_of(by_set, total, picks, fixed, glen):
    depth = np.zeros(total, dtype=np.int64)
    for i in picks:
        for a, b in by_set.get(i, ()):
            depth[a:b] += 1
    if fixed is not None:
        for rr in _global_rows(fixed, glen)[0].values():
            for a, b in rr:
                depth[a:b] += 1
    return depth


def _walk(rows, glen, picks, depth, fixed=None):
    """The walk over NumPy slices of the global coordinate space.  rows / fixed = (set, universe, start, end) arrays.
    -> (kept in pick order, removed in examination order, depth per base before, after)."""
    by_set, _off, total = _global_rows(rows, glen)
    d = _depth_of(by_set, total, picks, fixed, glen)
    before = d.copy()
    removed = []
    for i in reversed(picks):
        rr = by_set.get(i, ())
        if all((d[a:b] >= depth + 1).all() for a, b in rr):
            removed.append(i)
            for a, b in rr:
                d[a:b] -= 1
    gone = set(removed)
    return [i for i in picks if i not in gone], removed, before, d


def _rounds(rows, glen, picks, depth, fixed=None, rng=None):
    """The round scheme of csrc/prune.hip, without its one-workgroup tail.  rng: the candidates enter the per-base
    counts in a random order (what the order of the atomics may be).  -> (kept, removed, rounds)."""
    by_set, _off, total = _global_rows(rows, glen)
    d = _depth_of(by_set, total, picks, fixed, glen)
    exam = {s: e for e, s in enumerate(reversed(picks))}

    def removable(i):
        return all((d[a:b] >= depth + 1).all() for a, b in by_set.get(i, ()))

    cands = [i for i in picks if removable(i)]          # (the others are kept for good)
    removed, rounds = [], 0
    while cands:
        rounds += 1
        cand = np.zeros(total, dtype=np.int64)
        first = np.full(total, len(picks), dtype=np.int64)
        for i in (cands if rng is None else [cands[j] for j in rng.permutation(len(cands))]):
            for a, b in by_set.get(i, ()):
                cand[a:b] += 1
                first[a:b] = np.minimum(first[a:b], exam[i])
        gone = [i for i in cands
                if all(((d[a:b] - cand[a:b] >= depth) | (first[a:b] == exam[i])).all() for a, b in by_set.get(i, ()))]
        assert gone and min(cands, key=exam.get) in gone     # the earliest candidate always passes
        for i in gone:
            for a, b in by_set.get(i, ()):
                d[a:b] -= 1
        removed += gone
        cands = [i for i in cands if i not in gone and removable(i)]
    removed.sort(key=exam.get)
    gone = set(removed)
    return [i for i in picks if i not in gone], removed, rounds


def _cases_1213():
    """The 60 instances at D = 1, 2, 3 under two pick lists each: a random permutation of the non-empty sets and
    its first 60 %.  -> (case, glen, nsets, rows, fixed rows table, sets, D, picks)."""
    rng = np.random.default_rng(1213)
    for case in range(60):
        glen, nsets, rows, cov, sets, _fixed = _instance(rng)
        nonempty = [i for i in range(nsets) if sets[i]]
        for depth in (1, 2, 3):
            perm = [int(x) for x in rng.permutation(nonempty)]
            for picks in (perm, perm[:int(0.6 * len(perm))]):
                yield case, glen, nsets, rows, cov, sets, depth, picks


_walk_cache = {}


def _walks_1213():
    """[(case, glen, nsets, rows, cov, D, picks, (kept, removed) without fixed rows, (kept, removed) with them,
    conflict)], computed once over Python sets."""
    if not _walk_cache:
        out = []
        for case, glen, nsets, rows, cov, sets, depth, picks in _cases_1213():
            kept, removed, _b, _a, removable = _walk_sets(sets, picks, depth)
            fixed_rows = list(zip(cov[1].tolist(), cov[2].tolist(), cov[3].tolist()))
            fk, fr, _b, _a, _r = _walk_sets(sets, picks, depth, fixed_rows)
            out.append((case, glen, nsets, rows, cov, depth, picks, (kept, removed), (fk, fr),
                        any(i in kept for i in removable)))
        _walk_cache["all"] = out
    return _walk_cache["all"]


# ------------------------------------------------------------------ without a GPU
def test_symbol_is_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_prune\s*\(", hdr)
    assert "catchhip_rows_prune" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["catchhip_rows_prune"][1]) == 10
    assert callable(engine.Rows.prune)
    sig = inspect.signature(engine.Rows.prune).parameters
    assert list(sig) == ["self", "num_sets", "picks", "depth", "fixed"]
    assert sig["depth"].default == 1 and sig["fixed"].default is None
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "prune.hip" in mk and "depth.hip" in mk
    assert "#define CATCHHIP_ABI_VERSION 2\n" in hdr
    src = open(os.path.join(REPO, "catch_amd", "csrc", "prune.hip")).read()
    # the depth machinery is shared with depth.hip, not copied
    for name in ("chip_depth_marks", "chip_depth_array", "chip_depth_bitmap"):
        assert name in src
    assert "dp_diff_kernel" not in src and "double" not in src and "float" not in src


def test_filter_keeps_the_reference_signature_and_takes_prune_redundant():
    from catch_amd.filter import set_cover_filter as scf
    names = list(inspect.signature(scf.SetCoverFilter.__init__).parameters)
    assert names[-2:] == ["kmer_probe_map_use_native_dict", "fixed_probes"]
    call = inspect.signature(scf.SetCoverFilter).parameters
    assert call["prune_redundant"].kind is inspect.Parameter.KEYWORD_ONLY and call["prune_redundant"].default is False
    assert call["coverage_depth"].kind is inspect.Parameter.KEYWORD_ONLY and call["coverage_depth"].default == 1
    f = scf.SetCoverFilter(2, 100)
    assert f.prune_redundant is False and f.last_pruned == []
    f = scf.SetCoverFilter(2, 100, 0, None, None, None, None, None, False, [], 1.0, 0, 20, False, None,
                           prune_redundant=True)
    assert f.prune_redundant is True and f.coverage_depth == 1
    with pytest.raises(TypeError):
        scf.SetCoverFilter(2, 100, 0, None, None, None, None, None, False, [], 1.0, 0, 20, False, None, 1, True)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            scf.SetCoverFilter(2, 100, prune_redundant=bad)
    assert scf.SetCoverFilter(2, 100, coverage_depth=3, prune_redundant=True).coverage_depth == 3
    assert scf.SetCoverFilter(2, 100, fixed_probes=["ACGT" * 25], prune_redundant=True).fixed_probes


def test_front_end_stays_on_the_host_when_pruning():
    from catch_amd.filter import probe_designer, set_cover_filter as scf
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for prune, want in ((False, "per group"), (True, None)):
        f = scf.SetCoverFilter(2, 100, prune_redundant=prune)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == want


def test_command_line_refusals(tmp_path):
    from catch_amd import analyze_probe_coverage, design, design_grid, pool, prune_probes
    fa = tmp_path / "t.fasta"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    probes = tmp_path / "p.fasta"
    probes.write_text(">p\n" + "ACGT" * 25 + "\n")
    out = str(tmp_path / "o.fasta")
    base = [str(fa), "-o", out, "--prune-redundant"]
    assert design.parse_args([str(fa)]).prune_redundant is False
    assert design.parse_args(base).prune_redundant is True
    assert design.parse_args(base, args_type="large").prune_redundant is True
    with pytest.raises(Exception, match="--prune-redundant with --skip-set-cover"):
        design.main(design.parse_args(base + ["--skip-set-cover"]))
    with pytest.raises(Exception, match="--prune-redundant with --cluster-and-design-separately"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="--prune-redundant with --cluster-and-design-separately"):   # design_large
        design.main(design.parse_args(base, args_type="large"))
    with pytest.raises(Exception, match="--prune-redundant with --cluster-from-fragments"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0"], args_type="large"))
    # allowed beside --extend-probes and --coverage-depth: what the messages advise parses
    args = design.parse_args(base + ["--cluster-and-design-separately", "0", "--cluster-from-fragments", "0",
                                     "--coverage-depth", "2"], args_type="large")
    assert args.prune_redundant and args.coverage_depth == 2 and not args.cluster_and_design_separately
    assert design.parse_args(base + ["--extend-probes", str(probes)]).prune_redundant
    assert not os.path.exists(out)
    # the other commands do not know the option
    for parse, argv in ((design_grid.parse_args, [str(fa), "--grid-mismatches", "0", "--grid-cover-extension", "0",
                                                  "-o", str(tmp_path / "grid")]),
                        (pool._parser().parse_args, ["counts.tsv", "100", "params.tsv"]),
                        (analyze_probe_coverage.parse_args, ["-d", str(fa), "-f", str(probes), "-m", "0", "-l", "100"])):
        parse(argv)
        with pytest.raises(SystemExit):
            parse(argv + ["--prune-redundant"])
    # prune_probes: its options, and a depth below 1
    args = prune_probes.parse_args(["-d", str(fa), str(fa), "-f", str(probes), "-o", out, "-m", "2", "-l", "100",
                                    "-e", "50", "--island-of-exact-match", "0", "--kmer-probe-map-k", "20",
                                    "--coverage-depth", "2", "--write-removed", str(tmp_path / "r.fasta")])
    assert args.coverage_depth == 2 and args.cover_extension == 50 and len(args.dataset) == 2
    with pytest.raises(SystemExit):
        prune_probes.parse_args(["-d", str(fa), "-f", str(probes)])               # no -o
    with pytest.raises(ValueError, match="--coverage-depth must be at least 1"):
        prune_probes.main(prune_probes.parse_args(["-d", str(fa), "-f", str(probes), "-o", out,
                                                   "--coverage-depth", "0"]))
    assert not os.path.exists(out)


def test_help_says_that_the_layers_no_longer_nest(capsys):
    from catch_amd import design
    with pytest.raises(SystemExit):
        design.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--prune-redundant" in text and "no longer the design at depth k" in text


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel
    from catch_amd.filter import set_cover_filter as scf

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    for kw in (dict(), dict(coverage_depth=2), dict(fixed_probes=["ACGT" * 25])):
        f = scf.SetCoverFilter(2, 100, prune_redundant=True, **kw)
        with pytest.raises(NotImplementedError):
            f._filter_strs([["ACGT" * 25]], [[]])
    with pytest.raises(NotImplementedError):
        scf.SetCoverFilter(2, 100).prune_probe_strs(["ACGT" * 25], [])


def test_walk_consequences_and_the_round_scheme_on_the_360_combinations():
    """On every combination, without and with the instance's fixed rows: the walk over Python sets == the walk over
    NumPy slices == the round scheme (candidates in pick order and in a shuffled order: one fixed answer); min(depth,
    D) is the same before and after for every base; after the pass no kept pick is removable."""
    rng = np.random.default_rng(5)
    combos = something = conflicts = multi = 0
    for case, glen, nsets, rows, cov, depth, picks, plain, with_fixed, conflict in _walks_1213():
        for fixed, want in ((None, plain), (cov, with_fixed)):
            kept, removed, before, after = _walk(rows, glen, picks, depth, fixed)
            assert (kept, removed) == want, (case, depth, picks)
            assert sorted(kept + removed) == sorted(picks)
            assert np.array_equal(np.minimum(before, depth), np.minimum(after, depth))
            assert _walk(rows, glen, kept, depth, fixed)[1] == []            # nothing left to remove
            r1 = _rounds(rows, glen, picks, depth, fixed)
            r2 = _rounds(rows, glen, picks, depth, fixed, rng)
            assert r1[:2] == want and r2[:2] == want, (case, depth, picks)
            multi += r1[2] > 1
        combos += 1
        something += len(plain[1]) > 0
        conflicts += conflict
    print("%d combinations: the walk removes something in %d, keeps a pick that was removable at the start in %d; "
          "the rounds take more than one round in %d of %d runs" % (combos, something, conflicts, multi, 2 * combos))
    assert combos == 360 and something >= 100 and conflicts >= 20


# ------------------------------------------------------------------ kernel, through the C ABI
def _check_prune(rows, glen, nsets, picks, depth, R, fixed=None, F=None, tag=None, want=None):
    kept, removed = R.prune(nsets, picks, depth, F)
    if want is None:
        want = _walk(rows, glen, picks, depth, fixed)[:2]
    assert (kept, removed) == tuple(want), (tag, depth, picks, kept, removed, want)
    return kept, removed


def _hand_made_cases():
    """name -> (universe lengths, rows (set, universe, start, end), number of sets, pick lists, fixed rows or None,
    {(depth, pick list index): removed} where the answer is written out)."""
    words = [(0, 0, 0, 400), (1, 0, 0, 400), (2, 0, 63, 64), (3, 0, 64, 65), (4, 0, 0, 63), (5, 0, 0, 64),
             (6, 0, 0, 65), (7, 0, 63, 128), (8, 0, 64, 128), (9, 0, 65, 129), (10, 0, 1, 63), (11, 0, 127, 193),
             (12, 0, 191, 192), (13, 0, 192, 256)]
    abc = [(0, 0, 0, 100), (1, 0, 50, 150), (2, 0, 0, 20), (2, 0, 100, 200), (3, 0, 20, 50), (3, 0, 150, 300)]
    return {
        "two identical sets: the later examined one stays": (
            [300], [(0, 0, 10, 50), (0, 0, 60, 70), (1, 0, 10, 50), (1, 0, 60, 70)], 2, [[0, 1], [1, 0]], None,
            {(1, 0): [1], (1, 1): [0], (2, 0): [], (2, 1): []}),
        "A, B, C conflict pairwise over a base layer": (
            [300], abc, 4, [[3, 0, 1, 2], [3, 2, 1, 0], [0, 1, 2, 3], [1, 3, 0, 2]], None,
            # (picked first, the base layer is examined last; picked last, it stays for its bases beyond 200)
            {(1, 0): [2], (1, 1): [0], (1, 2): [2], (2, 0): []}),
        "rows that start or end at bits 63, 64 and 65 of a word": (
            [400], words, 14, [list(range(14)), list(range(13, -1, -1)), [0, 2, 3, 5, 7, 9, 11, 13, 1]], None, {}),
        "a row that ends at total": (
            [64, 37], [(0, 1, 30, 37), (1, 0, 0, 64), (1, 1, 0, 37), (2, 1, 36, 37), (3, 0, 60, 64), (3, 1, 0, 37)],
            4, [[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 2]], None, {}),
        "a conflict on either side of a universe boundary": (
            # 0 and 1 conflict in universe 0, 2 and 3 in universe 1; 0 ends where universe 0 ends, 2 starts where
            # universe 1 starts: the last base of one universe and the first of the next share no depth
            [100, 100], [(0, 0, 80, 100), (1, 0, 70, 100), (2, 1, 0, 20), (3, 1, 0, 30), (4, 0, 0, 80), (4, 1, 20, 100)],
            5, [[4, 0, 1, 2, 3], [4, 1, 0, 3, 2], [4, 0, 3, 1, 2]], None,
            {(1, 0): [3, 1], (1, 1): [2, 0], (1, 2): [2, 1]}),
        "fixed rows that make every pick removable": (
            [200, 50], [(0, 0, 0, 100), (1, 0, 100, 200), (2, 1, 0, 50)], 3, [[0, 1, 2], [2, 0, 1]],
            [(0, 0, 0, 200), (0, 1, 0, 50), (1, 0, 0, 200), (1, 1, 0, 50), (7, 0, 0, 200), (7, 1, 0, 50)],
            {(1, 0): [2, 1, 0], (2, 0): [2, 1, 0], (3, 0): [2, 1, 0], (3, 1): [1, 0, 2]}),
        "fixed rows that make nothing removable": (
            # every pick keeps one base the fixed rows miss
            [200, 50], [(0, 0, 0, 100), (1, 0, 100, 200), (2, 1, 0, 50)], 3, [[0, 1, 2], [2, 0, 1]],
            [(0, 0, 1, 199), (0, 1, 0, 49), (1, 0, 1, 99), (1, 0, 100, 199)],
            {(1, 0): [], (2, 0): [], (3, 0): [], (1, 1): []}),
        "a pick without rows covers nothing alone": (
            [300], [(0, 0, 10, 50), (2, 0, 10, 50)], 4, [[0, 1, 2, 3], [3, 1]], None,
            {(1, 0): [3, 2, 1], (2, 0): [3, 1], (1, 1): [1, 3]}),
        "no picks": ([300, 20], [(0, 0, 10, 50), (3, 0, 20, 30), (3, 1, 0, 20)], 4, [[]], None, {(1, 0): []}),
        "an empty table": ([300], [], 3, [[1, 2]], None, {(1, 0): [2, 1]}),
    }


@pytest.mark.gpu
def test_rows_prune_hand_made_cases(ctx):
    for tag, (glen, rows, nsets, pick_lists, fixed, answers) in _hand_made_cases().items():
        table = _table(rows)
        ftable = None if fixed is None else _table(fixed)
        R = _from_host(ctx, table, glen)
        F = None if fixed is None else _from_host(ctx, ftable, glen)
        try:
            for depth in (1, 2, 3):
                for j, picks in enumerate(pick_lists):
                    kept, removed = _check_prune(table, glen, nsets, picks, depth, R, ftable, F, tag)
                    if (depth, j) in answers:
                        assert removed == answers[(depth, j)], (tag, depth, picks, removed)
                    assert kept == [i for i in picks if i not in removed]
        finally:
            R.close()
            if F is not None:
                F.close()


@pytest.mark.gpu
def test_rows_prune_refusals(ctx):
    from catch_amd import engine
    R = _from_host(ctx, _table([(0, 0, 10, 50), (1, 0, 0, 5), (2, 1, 0, 9)]), [100, 50])
    held = [R]
    try:
        for picks, depth, what in (([0], 0, "smallest depth"), ([0], -3, "smallest depth"),
                                   ([3], 1, "outside the set ids"), ([-1], 1, "outside the set ids"),
                                   ([0, 1, 0], 1, "given twice"), ([0, 1, 2, 1], 2, "picks of 3 sets")):
            with pytest.raises(ValueError, match=what):
                R.prune(3, picks, depth)
        with pytest.raises(ValueError, match="smallest depth"):          # refused before "no picks" returns
            R.prune(3, [], 0)
        for glen in ([100, 51], [150], [100, 50, 1], [50, 100]):
            F = _from_host(ctx, _table([(0, 0, 1, 2)]), glen)
            held.append(F)
            with pytest.raises(ValueError, match="coordinate space"):
                R.prune(3, [0, 1], 1, F)
        other = engine.upload_context()
        F = _from_host(other, _table([(0, 0, 1, 2)]), [100, 50])
        held.append(F)
        with pytest.raises(ValueError, match="another context"):
            R.prune(3, [0, 1], 1, F)
        assert R.prune(3, [], 1) == ([], [])
        assert R.prune(3, [0, 1, 2], 1) == ([0, 1, 2], [])                # ... and the table serves the next call
        # rows of a scan with group numbers (a union of instances), as the rows and as the fixed table
        from catch_amd import probe
        rng = np.random.default_rng(8)
        genome = "".join(rng.choice(list("ACGT"), size=400))
        strs = [genome[j:j + 60] for j in range(0, 340, 20)]
        k, uniq, owner, ep, eo = probe.anchor_table(strs, 1, 60, min_k=20, k=20)
        made = []
        for grouped in (True, False):
            p, t = engine.Probes(ctx, uniq, owner, ep, eo, k), engine.Targets(ctx, [[genome], [genome[50:300]]])
            held += [p, t]
            if grouped:
                p.set_groups(np.zeros(len(uniq), dtype=np.int32))
                t.set_groups(np.zeros(2, dtype=np.int32))
            made.append(engine.Rows.scan(ctx, p, t, 1, 60, 0, 0))
            held.append(made[-1])
        grouped, plain = made
        with pytest.raises(ValueError, match="group numbers"):
            grouped.prune(len(strs), [0, 1], 1)
        with pytest.raises(ValueError, match="group numbers"):
            plain.prune(len(strs), [0, 1], 1, grouped)
        # ... and the plain scan's rows prune like a table from the host, beside unmerged ranges as the fixed table
        ranges = engine.Rows.scan(ctx, held[-3], held[-2], 1, 60, 0, 0, merge=False)
        held.append(ranges)
        glen, picks = [400, 250], list(range(len(strs)))
        assert plain.prune(len(strs), picks, 1) == tuple(_walk(plain.fetch(), glen, picks, 1)[:2])
        assert plain.prune(len(strs), picks, 2, ranges) == tuple(_walk(plain.fetch(), glen, picks, 2, ranges.fetch())[:2])
    finally:
        for h in reversed(held):
            h.close()


@pytest.mark.gpu
def test_rows_prune_equals_the_walk_on_the_360_combinations(ctx):
    """Both series (without and with the instance's fixed rows) through the C ABI, against the walk over Python
    sets."""
    combos = something = conflicts = 0
    at, held = None, ()
    try:
        for case, glen, nsets, rows, cov, depth, picks, plain, with_fixed, conflict in _walks_1213():
            if case != at:
                for h in held:
                    h.close()
                at, held = case, (_from_host(ctx, rows, glen), _from_host(ctx, cov, glen))
            R, F = held
            _check_prune(rows, glen, nsets, picks, depth, R, tag=case, want=plain)
            _check_prune(rows, glen, nsets, picks, depth, R, cov, F, tag=(case, "fixed"), want=with_fixed)
            combos += 1
            something += len(plain[1]) > 0
            conflicts += conflict
    finally:
        for h in held:
            h.close()
    assert combos == 360 and something >= 100 and conflicts >= 20


@pytest.mark.gpu
def test_rows_prune_random_tables(ctx):
    """Tables of a few thousand sets in up to 4 universes, all sets picked in a random order and 60 % of them, at
    depths 1 to 3, without and with a fixed table; the rounds are recorded."""
    rng = np.random.default_rng(2024)
    gone = 0
    for case in range(3):
        nsets, nuniv = int(rng.integers(2000, 4000)), int(rng.integers(1, 5))
        # rows of 100 to 160 bases every 2,000 or so: some tens of sets over every base
        rows, glen = _big_table(rng, nsets, nuniv, 4, 4000, 160)
        fixed, _ = _big_table(rng, 3, nuniv, 5, 3000, 400)
        keep = fixed[3] <= np.asarray(glen)[fixed[1]]
        fixed = tuple(a[keep] for a in fixed)
        R, F = _from_host(ctx, rows, glen), _from_host(ctx, fixed, glen)
        try:
            perm = [int(x) for x in rng.permutation(nsets)]
            for depth in (1, 2, 3):
                for picks in (perm, perm[:int(0.6 * nsets)]):
                    _k, removed = _check_prune(rows, glen, nsets, picks, depth, R, tag=case)
                    r0 = R.last_prune_rounds
                    _k, rf = _check_prune(rows, glen, nsets, picks, depth, R, fixed, F, tag=(case, "fixed"))
                    print("case %d: %d sets, %d rows, D = %d, %d picks: %d removed in %d rounds; with fixed rows %d "
                          "in %d" % (case, nsets, rows[0].size, depth, len(picks), len(removed), r0, len(rf),
                                     R.last_prune_rounds))
                    gone += len(removed)
                    assert len(rf) >= len(removed)
        finally:
            R.close()
            F.close()
    assert gone > 1000


@pytest.mark.gpu
def test_rows_prune_where_the_scan_takes_its_second_pass(ctx):
    """A few hundred rows in a coordinate space just above 2,097,152 bases, with rows on both sides of, across and
    ending at the edge of the scan's first tile of tile sums, and a row that ends at total."""
    edge = 2048 * 1024
    rng = np.random.default_rng(edge)
    total = edge + 700
    rows = []
    for i in range(40):
        starts = np.sort(rng.choice(total // 400 - 1, size=6, replace=False)) * 400
        rows += [(i, 0, int(s) + int(rng.integers(0, 100)), int(s) + int(rng.integers(150, 390))) for s in starts]
    near = [(40, edge - 300, edge), (40, edge + 1, edge + 300), (41, edge - 100, edge + 100),
            (42, edge - 1, edge + 1), (43, edge, edge + 64), (44, edge - 2048, edge + 690),
            (45, edge - 64, edge - 1), (46, edge - 200, edge + 650), (47, edge + 600, total),
            (48, 0, 3), (49, edge - 50, edge + 50), (50, 0, total), (51, edge + 500, total)]
    rows += [(i, 0, s, t) for i, s, t in near]
    rows.sort()
    table = _table(rows)
    R = _from_host(ctx, table, [total])
    try:
        gone = 0
        for depth in (1, 2, 3):
            for picks in (list(range(52)), list(range(51, -1, -1)), list(range(0, 40, 2)) + list(range(40, 52))):
                gone += len(_check_prune(table, [total], 52, picks, depth, R, tag=edge)[1])
        assert gone > 0
    finally:
        R.close()


@pytest.mark.gpu
def test_rows_prune_finishes_a_chain_of_conflicts_in_few_rounds(ctx):
    """300 staggered picks over a base layer: each is removable at the start and conflicts with the next one
    examined, so the round scheme alone removes one pick per round; the one-workgroup walk finishes the chain."""
    n = 300
    rows = [(i, 0, 100 * i, 100 * i + 150) for i in range(n)]           # i and i + 1 share [100 (i + 1), 100 i + 150)
    rows.append((n, 0, 0, 100))                                          # the base layer: every base but the overlaps
    rows += [(n, 0, 100 * i + 50, 100 * i + 100) for i in range(1, n - 1)]
    rows.append((n, 0, 100 * (n - 1) + 50, 100 * n + 50))
    total = 100 * n + 50
    table = _table(rows)
    picks = [n] + list(range(n))
    want = _walk(table, [total], picks, 1)[:2]
    assert want[1] == list(range(n - 1, -1, -2))                        # every other one, from the last
    model_rounds = _rounds(table, [total], picks, 1)[2]
    R = _from_host(ctx, table, [total])
    try:
        _check_prune(table, [total], n + 1, picks, 1, R, tag="chain", want=want)
        print("a chain of %d picks: %d removed; the round scheme alone takes %d rounds, the device took %d"
              % (n, len(want[1]), model_rounds, R.last_prune_rounds))
        assert model_rounds >= n // 2 and 1 <= R.last_prune_rounds < n // 10
        _check_prune(table, [total], n + 1, [n] + list(range(n - 1, -1, -1)), 1, R, tag="chain, reversed")
        assert R.last_prune_rounds < n // 10
    finally:
        R.close()


# ------------------------------------------------------------------ filter level
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_prunes_what_the_walk_prunes_on_five_genomes(ctx, oracle, e, depth):
    g5, c5 = _ebola5()
    glen = [g.size() for g in g5]
    rows = _oracle_rows(oracle, c5, g5, e)
    layers, _facts, _n = _oracle_depth_design(oracle, rows, len(c5), glen, depth, [1.0] * len(glen))
    picks = [int(i) for layer in layers for i in layer]
    kept, removed, before, after = _walk(rows, glen, picks, depth)
    f = _filter(e, coverage_depth=depth, prune_redundant=True)
    got = f._filter_strs([c5], [g5], assume_unique=True)
    t = f.last_timings
    print("e = %d, D = %d: %d picked, %d redundant; scan_ms %.3f greedy_ms %.3f prune_ms %.3f (%d launches, %d "
          "rounds)" % (e, depth, len(picks), len(removed), t["scan_ms"], t["greedy_ms"], t["prune_ms"],
                       t["prune_launches"], t["prune_rounds"]))
    assert got == [kept] and f.last_pruned == [removed]
    assert len(removed) >= 1
    assert f.last_layer_sizes == [[len(x) for x in layers]]
    assert t["pruned"] == len(removed) and t["picks"] == len(kept) and t["prune_ms"] > 0 and t["prune_rounds"] >= 1
    assert np.array_equal(np.minimum(before, depth), np.minimum(after, depth))
    # with the keyword off the result is today's
    off = _filter(e, coverage_depth=depth, prune_redundant=False)
    assert off._filter_strs([c5], [g5], assume_unique=True) == [picks]
    assert "prune_ms" not in off.last_timings and off.last_pruned in ([], [[]])
    if depth == 1:
        assert _filter(e)._filter_strs([c5], [g5], assume_unique=True) == [picks]


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_filter_prunes_at_partial_coverage_what_the_walk_prunes(ctx, oracle, e):
    g5, c5 = _ebola5()
    glen = [g.size() for g in g5]
    rows = _oracle_rows(oracle, c5, g5, e)
    picks = [int(i) for i in oracle.approx_multiuniverse(*rows, len(c5), len(glen), universe_p=[0.9] * len(glen))]
    kept, removed, _b, _a = _walk(rows, glen, picks, 1)
    f = _filter(e, 0.9, prune_redundant=True)
    assert f._filter_strs([c5], [g5], assume_unique=True) == [kept] and f.last_pruned == [removed]
    print("e = %d, coverage 0.9: %d picked, %d redundant" % (e, len(picks), len(removed)))


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_filter_prunes_the_extension_from_five_genomes_to_ten(ctx, oracle, e):
    g10, c10, _d10, d5 = _design(e)
    glen = [g.size() for g in g10]
    new, _nreduced = _oracle_extension(oracle, c10, d5, g10, e, 1.0)
    new = [int(i) for i in new]
    rows, cov = _oracle_rows(oracle, c10, g10, e), _oracle_rows(oracle, d5, g10, e)
    # the fixed probes are one set to the filter: their union counts once per base
    by_set, _off, total = _global_rows(cov, glen)
    union = np.zeros(total, dtype=bool)
    for rr in by_set.values():
        for a, b in rr:
            union[a:b] = True
    edge = np.diff(np.concatenate([[0], union.astype(np.int8), [0]]))
    off = np.concatenate([[0], np.cumsum(glen)])
    runs = [(int(a), int(b)) for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1))]
    merged = []
    for a, b in runs:                                   # (a run of the union may cross a universe boundary)
        u = int(np.searchsorted(off, a, side="right") - 1)
        while a < b:
            stop = min(b, int(off[u + 1]))
            merged.append((0, u, a - int(off[u]), stop - int(off[u])))
            a, u = stop, u + 1
    kept, removed, _b, _a = _walk(rows, glen, new, 1, _table(merged))
    f = _filter(e, fixed_probes=d5, prune_redundant=True)
    got = f._filter_strs([c10], [g10], assume_unique=True)
    print("e = %d: %d fixed probes, %d new, %d of them redundant; prune_ms %.3f"
          % (e, len(d5), len(new), len(removed), f.last_timings["prune_ms"]))
    assert got == [kept] and f.last_pruned == [removed] and f.last_layer_sizes == [[len(new)]]
    assert f.last_timings["pruned"] == len(removed) and f.last_timings["picks"] == len(kept)
    assert _filter(e, fixed_probes=d5)._filter_strs([c10], [g10], assume_unique=True) == [new]


# ------------------------------------------------------------------ command line
@pytest.mark.gpu
def test_design_prune_redundant_and_prune_probes_end_to_end(ctx, tmp_path, capsys):
    from catch_amd import design, prune_probes
    from catch_amd.utils import seq_io
    g5, c5 = _ebola5()
    f = _filter(0, prune_redundant=True)
    kept = f._filter_strs([c5], [g5], assume_unique=True)[0]
    removed = f.last_pruned[0]
    assert len(removed) >= 1
    fa = _write_fasta(tmp_path / "five.fasta", list(seq_io.read_fasta(EBOLA).items())[:5])
    plain, pruned = str(tmp_path / "plain.fasta"), str(tmp_path / "pruned.fasta")
    base = [fa, "-pl", "100", "-ps", "50", "-m", "2", "-e", "0"]
    capsys.readouterr()
    design.main(design.parse_args(base + ["-o", plain]))
    assert capsys.readouterr().out.split() == [str(len(kept) + len(removed))]
    design.main(design.parse_args(base + ["--prune-redundant", "-o", pruned]))
    assert capsys.readouterr().out.split() == [str(len(kept))]
    assert list(seq_io.iterate_fasta(pruned)) == [c5[i] for i in kept]
    designed = list(seq_io.iterate_fasta(plain))
    assert sorted(designed) == sorted(c5[i] for i in kept + removed)
    # prune_probes on the unpruned design: the records are the picks in pick order, so it drops the same probes
    out, gone, again = str(tmp_path / "kept.fasta"), str(tmp_path / "gone.fasta"), str(tmp_path / "again.fasta")
    argv = ["-d", fa, "-f", plain, "-m", "2", "-l", "100", "-e", "0"]
    prune_probes.main(prune_probes.parse_args(argv + ["-o", out, "--write-removed", gone]))
    assert capsys.readouterr().out.split() == [str(len(kept)), str(len(removed))]
    assert list(seq_io.iterate_fasta(out)) == [c5[i] for i in kept]
    assert list(seq_io.iterate_fasta(gone)) == [c5[i] for i in removed]
    # ... on its own output it removes nothing
    prune_probes.main(prune_probes.parse_args(["-d", fa, "-f", out, "-m", "2", "-l", "100", "-e", "0", "-o", again]))
    assert capsys.readouterr().out.split() == [str(len(kept)), "0"]
    assert open(again).read() == open(out).read()
    # ... and of a list that holds every probe twice, the second copies go first
    twice = str(tmp_path / "twice.fasta")
    with open(twice, "w") as fh:
        for j, s in enumerate(list(seq_io.iterate_fasta(out)) * 2):
            fh.write(">p%d\n%s\n" % (j, s))
    prune_probes.main(prune_probes.parse_args(["-d", fa, "-f", twice, "-m", "2", "-l", "100", "-e", "0", "-o", again]))
    assert capsys.readouterr().out.split() == [str(len(kept)), str(len(kept))]
    assert open(again).read() == open(out).read()
