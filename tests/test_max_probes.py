"""--max-probes / SetCoverFilter(max_probes=N, pick_gains=True): the gain of every pick (the bases it covered first,
catchhip_rows_pick_gains), the coverage curve, and the budget allocation over datasets (allocate_budget).

The reference has no counterpart.  The kernel is checked against a NumPy model of first(b), the gains and the
curve, the model against a walk over Python sets, and the device against the independent checker
(catchhip_rows_cover_check), the oracle's greedy on concatenated instances and the oracle's rows of Ebola genomes.
"""
import heapq
import inspect
import os
import re

import numpy as np
import pytest

from test_coverage_depth import _ebola5, _filter
from test_extend_probes import (EBOLA, REPO, _big_table, _candidates, _design, _from_host, _instance, _np_subtract,
                                _oracle_extension, _oracle_rows, _table, _union_len, _write_fasta)

NONE = np.iinfo(np.int64).max


# ------------------------------------------------------------------ host models
def _first(rows, glen, picks):
    """first[b] over the concatenated universes: the smallest position in `picks` of a set with a row over b."""
    off = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
    first = np.full(int(off[-1]), NONE, dtype=np.int64)
    rank = {int(s): i for i, s in enumerate(picks)}
    for s, u, a, b in zip(*rows):
        r = rank.get(int(s))
        if r is not None:
            seg = first[off[u] + a:off[u] + b]
            np.minimum(seg, r, out=seg)
    return first, off


def _worst(cov, denom):
    """(universe, its cov) with the smallest cov / denom among denom > 0, exact, ties to the lower one; (-1, 0)."""
    best = -1
    for u, (c, d) in enumerate(zip(cov, denom)):
        if d > 0 and (best < 0 or int(c) * int(denom[best]) < int(cov[best]) * int(d)):
            best = u
    return (best, int(cov[best])) if best >= 0 else (-1, 0)


def _model(rows, glen, picks, checkpoints=(), denom=None, covered0=None):
    """(gains, [(covered_total, worst_universe, worst_covered) per checkpoint])."""
    first, off = _first(rows, glen, picks)
    gains = np.bincount(first[first != NONE], minlength=len(picks)).astype(np.int64)[:len(picks)]
    c0 = [0] * len(glen) if covered0 is None else covered0
    curve = []
    for k in checkpoints:
        cov = [int(c0[u]) + int(np.count_nonzero(first[off[u]:off[u + 1]] < k)) for u in range(len(glen))]
        curve.append((sum(cov),) + _worst(cov, denom))
    return gains, curve


def _walk_sets(sets, nuniv, picks, checkpoints=(), denom=None, covered0=None):
    """The same from the definition: the picks taken one after the other over Python sets (sets[i] = {u: set})."""
    covered = [set() for _ in range(nuniv)]
    c0 = [0] * nuniv if covered0 is None else covered0
    gains, curve = [], []
    for i, s in enumerate(picks):
        new = 0
        for u, elems in sets[s].items():
            new += len(elems - covered[u])
            covered[u] |= elems
        gains.append(new)
        if i + 1 in checkpoints:
            cov = [int(c0[u]) + len(covered[u]) for u in range(nuniv)]
            curve.append((sum(cov),) + _worst(cov, denom))
    return np.array(gains, dtype=np.int64), curve


def _random_call(rng, nsets, nuniv, glen):
    """A random subset of the sets in a random order, random checkpoints, denominators (some 0) and covered0."""
    picks = [int(x) for x in rng.permutation(nsets)[:int(rng.integers(1, nsets + 1))]]
    n = len(picks)
    ck = sorted(int(x) for x in rng.choice(np.arange(1, n + 1), size=int(rng.integers(0, n + 1)), replace=False))
    denom = [int(rng.integers(1, 2 * g + 2)) if rng.random() < 0.8 else 0 for g in glen]
    covered0 = None if rng.random() < 0.3 else [int(rng.integers(0, g + 1)) for g in glen]
    return picks, ck, denom, covered0


def _merge(gains_per_group):
    """The merged order as (group, position) pairs: the largest next gain first, the earlier group among equals."""
    heap = [(-int(g[0]), gi) for gi, g in enumerate(gains_per_group) if len(g)]
    heapq.heapify(heap)
    at, out = [0] * len(gains_per_group), []
    while heap:
        _neg, gi = heapq.heappop(heap)
        out.append((gi, at[gi]))
        at[gi] += 1
        if at[gi] < len(gains_per_group[gi]):
            heapq.heappush(heap, (-int(gains_per_group[gi][at[gi]]), gi))
    return out


# ------------------------------------------------------------------ without a GPU
def test_symbol_is_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bint catchhip_rows_pick_gains\s*\(", hdr)
    assert "catchhip_rows_pick_gains" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["catchhip_rows_pick_gains"][1]) == 13
    assert callable(engine.Rows.pick_gains)
    sig = inspect.signature(engine.Rows.pick_gains).parameters
    assert list(sig) == ["self", "num_sets", "picks", "checkpoints", "denom", "covered0"]
    assert all(sig[name].default is None for name in ("checkpoints", "denom", "covered0"))
    mk = open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert "gains.hip" in mk
    assert "#define CATCHHIP_ABI_VERSION 2\n" in hdr
    src = open(os.path.join(REPO, "catch_amd", "csrc", "gains.hip")).read()
    assert '#include "wave.h"' in src and "find_segment" in src and "chip_depth_marks" in src
    assert "double" not in src and "float" not in src                    # integer arithmetic only


def test_filter_keeps_the_reference_signature_and_takes_the_three_keywords():
    from catch_amd.filter import set_cover_filter as scf
    names = list(inspect.signature(scf.SetCoverFilter.__init__).parameters)
    assert names[-2:] == ["kmer_probe_map_use_native_dict", "fixed_probes"]
    call = inspect.signature(scf.SetCoverFilter).parameters
    for name, default in (("max_probes", None), ("pick_gains", False), ("curve_points", 100)):
        assert call[name].kind is inspect.Parameter.KEYWORD_ONLY and call[name].default == default
    f = scf.SetCoverFilter(2, 100)
    assert f.max_probes is None and f.pick_gains is False and f.curve_points == 100
    assert f.last_pick_gains == [] and f.last_budget_kept == [] and f.last_coverage_curve == []
    f = scf.SetCoverFilter(2, 100, 0, None, None, None, None, None, False, [], 1.0, 0, 20, False, None,
                           max_probes=7, curve_points=3)
    assert f.max_probes == 7 and f.pick_gains is True and f.curve_points == 3     # max_probes implies pick_gains
    assert scf.SetCoverFilter(2, 100, pick_gains=True).max_probes is None
    assert scf.SetCoverFilter(2, 100, max_probes=5, prune_redundant=True, fixed_probes=["ACGT" * 25]).pick_gains
    for kw in (dict(max_probes=0), dict(max_probes=-1), dict(max_probes=True), dict(max_probes=2.5),
               dict(pick_gains=1), dict(curve_points=0), dict(curve_points=None)):
        with pytest.raises(ValueError):
            scf.SetCoverFilter(2, 100, **kw)
    for kw in (dict(max_probes=5), dict(pick_gains=True)):
        with pytest.raises(NotImplementedError, match="coverage_depth"):
            scf.SetCoverFilter(2, 100, coverage_depth=2, **kw)


def test_front_end_stays_on_the_host_with_pick_gains():
    from catch_amd.filter import probe_designer, set_cover_filter as scf
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for kw, want in ((dict(), "per group"), (dict(pick_gains=True), None), (dict(max_probes=3), None)):
        f = scf.SetCoverFilter(2, 100, **kw)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == want


def test_allocate_budget():
    from catch_amd.filter.set_cover_filter import allocate_budget
    # a tie goes to the earlier group
    assert allocate_budget([[5, 3], [5, 4]], 1) == [1, 0]
    assert allocate_budget([[5, 3], [5, 4]], 2) == [1, 1]
    assert allocate_budget([[5, 3], [5, 4]], 3) == [1, 2]
    assert allocate_budget([[4, 4, 4], [4, 4]], 4) == [3, 1]
    # N at and above the sum of the picks keeps everything
    assert allocate_budget([[5, 3], [5, 4]], 4) == [2, 2]
    assert allocate_budget([[5, 3], [5, 4]], 1000) == [2, 2]
    # a group with no picks, and no groups
    assert allocate_budget([[], [2, 1], []], 1) == [0, 1, 0]
    assert allocate_budget([[], []], 3) == [0, 0]
    assert allocate_budget([], 3) == []
    # a sequence that is not monotone still keeps a prefix: the 9 is reached only through the 1 before it
    assert allocate_budget([[1, 9], [2]], 1) == [0, 1]
    assert allocate_budget([[1, 9], [2]], 2) == [1, 1]
    assert allocate_budget([[3, 1, 9], [2, 2]], 4) == [2, 2]
    # trailing picks with gain 0 are kept only if the budget reaches them
    assert allocate_budget([[3, 0, 0], [2, 0]], 2) == [1, 1]
    assert allocate_budget([[3, 0, 0], [2, 0]], 3) == [2, 1]
    assert allocate_budget([[3, 0, 0], [2, 0]], 5) == [3, 2]
    assert allocate_budget([np.array([3, 1], dtype=np.uint32), np.array([2], dtype=np.uint32)], np.int64(2)) == [1, 1]
    for bad in (0, -4, 1.5, None, True):
        with pytest.raises(ValueError):
            allocate_budget([[1]], bad)
    # named picks: a name the merge has taken already is kept without counting
    assert allocate_budget([[5, 3], [4, 2]], 2, [["a", "b"], ["a", "c"]]) == [2, 1]
    assert allocate_budget([[5, 3], [4, 2]], 3, [["a", "b"], ["a", "c"]]) == [2, 2]
    assert allocate_budget([[5, 3], [4, 2]], 3, [["a", "b"], ["c", "d"]]) == [2, 1]
    assert allocate_budget([[5, 3], [4, 2]], 1, [["a", "b"], ["a", "c"]]) == [1, 0]
    assert allocate_budget([[5, 3], [4, 2]], 9, [["a", "b"], ["b", "a"]]) == [2, 2]
    # against the merged order, on random sequences
    rng = np.random.default_rng(5)
    for _ in range(200):
        gains = [[int(x) for x in rng.integers(0, 6, size=int(rng.integers(0, 7)))] for _ in range(int(rng.integers(1, 5)))]
        order = _merge(gains)
        for n in range(1, len(order) + 2):
            want = [0] * len(gains)
            for gi, _pos in order[:n]:
                want[gi] += 1
            assert allocate_budget(gains, n) == want


def test_curve_checkpoints():
    from catch_amd.filter.set_cover_filter import curve_checkpoints
    assert curve_checkpoints(7, 3) == [3, 5, 7]
    assert curve_checkpoints(3, 100) == [1, 2, 3]
    assert curve_checkpoints(1, 1) == [1]
    assert curve_checkpoints(331, 1) == [331]
    assert curve_checkpoints(10, 2, extra=[4, 0, 11]) == [4, 5, 10]
    for n, p in ((331, 100), (1000, 7), (5, 5), (99, 100)):
        ks = curve_checkpoints(n, p)
        assert ks == sorted(set(ks)) and ks[-1] == n and ks[0] >= 1 and len(ks) <= p


def test_command_line_refusals(tmp_path):
    from catch_amd import analyze_probe_coverage, design, design_grid, pool, prune_probes
    fa = tmp_path / "t.fasta"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    probes = tmp_path / "p.fasta"
    probes.write_text(">p\n" + "ACGT" * 25 + "\n")
    out = str(tmp_path / "o.fasta")
    base = [str(fa), "-o", out, "--max-probes", "10"]
    args = design.parse_args([str(fa)])
    assert args.max_probes is None and args.write_coverage_curve is None and args.coverage_curve_points == 100
    assert design.parse_args(base).max_probes == 10
    assert design.parse_args(base, args_type="large").max_probes == 10
    with pytest.raises(Exception, match="--max-probes with --skip-set-cover"):
        design.main(design.parse_args(base + ["--skip-set-cover"]))
    with pytest.raises(Exception, match="--max-probes with --cluster-and-design-separately"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0.1"]))
    with pytest.raises(Exception, match="a default of design_large.py"):                          # design_large
        design.main(design.parse_args(base, args_type="large"))
    with pytest.raises(Exception, match="--max-probes with --cluster-from-fragments"):
        design.main(design.parse_args(base + ["--cluster-and-design-separately", "0"], args_type="large"))
    with pytest.raises(Exception, match="--max-probes with --coverage-depth above 1"):
        design.main(design.parse_args(base + ["--coverage-depth", "2"]))
    for n in ("0", "-3"):
        with pytest.raises(Exception, match="--max-probes must be at least 1"):
            design.main(design.parse_args([str(fa), "-o", out, "--max-probes", n]))
    with pytest.raises(Exception, match="--coverage-curve-points must be at least 1"):
        design.main(design.parse_args(base + ["--coverage-curve-points", "0"]))
    # the curve alone asks for the gains too
    curve = ["--write-coverage-curve", str(tmp_path / "curve.tsv")]
    with pytest.raises(Exception, match="--write-coverage-curve with --skip-set-cover"):
        design.main(design.parse_args([str(fa), "-o", out] + curve + ["--skip-set-cover"]))
    with pytest.raises(Exception, match="--write-coverage-curve with --coverage-depth above 1"):
        design.main(design.parse_args([str(fa), "-o", out] + curve + ["--coverage-depth", "3"]))
    # allowed beside these: what the messages advise parses
    args = design.parse_args(base + curve + ["--cluster-and-design-separately", "0", "--cluster-from-fragments", "0",
                                             "--prune-redundant", "--extend-probes", str(probes), "-c", "0.9",
                                             "--identify", "--avoid-genomes", str(fa), "--coverage-curve-points", "7"],
                             args_type="large")
    assert args.max_probes == 10 and args.coverage_curve_points == 7 and not args.cluster_and_design_separately
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "curve.tsv"))
    # the other commands do not know the options
    for parse, argv in ((design_grid.parse_args, [str(fa), "--grid-mismatches", "0", "--grid-cover-extension", "0",
                                                  "-o", str(tmp_path / "grid")]),
                        (pool._parser().parse_args, ["counts.tsv", "100", "params.tsv"]),
                        (analyze_probe_coverage.parse_args, ["-d", str(fa), "-f", str(probes), "-m", "0", "-l", "100"]),
                        (prune_probes.parse_args, ["-d", str(fa), "-f", str(probes), "-o", out])):
        parse(argv)
        for opt in (["--max-probes", "5"], ["--write-coverage-curve", "c.tsv"], ["--coverage-curve-points", "5"]):
            with pytest.raises(SystemExit):
                parse(argv + opt)


def test_help_says_when_the_budget_is_the_global_greedy(capsys):
    from catch_amd import design
    with pytest.raises(SystemExit):
        design.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--max-probes" in text and "--write-coverage-curve" in text and "--coverage-curve-points" in text
    assert "maximum coverage over all datasets together" in text and "otherwise a prefix rule" in text


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel
    from catch_amd.filter import set_cover_filter as scf

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    for kw in (dict(max_probes=3), dict(pick_gains=True), dict(max_probes=3, fixed_probes=["ACGT" * 25]),
               dict(max_probes=3, prune_redundant=True)):
        f = scf.SetCoverFilter(2, 100, **kw)
        with pytest.raises(NotImplementedError):
            f._filter_strs([["ACGT" * 25]], [[]])


def test_model_agrees_with_the_walk_over_python_sets():
    rng = np.random.default_rng(1213)
    shadowed = with_curve = 0
    for case in range(300):
        glen, nsets, rows, _cov, sets, _fixed = _instance(rng)
        picks, ck, denom, covered0 = _random_call(rng, nsets, len(glen), glen)
        gains, curve = _model(rows, glen, picks, ck, denom, covered0)
        want_gains, want_curve = _walk_sets(sets, len(glen), picks, ck, denom, covered0)
        assert np.array_equal(gains, want_gains), case
        assert curve == want_curve, case
        shadowed += int(np.count_nonzero(gains == 0))
        with_curve += len(curve) > 0
    assert shadowed >= 100 and with_curve >= 200


def _pair(seed):
    """Two random instances and their concatenation (B's set ids and universes after A's)."""
    rng = np.random.default_rng(seed)
    a, b = _instance(rng), _instance(rng)
    (ga, na, ra), (gb, nb, rb) = a[:3], b[:3]
    both = (np.concatenate([ra[0], rb[0] + na]).astype(np.int32), np.concatenate([ra[1], rb[1] + len(ga)]).astype(np.int32),
            np.concatenate([ra[2], rb[2]]), np.concatenate([ra[3], rb[3]]))
    return (ga, na, ra), (gb, nb, rb), (ga + gb, na + nb, both)


def _pairs_without_cross_tie(oracle, seeds):
    """[(seed, A, B, the oracle's picks of A, of B, of the concatenation)] where no gain of A's sequence equals
    one of B's: across instances the greedy's rule among equal gains is not the lowest id."""
    out = []
    for seed in seeds:
        A, B, C = _pair(seed)
        pa, pb, pc = ([int(x) for x in oracle.approx_multiuniverse(*t[2], t[1], len(t[0]))] for t in (A, B, C))
        ga, gb = _model(A[2], A[0], pa)[0], _model(B[2], B[0], pb)[0]
        if set(ga.tolist()) & set(gb.tolist()):
            continue
        out.append((seed, A, B, pa, pb, pc))
    return out


def test_enough_pairs_of_instances_have_no_cross_tie(oracle):
    """... and on them the merge by the model's gains is the oracle's greedy on the concatenated instance."""
    from catch_amd.filter.set_cover_filter import allocate_budget
    pairs = _pairs_without_cross_tie(oracle, range(200))
    assert len(pairs) >= 30, len(pairs)
    for seed, A, B, pa, pb, pc in pairs:
        gains = [_model(A[2], A[0], pa)[0], _model(B[2], B[0], pb)[0]]
        assert len(pc) == len(pa) + len(pb)
        for n in range(1, len(pc) + 1):
            ka, kb = allocate_budget(gains, n)
            assert sorted(pc[:n]) == sorted(pa[:ka] + [A[1] + s for s in pb[:kb]]), (seed, n)


# ------------------------------------------------------------------ kernel
def _check(R, rows, glen, nsets, picks, ck=(), denom=None, covered0=None, tag=None):
    """The device against the model; returns the gains."""
    want_gains, want_curve = _model(rows, glen, picks, ck, denom, covered0)
    gains, tot, wu, wc = R.pick_gains(nsets, picks, list(ck) or None, denom, covered0)
    assert gains.dtype == np.uint32 and gains.shape == (len(picks),), tag
    assert np.array_equal(gains.astype(np.int64), want_gains), (tag, "gains")
    if len(ck) == 0:
        assert tot is None and wu is None and wc is None, tag
    else:
        got = [(int(t), int(u), int(c)) for t, u, c in zip(tot, wu, wc)]
        assert got == want_curve, (tag, "curve")
    return gains


def _hand_made_cases():
    """(name, rows, glen, nsets, picks, gains to expect or None)."""
    cases = []
    # a later pick wholly shadowed by an earlier one
    cases.append(("shadowed", [(0, 0, 0, 100), (1, 0, 10, 50), (2, 0, 90, 120)], [130], 3, [0, 1, 2], [100, 0, 20]))
    cases.append(("shadowed, the other way", [(0, 0, 0, 100), (1, 0, 10, 50)], [130], 2, [1, 0], [40, 60]))
    # base 7 under five picks listed in descending set id: the rank decides, not the id
    cases.append(("five over one base", [(i, 0, i, i + 8) for i in range(5)], [12], 5, [4, 3, 2, 1, 0], [8, 1, 1, 1, 1]))
    # rows of 1, 63, 64, 65 and 129 bases starting at offsets 0, 1 and 63 of a 64-base line; a set over everything
    # picked in the middle shadows the later ones, and its row ends at the last base of the coordinate space
    rows, at = [], 0
    for ln in (1, 63, 64, 65, 129):
        for o in (0, 1, 63):
            rows.append((len(rows), 0, at + o, at + o + ln))
            at += 256
    total = at
    rows.append((15, 0, 0, total))
    lens = [b - a for _s, _u, a, b in rows[:15]]
    order = [3, 14, 0, 7, 9, 12, 1, 15, 2, 4, 5, 6, 8, 10, 11, 13]
    want = [lens[s] for s in order[:7]] + [total - sum(lens[s] for s in order[:7])] + [0] * 8
    cases.append(("lengths and offsets", rows, [total], 16, order, want))
    cases.append(("lengths and offsets, in order", rows, [total], 16, list(range(15)), lens))
    # rows that end at the last base of their universe and of the space; a pick without rows (set 3), an unpicked set
    cases.append(("ends and empties", [(0, 0, 5, 10), (0, 1, 0, 7), (1, 1, 6, 7), (2, 2, 0, 3), (4, 2, 0, 3)],
                  [10, 7, 3], 6, [3, 1, 0, 2, 5], [0, 1, 11, 3, 0]))
    cases.append(("one base", [(0, 0, 0, 1)], [1], 1, [0], [1]))
    cases.append(("no rows at all", [], [4, 4], 3, [2, 0], [0, 0]))
    return cases


@pytest.mark.gpu
def test_rows_pick_gains_hand_made_cases(ctx):
    for name, rows, glen, nsets, picks, want in _hand_made_cases():
        table = _table(sorted(rows))
        R = _from_host(ctx, table, glen)
        try:
            n = len(picks)
            denom = [g + 1 for g in glen]
            for ck in ((), (1,), (n,), tuple(range(1, n + 1))):
                gains = _check(R, table, glen, nsets, picks, ck, denom if ck else None, None, tag=(name, ck))
                assert gains.tolist() == want, name
            _check(R, table, glen, nsets, picks, (n,), denom, [1] * len(glen), tag=(name, "covered0"))
        finally:
            R.close()


@pytest.mark.gpu
def test_rows_pick_gains_worst_universe_rules(ctx):
    # universe 0: 5 of 10, universe 1: 10 of 20, universe 2: 3 of 4 after both picks
    table = _table([(0, 0, 0, 5), (0, 1, 0, 4), (1, 1, 4, 10), (1, 2, 0, 3)])
    glen = [10, 20, 4]
    R = _from_host(ctx, table, glen)
    try:
        def call(ck, denom, covered0=None):
            _g, tot, wu, wc = R.pick_gains(2, [0, 1], ck, denom, covered0)
            _check(R, table, glen, 2, [0, 1], ck, denom, covered0)
            return [(int(t), int(u), int(c)) for t, u, c in zip(tot, wu, wc)]
        # a tie (5 / 10 == 10 / 20, exactly) goes to the lower universe
        assert call([2], [10, 20, 4]) == [(18, 0, 5)]
        assert call([2], [10, 20, 3]) == [(18, 0, 5)]
        assert call([2], [10, 21, 4]) == [(18, 1, 10)]
        assert call([2], [11, 20, 4]) == [(18, 0, 5)]
        # after one pick: 5 / 10, 4 / 20, 0 / 4
        assert call([1, 2], [10, 20, 4]) == [(9, 2, 0), (18, 0, 5)]
        # a universe with denom 0 is skipped; all zero gives -1
        assert call([1, 2], [10, 20, 0]) == [(9, 1, 4), (18, 0, 5)]
        assert call([2], [0, 0, 4]) == [(18, 2, 3)]
        assert call([1, 2], [0, 0, 0]) == [(9, -1, 0), (18, -1, 0)]
        # covered0 changes which universe is worst: 6 / 10 against 10 / 20
        assert call([2], [10, 20, 4], [1, 0, 0]) == [(19, 1, 10)]
        assert call([2], [10, 20, 4], [0, 0, 1]) == [(19, 0, 5)]
        assert call([1], [10, 20, 4], [0, 0, 3]) == [(12, 1, 4)]
        # factors near 2^32: the comparison is exact in 64 bits
        big = 2 ** 32 - 1
        assert call([2], [big, big - 1, big]) == [(18, 2, 3)]
        assert call([2], [big, big, 4]) == [(18, 0, 5)]
    finally:
        R.close()


@pytest.mark.gpu
def test_rows_pick_gains_refusals(ctx, monkeypatch):
    from catch_amd import engine, probe
    R = _from_host(ctx, _table([(0, 0, 10, 50), (1, 0, 0, 5), (2, 1, 0, 9)]), [100, 50])
    held = [R]
    try:
        for picks, what in (([3], "outside the set ids"), ([-1], "outside the set ids"), ([0, 1, 0], "given twice"),
                            ([0, 1, 2, 1], "picks of 3 sets")):
            with pytest.raises(ValueError, match="rows_pick_gains: .*" + what):
                R.pick_gains(3, picks)
        for ck, what in (([0], "outside 1 .. 3 picks"), ([4], "outside 1 .. 3 picks"), ([1, 4], "outside 1 .. 3 picks"),
                         ([2, 2], "not strictly ascending"), ([3, 1], "not strictly ascending")):
            with pytest.raises(ValueError, match="rows_pick_gains: .*" + what):
                R.pick_gains(3, [0, 1, 2], ck, [100, 50])
        with pytest.raises(ValueError, match="rows_pick_gains: 1 checkpoints of an empty pick list"):
            R.pick_gains(3, [], [1], [100, 50])
        for denom, c0 in (([-1, 5], None), ([2 ** 32, 5], None), ([5, 5], [-1, 0]), ([5, 5], [0, 2 ** 32 - 50])):
            with pytest.raises(ValueError, match="do not fit 32 bits"):
                R.pick_gains(3, [0], [1], denom, c0)
        with pytest.raises(ValueError, match="one value per universe"):
            R.pick_gains(3, [0], [1], [100])
        with pytest.raises(ValueError, match="need denom"):
            R.pick_gains(3, [0], [1])
        # no picks: at once; and the table serves the next call
        g, tot, wu, wc = R.pick_gains(3, [])
        assert g.size == 0 and tot is None and wu is None and wc is None
        assert R.pick_gains(3, [2, 0, 1])[0].tolist() == [9, 40, 5]
        # checkpoints x universes at 2^31: refused by the library, split by the wrapper
        many = engine.Rows.from_host(ctx, [], [], [], [], [1] * 32768)
        held.append(many)
        picks, ones = np.arange(65536), [1] * 32768
        monkeypatch.setattr(engine.Rows, "PICK_GAINS_TABLE_LIMIT", 1 << 40)
        with pytest.raises(ValueError, match="split the checkpoints"):
            many.pick_gains(65536, picks, np.arange(1, 65537), ones)
        monkeypatch.setattr(engine.Rows, "PICK_GAINS_TABLE_LIMIT", 9)       # 4 checkpoints of 2 universes per call
        ck = [1, 2, 3]
        whole = _model(_table([(0, 0, 10, 50), (1, 0, 0, 5), (2, 1, 0, 9)]), [100, 50], [2, 0, 1], ck, [100, 50])
        for limit, calls in ((9, 1), (5, 2), (3, 3), (1 << 31, 1)):
            monkeypatch.setattr(engine.Rows, "PICK_GAINS_TABLE_LIMIT", limit)
            g, tot, wu, wc = R.pick_gains(3, [2, 0, 1], ck, [100, 50])
            assert g.tolist() == whole[0].tolist()
            assert [(int(t), int(u), int(c)) for t, u, c in zip(tot, wu, wc)] == whole[1]
            # the time and the launches of every library call count (5 launches each with checkpoints: the pick table,
            # first, count, prefix, reduce)
            assert R.last_gains_launches == 5 * calls and R.last_gains_ms > 0
        R.pick_gains(3, [2, 0, 1])
        assert R.last_gains_launches == 3
        R.pick_gains(3, [])
        assert R.last_gains_launches == 0 and R.last_gains_ms == 0.0
        # rows of a scan with group numbers (a union of instances)
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
        with pytest.raises(ValueError, match="rows_pick_gains: .*group numbers"):
            grouped.pick_gains(len(strs), [0, 1])
        # ... and the plain scan's rows serve like a table from the host
        picks = list(range(len(strs) - 1, -1, -1))
        _check(plain, plain.fetch(), [400, 250], len(strs), picks, (1, len(picks)), [400, 250], tag="scan")
    finally:
        for h in reversed(held):
            h.close()


@pytest.mark.gpu
def test_rows_pick_gains_random_tables_and_the_independent_checker(ctx):
    rng = np.random.default_rng(4242)
    zero = curves = 0
    for case in range(300):
        glen, nsets, rows, _cov, _sets, _fixed = _instance(rng, max_sets=20, max_len=300)
        picks, ck, denom, covered0 = _random_call(rng, nsets, len(glen), glen)
        R = _from_host(ctx, rows, glen)
        try:
            gains = _check(R, rows, glen, nsets, picks, ck, denom, covered0, tag=case)
            chk = R.cover_check(nsets, picks)
            assert int(gains.sum()) == chk["covered_bases"] and chk["bad_pick_ids"] == 0, (case, chk)
            assert int(np.count_nonzero(gains == 0)) == chk["picks_without_gain"], (case, chk)
        finally:
            R.close()
        zero += int(np.count_nonzero(gains == 0))
        curves += len(ck)
    assert zero >= 100 and curves >= 500


_large = {}


def _large_table():
    """About 300 sets x 6 universes x 40 rows of up to 300 bases, every set picked, in shuffled order."""
    if not _large:
        rng = np.random.default_rng(300640)
        rows, glen = _big_table(rng, 300, 6, 40, 120, 300)
        picks = [int(x) for x in rng.permutation(300)]
        _large.update(rows=rows, glen=glen, picks=picks, ck=list(range(1, 301, 7)) + [300])
        _large["model"] = _model(rows, glen, picks, _large["ck"], glen)
    return _large


@pytest.mark.gpu
def test_rows_pick_gains_large_table(ctx):
    import time
    t = _large_table()
    rows, glen, picks, ck = t["rows"], t["glen"], t["picks"], t["ck"]
    assert 65_000 < rows[0].size <= 72_000 and (rows[3] - rows[2]).max() > 256 and len(picks) > 256
    want_gains, want_curve = t["model"]
    R = _from_host(ctx, rows, glen)
    try:
        gains, tot, wu, wc = R.pick_gains(300, picks, ck, glen)
        assert np.array_equal(gains.astype(np.int64), want_gains)
        assert [(int(a), int(b), int(c)) for a, b, c in zip(tot, wu, wc)] == want_curve
        chk = R.cover_check(300, picks)
        assert int(gains.sum()) == chk["covered_bases"] == int(_union_len(rows, len(glen)).sum())
        assert int(np.count_nonzero(gains == 0)) == chk["picks_without_gain"]
        # the order of the atomics is the hardware's: the same again, with and without checkpoints
        ms = []
        for rep in range(5):
            t0 = time.perf_counter()
            again = R.pick_gains(300, picks, ck if rep % 2 == 0 else None, glen if rep % 2 == 0 else None)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(again[0], gains)
        dev_ms, launches = ctx.kernel_ms(1)
        print("large table: %d rows, %d picked-row bases over %d bases, %d checkpoints: device %.3f ms in %d launches; "
              "host wall per call %s ms" % (rows[0].size, int((rows[3] - rows[2]).sum()), sum(glen), len(ck), dev_ms,
                                            launches, " ".join("%.3f" % x for x in ms)))
    finally:
        R.close()


# ------------------------------------------------------------------ merge equals the greedy over all datasets
@pytest.mark.gpu
def test_merge_by_device_gains_is_the_greedy_on_the_concatenated_instance(ctx, oracle):
    from catch_amd.filter.set_cover_filter import allocate_budget
    pairs = _pairs_without_cross_tie(oracle, range(200))
    assert len(pairs) >= 30, len(pairs)
    for seed, A, B, pa, pb, pc in pairs:
        gains, picked = [], []
        for glen, nsets, rows in (A, B):
            R = _from_host(ctx, rows, glen)
            try:
                picks = R.greedy(nsets)
                gains.append(R.pick_gains(nsets, picks)[0])
                picked.append([int(x) for x in picks])
            finally:
                R.close()
        assert picked == [pa, pb], seed
        for g in gains:
            assert np.all(np.diff(g.astype(np.int64)) <= 0) and np.all(g > 0), seed
        shifted = [pa, [A[1] + s for s in pb]]
        at = [0, 0]
        for n in range(1, len(pc) + 1):
            kept = allocate_budget(gains, n)
            step = [k - a for k, a in zip(kept, at)]
            assert sorted(step) == [0, 1], (seed, n)
            gi = step.index(1)
            assert shifted[gi][at[gi]] == pc[n - 1], (seed, n)          # the n-th pick of the greedy over both
            at = kept
        assert allocate_budget(gains, len(pc) + 5) == [len(pa), len(pb)]


# ------------------------------------------------------------------ filter level
@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_reports_the_gains_of_its_picks_on_five_genomes(ctx, oracle, e, coverage):
    g5, c5 = _ebola5()
    glen = [g.size() for g in g5]
    rows = _oracle_rows(oracle, c5, g5, e)
    up = None if coverage == 1.0 else [coverage] * len(glen)
    picks = [int(i) for i in oracle.approx_multiuniverse(*rows, len(c5), len(glen), universe_p=up)]
    union = _union_len(rows, len(glen))
    f = _filter(e, coverage, pick_gains=True, curve_points=10)
    assert f._filter_strs([c5], [g5], assume_unique=True) == [picks]
    ck = [row[0] for row in f.last_coverage_curve[0]]
    want_gains, want_curve = _model(rows, glen, picks, ck, union)
    gains = f.last_pick_gains[0]
    assert gains.dtype == np.uint32 and np.array_equal(gains.astype(np.int64), want_gains)
    assert ck[-1] == len(picks) and 2 <= len(ck) <= 10 and f.last_budget_kept == [len(picks)]
    coverable = int(union.sum())
    assert f.last_coverage_curve[0] == [(k, t, coverable, u, c, int(union[u]))
                                        for k, (t, u, c) in zip(ck, want_curve)]
    t = f.last_timings
    print("e = %d, coverage %g: %d picks, gains %d .. %d; scan_ms %.3f greedy_ms %.3f gains_ms %.3f (%d launches)"
          % (e, coverage, len(picks), int(gains[0]), int(gains[-1]), t["scan_ms"], t["greedy_ms"], t["gains_ms"],
             t["gains_launches"]))
    assert t["gains_ms"] > 0 and t["gains_launches"] >= 5 and t["picks"] == len(picks)
    if coverage == 1.0:
        assert np.all(np.diff(gains.astype(np.int64)) <= 0) and int(gains.sum()) == coverable
        assert f.last_coverage_curve[0][-1][1] == coverable
        # with the keywords off the result is today's, and nothing is measured
        off = _filter(e)
        assert off._filter_strs([c5], [g5], assume_unique=True) == [picks] and "gains_ms" not in off.last_timings
        # a budget keeps a prefix and measures the cut
        cut = _filter(e, max_probes=37, curve_points=10)
        assert cut._filter_strs([c5], [g5], assume_unique=True) == [picks[:37]]
        assert cut.last_budget_kept == [37] and np.array_equal(cut.last_pick_gains[0], gains)
        at = [row for row in cut.last_coverage_curve[0] if row[0] == 37]
        assert len(at) == 1 and at[0][1] == int(gains[:37].sum()) and cut.last_timings["picks"] == 37
    else:
        assert int(gains.sum()) < coverable and np.all(gains > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_filter_reports_the_gains_of_an_extension_from_five_genomes_to_ten(ctx, oracle, e):
    g10, c10, _d10, d5 = _design(e)
    glen = [g.size() for g in g10]
    new, _nreduced = _oracle_extension(oracle, c10, d5, g10, e, 1.0)
    new = [int(i) for i in new]
    rows, cov = _oracle_rows(oracle, c10, g10, e), _oracle_rows(oracle, d5, g10, e)
    reduced = _np_subtract(rows, cov, glen)
    n2, c0 = _union_len(reduced, len(glen)), _union_len(cov, len(glen))
    f = _filter(e, fixed_probes=d5, pick_gains=True, curve_points=5)
    assert f._filter_strs([c10], [g10], assume_unique=True) == [new]
    ck = [row[0] for row in f.last_coverage_curve[0]]
    want_gains, want_curve = _model(reduced, glen, new, ck, n2 + c0, c0)
    gains = f.last_pick_gains[0]
    assert np.array_equal(gains.astype(np.int64), want_gains) and np.all(gains > 0)
    coverable = int((n2 + c0).sum())
    assert f.last_coverage_curve[0] == [(k, t, coverable, u, c, int((n2 + c0)[u]))
                                        for k, (t, u, c) in zip(ck, want_curve)]
    last = f.last_coverage_curve[0][-1]
    assert last[0] == len(new) and last[1] == int(c0.sum()) + int(gains.sum()) == coverable
    print("e = %d: %d fixed probes cover %d of %d bases, %d new picks add %d; gains_ms %.3f"
          % (e, len(d5), int(c0.sum()), coverable, len(new), int(gains.sum()), f.last_timings["gains_ms"]))
    # after pruning, the gains are those of the pruned list on the same table
    p = _filter(e, fixed_probes=d5, pick_gains=True, prune_redundant=True)
    kept = p._filter_strs([c10], [g10], assume_unique=True)[0]
    assert len(kept) + len(p.last_pruned[0]) == len(new)
    assert np.array_equal(p.last_pick_gains[0].astype(np.int64), _model(reduced, glen, kept)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [False, True])
def test_filter_releases_the_tables_kept_for_the_cut_when_a_later_group_raises(ctx, monkeypatch, fixed):
    from catch_amd import engine
    g5, c5 = _ebola5()
    seen, real = [], engine.Rows.pick_gains

    def failing(self, *args, **kw):
        seen.append(self)
        if len(seen) == 2:
            raise RuntimeError("the second group fails")
        return real(self, *args, **kw)
    monkeypatch.setattr(engine.Rows, "pick_gains", failing)
    f = _filter(50, max_probes=40, fixed_probes=c5[:3] if fixed else None)
    with pytest.raises(RuntimeError, match="the second group fails"):
        f._filter_strs([c5, c5], [g5, g5], assume_unique=True)
    assert len(seen) == 2 and seen[0] is not seen[1]
    assert all(not t._h for t in seen)                   # both closed: the one held for the cut too
    monkeypatch.setattr(engine.Rows, "pick_gains", real)
    again = _filter(50, max_probes=40, fixed_probes=c5[:3] if fixed else None)
    kept = again._filter_strs([c5, c5], [g5, g5], assume_unique=True)
    assert sum(again.last_budget_kept) >= 40 and [len(k) for k in kept] == again.last_budget_kept


# ------------------------------------------------------------------ command line
def _read_curve(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["dataset", "probes", "bases_covered", "bases_coverable", "fraction", "worst_genome",
                                    "worst_genome_fraction"]
    blocks = {}
    for ln in lines[1:]:
        cells = ln.split("\t")
        assert len(cells) == 7
        blocks.setdefault(cells[0], []).append(cells[1:])
    return blocks


@pytest.mark.gpu
def test_design_max_probes_end_to_end(ctx, tmp_path, capsys):
    from catch_amd import design
    from catch_amd.filter.set_cover_filter import allocate_budget
    from catch_amd.utils import seq_io
    records = list(seq_io.read_fasta(EBOLA).items())
    fa = [_write_fasta(tmp_path / "one.fasta", records[:5]), _write_fasta(tmp_path / "two.fasta", records[5:10])]
    base = fa + ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
    for extra in ([], ["--prune-redundant"]):
        tag = "pruned" if extra else "plain"
        capsys.readouterr()
        full, cut, curve = (str(tmp_path / (tag + name)) for name in ("_full.fasta", "_cut.fasta", "_curve.tsv"))
        design.main(design.parse_args(base + extra + ["-o", full]))
        whole = list(seq_io.iterate_fasta(full))
        assert capsys.readouterr().out.split() == [str(len(whole))] and len(whole) > 200
        design.main(design.parse_args(base + extra + ["--max-probes", "200", "--write-coverage-curve", curve, "-o", cut]))
        assert capsys.readouterr().out.split() == ["200"]
        kept = list(seq_io.iterate_fasta(cut))
        assert len(kept) == 200
        blocks = _read_curve(curve)
        assert list(blocks) == ["one.fasta", "two.fasta", "*"]
        n1, n2 = int(blocks["one.fasta"][-1][0]), int(blocks["two.fasta"][-1][0])
        # the picks of the two datasets (the designer writes a probe picked for both once)
        genomes = [seq_io.read_genomes_from_fasta(p) for p in fa]
        cands = [_candidates(g) for g in genomes]
        f = _filter(50, pick_gains=True, prune_redundant=bool(extra))
        picked = f._filter_strs(cands, genomes, assume_unique=True)
        assert [len(p) for p in picked] == [n1, n2]
        strs = [[c[i] for i in p] for c, p in zip(cands, picked)]
        assert list(dict.fromkeys(strs[0] + strs[1])) == whole
        # the records are per-dataset prefixes of the run without a budget: those the merge by gain takes until
        # 200 distinct probes are kept
        k1, k2 = allocate_budget(f.last_pick_gains, 200, strs)
        assert 0 < k1 <= n1 and 0 < k2 <= n2 and k1 + k2 >= 200
        assert kept == list(dict.fromkeys(strs[0][:k1] + strs[1][:k2]))
        order = _merge(f.last_pick_gains)
        assert sorted(order[:k1 + k2]) == [(0, i) for i in range(k1)] + [(1, i) for i in range(k2)]
        assert len(set(strs[gi][pos] for gi, pos in order[:k1 + k2 - 1])) == 199
        cutf = _filter(50, max_probes=200, prune_redundant=bool(extra))
        assert cutf._filter_strs(cands, genomes, assume_unique=True) == [picked[0][:k1], picked[1][:k2]]
        assert cutf.last_budget_kept == [k1, k2]
        for name, k in (("one.fasta", k1), ("two.fasta", k2)):
            rows = blocks[name]
            assert [int(r[0]) for r in rows] == sorted({int(r[0]) for r in rows}) and len(rows) <= 101
            assert any(int(r[0]) == k for r in rows)                       # the cut is measured
            assert rows[-1][1] == rows[-1][2] and float(rows[-1][3]) == 1.0 and float(rows[-1][5]) == 1.0
            assert all(int(a[1]) <= int(b[1]) for a, b in zip(rows, rows[1:]))
            assert all(0 <= int(r[4]) < 5 and 0.0 <= float(r[5]) <= float(r[3]) + 1e-6 for r in rows)
        # the merged block: the cumulative sum of the gains in merged order
        cum = np.cumsum([int(f.last_pick_gains[gi][pos]) for gi, pos in order])
        star = blocks["*"]
        assert [int(r[0]) for r in star] == list(range(1, n1 + n2 + 1))
        assert [int(r[1]) for r in star] == cum.tolist()
        coverable = int(blocks["one.fasta"][-1][2]) + int(blocks["two.fasta"][-1][2])
        assert all(int(r[2]) == coverable and r[4] == "NA" and r[5] == "NA" for r in star)
        assert int(star[-1][1]) == coverable
        at = {name: next(r for r in blocks[name] if int(r[0]) == k) for name, k in (("one.fasta", k1), ("two.fasta", k2))}
        assert int(at["one.fasta"][1]) + int(at["two.fasta"][1]) == int(star[k1 + k2 - 1][1])
        print("%s: %d + %d picks, %d distinct; budget 200 keeps %d + %d, %d of %d coverable bases"
              % (tag, n1, n2, len(whole), k1, k2, int(star[k1 + k2 - 1][1]), coverable))
