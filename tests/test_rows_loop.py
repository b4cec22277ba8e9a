"""SetCoverFilter._filter_strs_keeping_rows, the one loop behind fixed_probes, coverage_depth, prune_redundant and
pick_gains / max_probes, and the helpers the filter's paths share.  On the host: the packer, needs_rows and the
timings' base keys.  On the GPU: every combination of the options replayed against what the commit before the loop
selected and reported (tests/golden/rows_loop_parent.json.gz, written by tests/golden/make_rows_loop_golden.py)."""
import gzip
import importlib.util
import itertools
import json
import os
import random

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
RUNS = 29


# ------------------------------------------------------------------ host
def _pack_as_before(sizes, cap, counts=None, count_cap=None):
    """The chunking loop as _filter_genomes_device_union and _filter_strs_union each spelled it out."""
    chunks, at = [], 0
    while at < len(sizes):
        chunk, total, n = [], 0, 0
        while at < len(sizes):
            if chunk and (total + sizes[at] > cap or (counts is not None and n + counts[at] > count_cap)):
                break
            chunk.append(at)
            total += sizes[at]
            n += counts[at] if counts is not None else 0
            at += 1
        chunks.append(chunk)
    return chunks


def test_pack_under_cap():
    from catch_amd.filter.set_cover_filter import _pack_under_cap
    assert _pack_under_cap([5, 5, 5], 10) == [[0, 1], [2]]
    assert _pack_under_cap([12, 3], 10) == [[0], [1]]              # alone above the cap: a chunk of its own
    assert _pack_under_cap([10, 1], 10) == [[0], [1]]
    assert _pack_under_cap([], 10) == []
    assert _pack_under_cap([4, 4, 4, 4], 100, [3, 3, 3, 3], 7) == [[0, 1], [2, 3]]
    rng = random.Random(3)
    for _ in range(300):
        n = rng.randrange(0, 12)
        sizes = [rng.randrange(0, 15) for _ in range(n)]
        counts = [rng.randrange(0, 6) for _ in range(n)]
        cap, count_cap = rng.randrange(1, 30), rng.randrange(1, 12)
        assert _pack_under_cap(sizes, cap) == _pack_as_before(sizes, cap)
        assert _pack_under_cap(sizes, cap, counts, count_cap) == _pack_as_before(sizes, cap, counts, count_cap)


def _option_grid():
    """(keywords, needs the rows) over fixed probes x depth x pruning x gains, without what the constructor refuses."""
    out = []
    for fixed, deep, prune, gains in itertools.product((False, True), repeat=4):
        if deep and (fixed or gains):
            continue
        kw = {}
        if fixed:
            kw["fixed_probes"] = ["ACGT" * 25]
        if deep:
            kw["coverage_depth"] = 2
        if prune:
            kw["prune_redundant"] = True
        if gains:
            kw["pick_gains"] = True
        out.append((kw, fixed or deep or prune or gains))
    return out


def test_needs_rows_over_the_option_grid():
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    grid = _option_grid()
    assert len(grid) == 10 and sum(1 for _kw, want in grid if not want) == 1
    for kw, want in grid:
        assert SetCoverFilter(2, 100, **kw).needs_rows is want, kw
    assert SetCoverFilter(2, 100, max_probes=3).needs_rows is True          # (it implies pick_gains)
    for kw in (dict(fixed_probes=["ACGT" * 25]), dict(pick_gains=True), dict(max_probes=3)):
        with pytest.raises(NotImplementedError):
            SetCoverFilter(2, 100, coverage_depth=2, **kw)


def test_device_front_end_is_left_exactly_when_the_rows_are_needed():
    from catch_amd.filter import probe_designer
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    from catch_amd.genome import Genome
    genomes = [[Genome.from_one_seq("ACGT" * 100)]]
    first = DuplicateFilter()
    for kw, _want in _option_grid():
        f = SetCoverFilter(2, 100, **kw)
        pd = probe_designer.ProbeDesigner(genomes, [first, f], 100, 50)
        assert pd._device_front_end_mode(genomes, first, f) == (None if f.needs_rows else "per group"), kw


def test_new_timings_has_the_base_keys():
    from catch_amd.filter.set_cover_filter import _new_timings
    base = dict(scan_ms=0.0, rows_ms=0.0, greedy_ms=0.0, picks=0, rows=0, scan_launches=0, greedy_launches=0)
    t = _new_timings()
    assert t == base and all(type(t[k]) is type(base[k]) for k in base)
    assert _new_timings(candidates=0, depth_ms=0.0) == dict(base, candidates=0, depth_ms=0.0)
    t["picks"] += 1
    assert _new_timings()["picks"] == 0                            # a fresh dict per call


# ------------------------------------------------------------------ GPU: the parent's recording, replayed
@pytest.mark.gpu
def test_every_option_combination_equals_the_parent(ctx, tmp_path):
    spec = importlib.util.spec_from_file_location("make_rows_loop_golden",
                                                  os.path.join(GOLDEN, "make_rows_loop_golden.py"))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    with gzip.open(os.path.join(GOLDEN, "rows_loop_parent.json.gz"), "rt") as f:
        recorded = json.load(f)
    assert len(recorded["recorded_at"]) == 40 and len(recorded["runs"]) == RUNS
    configs = recorder.configurations()
    assert [r["config"] for r in recorded["runs"]] == configs
    g5, c5 = recorder.inputs()
    avoided = recorder.write_avoided(tmp_path, g5)
    replayed = 0
    for want in recorded["runs"]:
        got, _timings = recorder.run(want["config"], g5, c5, avoided)
        assert sorted(got) == sorted(want)
        for field in want:
            assert got[field] == want[field], (want["config"], field)
        replayed += 1
    assert replayed == len(recorded["runs"]) == RUNS
