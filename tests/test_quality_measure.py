"""The measure behind the candidate rules (catch_amd/filter/quality.py; not in the reference): gc, homopolymer, dust,
stem and dimer as values, where the filters only say yes or no at a threshold.  The measure exists three times: measure
(from the quantifiers: the oracle), the NumPy form of the host path and the kernels of the device front end
(catchhip_candidates_measure).  Here: measure against a brute force over positions and hand values; its ties to _fails of
CompositionFilter and StructureFilter, to TmFilter and to BackgroundFilter; NumPy against measure; the kernels against
the definition, candidate by candidate, and the four flag kernels against the measured values.

The kernel tests compare with the NumPy form, which is fast enough for 2,000 candidates of 300 characters;
test_kernel_test_inputs_are_not_vacuous compares that reference with measure itself on the same inputs."""
import collections
import functools
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTNER = dict(A="T", C="G", G="C", T="A")
NAME = "catchhip_candidates_measure"
FIVE = ("gc", "homopolymer", "dust", "stem", "dimer")
PS, WS = (0, 3, 7), (3, 16, 64, 256)


def Q():
    from catch_amd.filter import quality
    return quality


def _revcomp(u):
    return "".join(PARTNER[c] for c in reversed(u))


def _pairs(s, x, y):
    return s[x] in PARTNER and s[y] == PARTNER[s[x]]


# ------------------------------------------------------------------ the definition, by brute force and by hand
def _literal(s, P, W):
    """The five quantities by the quantifiers as the module states them, nothing rearranged."""
    L = len(s)
    gc = len([c for c in s if c in "GC"])
    homopolymer = max([n for n in range(1, L + 1) for a in range(L - n + 1)
                       if s[a] in PARTNER and s[a:a + n] == s[a] * n], default=0)
    dust = 0
    if L >= 3:
        We = min(W, L)
        for i in range(L - We + 1):
            trip = [s[j:j + 3] for j in range(i, i + We - 2) if all(c in PARTNER for c in s[j:j + 3])]
            T = len(trip)
            S = sum(c * (c - 1) // 2 for c in collections.Counter(trip).values())
            if T >= 2:
                dust = max(dust, next(X for X in range(10 * S + 1) if not 10 * S > X * (T - 1)))
    stem = max([n for n in range(1, L + 1) for i in range(L) for j in range(i + 1, L)
                if i + n - 1 < L and j - n + 1 >= 0 and all(_pairs(s, i + t, j - t) for t in range(n))
                and (j - n + 1) - (i + n - 1) - 1 >= P], default=0)
    dimer = max([n for n in range(1, L + 1) for a in range(L) for b in range(L)
                 if a + n - 1 <= L - 1 and b - n + 1 >= 0 and all(_pairs(s, a + t, b - t) for t in range(n))], default=0)
    return gc, homopolymer, dust, stem, dimer


def test_measure_equals_its_quantifiers():
    rng = random.Random(17)
    seen = collections.defaultdict(set)
    for _ in range(500):
        L = rng.randrange(0, 19)
        s = "".join(rng.choice(rng.choice(["AT", "ACGT", "ACGTN", "AC", "ACGTx"])) for _ in range(L))
        P, W = rng.choice(PS), rng.choice([3, 5, 16, 64])
        got = Q().measure(s, P, W)
        assert got == _literal(s, P, W), (s, P, W)
        assert got[3] <= got[4] <= L and got[3] <= max(0, (L - P) // 2) and got[2] <= 5 * max(0, min(W, L) - 2)
        for name, v in zip(FIVE, got):
            seen[name].add(v)
    assert all(len(seen[name]) >= 5 for name in FIVE), seen


def test_hand_values():
    m = Q().measure
    assert m("ACGT", 3) == (2, 1, 0, 0, 4)
    assert m("ACxxxGT") == (2, 1, 0, 2, 2)
    assert m("AT" * 20, 3, 64) == (0, 1, 93, 18, 40)
    # dust rounds up: (AC)32 scores 9300 / 61 = 152.46, is dropped at 152 and kept at 153; A x 64 is 310 exactly
    assert m("AC" * 32)[2] == 153 and m("A" * 64)[2] == 310 and m("A" * 64)[1] == 64
    assert m("") == (0, 0, 0, 0, 0) and m("A") == (0, 1, 0, 0, 0) and m("N") == (0, 0, 0, 0, 0)
    assert m("AT", 0) == (0, 1, 0, 1, 2) and m("AT", 1) == (0, 1, 0, 0, 2) and m("acgt") == (0, 0, 0, 0, 0)
    assert m("AAA")[2] == 0 and m("AAAA")[2] == 10 and m("AAAA", 3, 3)[2] == 0
    # the loop: the same arms, one character too close
    for P in (1, 3, 7):
        arm = "ACCAACACCA"[:5]
        assert m(arm + "x" * P + _revcomp(arm), P)[3:] == (5, 5)
        assert m(arm + "x" * (P - 1) + _revcomp(arm), P)[3] == 4       # the innermost pair gives way to the loop
    # loop 0: the run crosses the middle of an odd antidiagonal and dimer is twice the arm
    assert m("xACCAC" + "GTGGTx", 0)[3:] == (5, 10) and m("xACCAC" + "GTGGTx", 3)[3:] == (3, 10)
    for bad in (dict(min_loop=-1), dict(min_loop=1.5), dict(dust_window=2), dict(dust_window=257), dict(dust_window="64")):
        with pytest.raises(ValueError):
            m("ACGT", **bad)


def test_ties_to_the_composition_and_structure_filters():
    """The thresholds at which _fails of the two filters drops a string are exactly those below its measured value."""
    from catch_amd.filter.composition_filter import CompositionFilter
    from catch_amd.filter.structure_filter import StructureFilter
    rng = random.Random(23)
    strs = []
    for k in range(400):
        L = rng.randrange(2, 71)
        s = [rng.choice(("AT", "ACGT", "ACGTN", "AC", "ACGTx")[k % 5]) for _ in range(L)]
        if k % 3 == 0 and L >= 12:
            R, loop = rng.randrange(2, L // 4 + 1), rng.choice([0, 1, 3, 7])
            arm = "".join(rng.choice("ACGT") for _ in range(R))
            at = rng.randrange(0, L - 2 * R - loop + 1) if 2 * R + loop <= L else None
            if at is not None:
                s[at:at + 2 * R + loop] = arm + "x" * loop + _revcomp(arm)
        if k % 7 == 0:
            at = rng.randrange(0, L)
            s[at:at + 9] = list((rng.choice("ACGT") * 9)[:len(s[at:at + 9])])
        strs.append("".join(s))
    n = 0
    for s in strs:
        L = len(s)
        for P in PS:
            gc, run, _, stem, dimer = Q().measure(s, P, 64)
            for K in range(1, 14):
                assert StructureFilter(max_hairpin_stem=K, hairpin_min_loop=P)._fails(s)[0] == (stem > K), (s, K, P)
            for D in range(1, 20):
                assert StructureFilter(max_self_dimer=D)._fails(s)[1] == (dimer > D), (s, D)
            n += 13 + 19
        for W in (3, 16, 64):
            gc, run, dust, _, _ = Q().measure(s, 3, W)
            for X in (0, 1, 5, 20, 60, 152, 153, 310):
                assert CompositionFilter(max_dust=X, dust_window=W)._fails(s)[2] == (dust > X), (s, X, W)
            n += 8
        for H in range(1, 8):
            assert CompositionFilter(max_homopolymer=H)._fails(s)[1] == (run > H), (s, H)
        for rng_gc in (("0.4", "0.6"), ("0", "0.5"), ("1/3", "1")):
            f = CompositionFilter(gc_range=rng_gc)
            lo, hi = f._gc_bounds(L)
            assert f._fails(s)[0] == (not lo <= gc <= hi)
        n += 10
    assert n == 400 * (3 * 32 + 3 * 8 + 10)


def test_tm_and_hits_are_the_filters_own():
    """tm_c and hits have no second definition: the report and the kernels are compared with TmFilter._tm_c and
    BackgroundFilter._hits, whose NumPy forms these are."""
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.filter.tm_filter import TmFilter
    rng = random.Random(4)
    strs = ["".join(rng.choice("ACGTN") for _ in range(40)) for _ in range(50)]
    tf = TmFilter(sodium_mm="100", formamide_pct="10")
    assert tf._tm_c_equal_length(strs, 40).tolist() == [tf._tm_c(s) for s in strs] and tf._tm_c("A") is None
    bf = BackgroundFilter(["".join(strs[:10])], kmer=8)
    hits = bf._hits_equal_length(strs, 40).tolist()
    assert hits == [bf._hits(s) for s in strs] and max(hits) > 5 and min(hits) == 0 and bf._hits("ACGT") == 0


# ------------------------------------------------------------------ host: NumPy against the definition
@pytest.mark.parametrize("alphabet", ["AT", "ACGT", "ACGTN"])
def test_numpy_measure_equals_definition(alphabet):
    rng = random.Random(len(alphabet))
    for L in list(range(1, 40)) + [64, 65, 100]:
        n = 24 if L < 40 else 6
        strs = ["".join(rng.choice(alphabet) for _ in range(L)) for _ in range(n)]
        if L >= 10:
            arm = "".join(rng.choice("ACGT") for _ in range(L // 4))
            strs.append((arm + "x" * rng.choice([0, 1, 3]) + _revcomp(arm)).ljust(L, "n")[:L])
        for P, W in ((0, 3), (3, 64), (7, 16)):
            got = Q().measure_equal_length(strs, L, P, W)
            assert got.tolist() == [list(Q().measure(s, P, W)) for s in strs], (L, P, W)
            assert Q().measure_equal_length(strs, L, P, W, structure=False)[:, :3].tolist() == got[:, :3].tolist()
            assert Q().measure_equal_length(strs, L, P, W, composition=False)[:, 3:].tolist() == got[:, 3:].tolist()


def test_numpy_measure_in_chunks_mixed_lengths_and_duplicates(monkeypatch):
    from catch_amd import probe
    q = Q()
    rng = random.Random(3)
    a = ["".join(rng.choice("ACGT") for _ in range(24)) for _ in range(300)]
    a = a + a[:150] + ["".join(rng.choice("ACGTN") for _ in range(rng.randrange(0, 40))) for _ in range(200)]
    rng.shuffle(a)
    want = [list(q.measure(s, 3, 16)) for s in a]
    assert q.measure_many(a, 3, 16).tolist() == want
    calls = []
    real = q.measure_equal_length
    monkeypatch.setattr(q, "measure_equal_length", lambda strs, L, *r, **k: calls.append((L, len(strs))) or real(strs, L, *r, **k))
    monkeypatch.setattr(q, "_CHUNK_CELLS", 25 * 64)                  # 64 strings of 24 characters a chunk
    assert q.measure_many(a, 3, 16).tolist() == want
    assert max(n for L, n in calls if L == 24) == 64 and sum(n for L, n in calls if L == 24) >= 450
    # the profile counts what it is given, duplicates too, and drops nothing
    prof = q.QualityProfile(3, 16)
    assert prof._filter_strs(a) == a and prof._filter_strs([]) == []
    probes = [probe.Probe.from_str(s) for s in a[:50] if s]
    assert prof._filter(probes) == probes
    both = want + [w for w, s in zip(want[:50], a[:50]) if s]
    for k, name in enumerate(FIVE):
        assert prof.histograms[k].tolist() == np.bincount([w[k] for w in both], minlength=1280).tolist(), name
    for bad in (dict(min_loop=-1), dict(dust_window=2), dict(dust_window=300)):
        with pytest.raises(ValueError):
            q.QualityProfile(**bad)


def test_write_profile_format(tmp_path):
    q = Q()
    prof = q.QualityProfile()
    path = tmp_path / "p.tsv"
    prof.write_profile(str(path))
    assert path.read_text() == "quantity\tvalue\tcandidates\tcandidates_above\n" and prof.medians()["gc"] is None
    strs = ["ACGT" * 5, "ACGT" * 5, "AAAAAAAAAAAAAAAAAAAA", "ACCACxxxGTGGTxxxxxxx", "G" * 20]
    prof._filter_strs(strs)
    prof.write_profile(str(path))
    rows = [line.split("\t") for line in path.read_text().splitlines()]
    assert rows[0] == ["quantity", "value", "candidates", "candidates_above"]
    vals = [q.measure(s) for s in strs]
    at = 1
    for k, name in enumerate(FIVE):
        col = [v[k] for v in vals]
        for value in range(min(col), max(col) + 1):                  # lowest to highest, the empty ones between included
            assert rows[at] == [name, str(value), str(col.count(value)), str(sum(1 for c in col if c > value))], (name, value)
            at += 1
        assert rows[at - 1][3] == "0"
    assert at == len(rows)
    assert prof.medians() == {name: sorted(v[k] for v in vals)[2] for k, name in enumerate(FIVE)}
    # values from 1279 up share the last bin
    big = q.QualityProfile()
    big._count(q.histograms_of(np.array([[1279, 5000, 1270, 2, 65535]])))
    assert [int(np.flatnonzero(h)[0]) for h in big.histograms] == [1279, 1279, 1270, 2, 1279]


def test_symbol_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    at = re.search(r"\b%s\s*\(" % NAME, hdr)
    assert at and "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 17
    assert hasattr(_lib.lib(), NAME) and hasattr(engine.Candidates, "measure")
    assert "measure.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------ inputs of the kernel tests
def _planted(rng, L, R, loop, start, filler="x"):
    """A stem of exactly R pairs -- an arm over A and C from `start`, `loop` fillers, its reverse complement -- in a
    background that pairs with nothing; None where it does not fit."""
    if start < 0 or start + 2 * R + loop > L:
        return None
    arm = "".join(rng.choice("AC") for _ in range(R))
    s = filler * start + arm + filler * loop + _revcomp(arm)
    return s + filler * (L - len(s))


LENGTHS = [2, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300]
# where the two launches (csrc/measure.hip) change their workgroup, in the call the kernel test makes first -- both
# families, values and histograms, W = 64 -- and in the structure launch without histograms; the mirrors are below
TIER_EDGES = [145, 146, 288, 289, 353, 354, 544, 545, 640, 641, 721, 722, 992, 993, 1312, 1313]
RUNS = (31, 32, 33, 64, 65)
LOOPS = (0, 1, 2, 3, 6, 7)                   # 0, 1, P - 1 and P of the three P


def _structure_workgroup(L, histograms):
    """(candidates per workgroup, bytes of dynamic LDS) of measure_structure_kernel; (256, bins only): planes in global memory."""
    per = (6 * ((L + 31) // 32) + 7) * 4
    bins = 2 * (min(L, 1279) + 1) * 8 if histograms else 0
    for rows in (256, 128, 64):
        if rows * per + 4 + bins <= 65536:
            return rows, ((rows * per // 4 + 1) & ~1) * 4 + bins
    return 256, bins


def _rows_workgroup(L, W, histograms, tm=False):
    """(candidates per workgroup, rows staged) of measure_rows_kernel with the composition family on."""
    pitch = 4 * ((L + 30) // 16) + 1
    We = min(W, L) if L >= 4 else 0
    bins = (2 * (min(L, 1279) + 1) + (min(5 * (We - 2), 1279) + 1 if We else 1)) * 8 if histograms else 0
    extra = (64 if tm else 0) + bins
    for rows in (256, 128, 64):
        if rows * (pitch * 4 + (64 if We else 0)) + extra + 4 <= 65536:
            return rows, True
    return 256, False


def test_tier_edges_sit_on_the_workgroup_sizes_claimed():
    assert [_structure_workgroup(L, True)[0] for L in (256, 257, 544, 545, 992, 993)] == [256, 128, 128, 64, 64, 256]
    assert _structure_workgroup(992, True) == (64, 65296) and _structure_workgroup(993, True) == (256, 15904)
    assert [_structure_workgroup(L, False) for L in (288, 289, 640, 641, 1312, 1313)] == [
        (256, 62464), (128, 34304), (128, 65024), (64, 34048), (64, 64768), (256, 0)]
    assert [_rows_workgroup(L, 64, True) for L in (145, 146, 353, 354, 721, 722)] == [
        (256, True), (128, True), (128, True), (64, True), (64, True), (256, False)]
    for L in LENGTHS + TIER_EDGES:           # every change of either launch between two lengths run is an edge named above
        assert L in TIER_EDGES or L <= 300
    changes = [L for L in range(3, 1400) if _structure_workgroup(L, True)[0] != _structure_workgroup(L - 1, True)[0]
               or _structure_workgroup(L, False)[0] != _structure_workgroup(L - 1, False)[0]
               or _rows_workgroup(L, 64, True) != _rows_workgroup(L - 1, 64, True)]
    assert set(changes) <= set(LENGTHS + TIER_EDGES) and all(L - 1 in LENGTHS + TIER_EDGES for L in changes)


def _candidates(L):
    """2,000 candidates of L characters (400 beyond L = 300), a third of them duplicates: random over AT, ACGT, ACGTN (N
    isolated: two in a row would cut the window) and AC; stems planted with loops 0, 1, P - 1 and P at both ends of the
    candidate and across every 32- and 64-character boundary, in fillers x, n, -; arms of exactly 31, 32, 33, 64 and 65
    pairs where they fit (with loop 0 the run crosses the middle of an odd antidiagonal: dimer is twice the arm);
    (AT)n whole, whose dimer is L; a candidate with no base at all."""
    rng = random.Random(3000 + L)
    total = 2000 if L <= 300 else 400
    planted = []
    for R in (1, 2, 4, 5, 9, 10, 13):
        for loop in LOOPS:
            span = 2 * R + loop
            starts = {0, L - span} | {b - R // 2 for b in range(32, L, 32)} | {b - R - loop - R // 2 for b in range(32, L, 32)}
            for start in sorted(starts):
                s = _planted(rng, L, R, loop, start, rng.choice("xn-"))
                if s is not None:
                    planted.append(s)
    rng.shuffle(planted)
    planted = planted[:total // 4]
    for R in RUNS:
        for loop in LOOPS:
            for start in (0, L - 2 * R - loop, (L - 2 * R - loop) // 2):
                s = _planted(rng, L, R, loop, start, rng.choice("xn-"))
                if s is not None:
                    planted.append(s)
    special = [("AT" * L)[:L], "x" * L, ("TA" * L)[:L], "A" * L, ("AC" * L)[:L]]
    out = special + planted
    nrandom = max(total * 2 // 3 - len(out), total // 4)
    for k in range(nrandom):
        alpha = ("AT", "ACGT", "ACGTN", "AC", "ACGTNNNN", "AAT", "ACGGC")[k % 7]
        s = "".join(rng.choice(alpha) for _ in range(L))
        out.append(re.sub("NN", "Nn", re.sub("NN", "Nn", s)))
    out += [rng.choice(out) for _ in range(max(total - len(out), (len(out) + 1) // 2))]     # duplicates, for the multiplicities
    rng.shuffle(out)
    assert not any("NN" in s for s in out) and all(len(s) == L for s in out)
    return out


@functools.lru_cache(maxsize=None)
def _unique(L):
    c = collections.Counter(_candidates(L))
    return tuple(sorted(c)), c


@functools.lru_cache(maxsize=None)
def _composition(L, W):
    """{candidate: (gc, homopolymer, dust)} over the unique candidates of length L: computed once per (L, W)."""
    uniq = _unique(L)[0]
    got = Q().measure_equal_length(list(uniq), L, 3, W, structure=False)[:, :3]
    return dict(zip(uniq, map(tuple, got.tolist())))


@functools.lru_cache(maxsize=None)
def _structure(L, P):
    """{candidate: (stem, dimer)}, once per (L, P)."""
    uniq = _unique(L)[0]
    got = Q().measure_equal_length(list(uniq), L, P, 64, composition=False)[:, 3:]
    return dict(zip(uniq, map(tuple, got.tolist())))


def _check_inputs(L):
    """The conditions of the issue on the inputs at length L, or the exact reason one cannot hold there."""
    uniq, counts = _unique(L)
    assert sum(counts.values()) >= (2000 if L <= 300 else 400) and max(counts.values()) > 1
    assert 3 * (sum(counts.values()) - len(uniq)) >= sum(counts.values()) - 3 or L <= 3     # a third are duplicates
    for P in PS:
        comp, struct = _composition(L, 64), _structure(L, P)
        cols = list(zip(*[comp[s] + struct[s] for s in uniq]))
        for name, col in zip(FIVE, cols):
            if L >= 31 and not (name == "stem" and L < 2 * 4 + P):
                assert len(set(col)) >= 4, (L, P, name)
        stem, dimer = cols[3], cols[4]
        assert all(a <= b for a, b in zip(stem, dimer))
        assert any(a < b for a, b in zip(stem, dimer)) and any(a == b for a, b in zip(stem, dimer)), (L, P)
        if L >= 100:
            assert max(stem) >= 33 and max(dimer) >= 33, (L, P)
        else:
            # an arm of 33 pairs and a loop of P need 66 + P characters; a self-dimer of 33 pairs needs 34: the only
            # antidiagonal of 33 cells in a table of 33 x 33 holds its own middle cell, which never pairs
            assert L >= 66 + P or max(stem) <= max(0, (L - P) // 2) < 33, (L, P)
            assert (max(dimer) >= 33) == (L >= 34), (L, P)
        assert max(dimer) == L or L % 2, (L, P)                        # (AT)n whole
        assert struct["x" * L] == (0, 0) and comp["x" * L] == (0, 0, 0)
    return uniq, counts


@pytest.mark.parametrize("L", [2, 3, 31, 33, 64, 100])
def test_kernel_test_inputs_are_not_vacuous(L):
    """No GPU: the inputs of the kernel test spread every quantity (the other lengths are checked where they run), and
    the NumPy reference of the kernel test equals measure on a sample of them."""
    uniq, _ = _check_inputs(L)
    rng = random.Random(L)
    for s in rng.sample(uniq, min(len(uniq), 25)) + [("AT" * L)[:L]]:
        for P, W in ((0, 3), (3, 64), (7, 256)):
            assert _composition(L, W)[s] + _structure(L, P)[s] == Q().measure(s, P, W), (s, P, W)
    assert 400 <= sum(_unique(641)[1].values()) < 500


# ------------------------------------------------------------------ GPU: the kernels against the definition
def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


@pytest.fixture(scope="module")
def device_lists(ctx):
    """Per length: the targets (one sequence per candidate, stride = L: the windows are the candidates) and the
    unique list, made once and shared by the tests of that length."""
    from catch_amd import engine
    made = {}

    def get(L):
        if L not in made:
            seqs = _candidates(L)
            targets = engine.Targets(ctx, [[s] for s in seqs])
            base = engine.Candidates(ctx, targets, L, L)
            made[L] = (targets, "".join(seqs), base, _snapshot(base, "".join(seqs), L))
        return made[L]
    yield get
    for targets, _, base, _ in made.values():
        base.close()
        targets.close()


def _hist_of(values, mult):
    return np.bincount(np.minimum(np.asarray(values, dtype=np.int64), 1279), weights=mult, minlength=1280).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS + TIER_EDGES)
def test_measure_kernel_equals_definition(ctx, device_lists, monkeypatch, L):
    """catchhip_candidates_measure against the definition for P in 0, 3, 7 and W in 3, 16, 64, 256: every value of every
    unique candidate, every histogram against np.bincount weighted by the multiplicities, the list untouched, and
    the narrower calls (values only, histograms only, one family, Tm, hits) against the full one."""
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.filter.tm_filter import TmFilter
    if L == 1313:                            # a plane buffer of 100 candidates: the list takes several launches
        monkeypatch.setenv("CATCHHIP_STRUCT_PLANE_BYTES", str(100 * (6 * 42 + 7) * 4))
    if L > 100:
        _check_inputs(L)
    targets, concat, c, (pos0, mult0, grp0, strs0) = device_lists(L)
    uniq, counts = _unique(L)
    n = len(strs0)
    assert sorted(strs0) == list(uniq) and [counts[s] for s in strs0] == mult0.tolist() and c.n == n
    assert n > 256 or L <= 3
    weights = mult0.astype(np.float64)
    for P in PS:
        for W in WS:
            comp, struct = _composition(L, W), _structure(L, P)
            want = np.array([comp[s] + struct[s] for s in strs0], dtype=np.int64).reshape(n, 5)
            got = c.measure(what=("composition", "structure"), min_loop=P, dust_window=W, values=True, histograms=True)
            for k, name in enumerate(FIVE):
                wrong = np.flatnonzero(got[name].astype(np.int64) != want[:, k])
                assert wrong.size == 0, (name, P, W, [(strs0[i], int(got[name][i]), int(want[i, k])) for i in wrong[:3]])
                assert got[name].dtype == np.uint16
                assert got["histograms"][name].tolist() == _hist_of(want[:, k], weights).tolist(), (name, P, W)
            assert sorted(got) == sorted(FIVE + ("histograms",))
    # the list is as it was
    pos, mult, grp, _ = _snapshot(c, concat, L)
    assert (pos.tolist(), mult.tolist(), grp.tolist(), c.n) == (pos0.tolist(), mult0.tolist(), grp0.tolist(), n)
    # narrower calls at P = 3, W = 64
    full = c.measure(min_loop=3, dust_window=64, values=True, histograms=True)
    only_values = c.measure(min_loop=3, dust_window=64, values=True, histograms=False)
    only_hist = c.measure(min_loop=3, dust_window=64, values=False, histograms=True)
    assert sorted(only_values) == sorted(FIVE) and sorted(only_hist) == ["histograms"]
    for name in FIVE:
        assert only_values[name].tolist() == full[name].tolist(), name
        assert only_hist["histograms"][name].tolist() == full["histograms"][name].tolist(), name
    tf = TmFilter(sodium_mm="75", formamide_pct="5")
    bf = BackgroundFilter(["".join(strs0[:40]), _revcomp("".join(s for s in strs0[40:60] if set(s) <= set("ACGT")))], kmer=12)
    index = bf._device_index(ctx)
    try:
        for family, names in (("composition", FIVE[:3]), ("structure", FIVE[3:])):
            one = c.measure(what=family, min_loop=3, dust_window=64, values=True, histograms=True)
            assert sorted(one) == sorted(names + ("histograms",)) and sorted(one["histograms"]) == sorted(names)
            for name in names:
                assert one[name].tolist() == full[name].tolist(), name
                assert one["histograms"][name].tolist() == full["histograms"][name].tolist(), name
        tm_want = tf._tm_c_equal_length(strs0, L)
        hits_want = bf._hits_equal_length(strs0, L) if L >= 12 else np.zeros(n, dtype=np.int64)
        assert L < 12 or (hits_want.max() >= L - 11 and (hits_want == 0).any())
        every = c.measure(what=("composition", "structure", "tm", "hits"), min_loop=3, dust_window=64,
                          tm=(tf._q(L), tf.offset_c), index=index, values=True, histograms=True)
        for name in FIVE:
            assert every[name].tolist() == full[name].tolist() and every["histograms"][name].tolist() == full["histograms"][name].tolist()
        assert every["tm_c"].dtype == np.int32 and every["tm_c"].tolist() == tm_want.tolist()
        assert every["hits"].dtype == np.uint32 and every["hits"].tolist() == hits_want.tolist()
        alone = c.measure(what=("tm", "hits"), tm=(tf._q(L), tf.offset_c), index=index, values=True, histograms=True)
        assert alone["tm_c"].tolist() == tm_want.tolist() and alone["hits"].tolist() == hits_want.tolist()
        assert alone["histograms"] == {} and c.measure(what="hits", index=index, values=True, histograms=False)["hits"].tolist() == hits_want.tolist()
        assert c.measure(what=("tm", "composition"), tm=(tf._q(L), tf.offset_c), values=True, histograms=False)["tm_c"].tolist() == tm_want.tolist()
    finally:
        bf.close()
    pos, mult, grp, _ = _snapshot(c, concat, L)
    assert (pos.tolist(), mult.tolist(), grp.tolist(), c.n) == (pos0.tolist(), mult0.tolist(), grp0.tolist(), n)


KS, DS = (1, 3, 9), (1, 4, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [33, 100, 300])
def test_flag_kernels_against_the_measure(ctx, device_lists, L):
    """The four flag kernels and the measure kernels check each other on the same device list: the survivors of
    drop_composition, drop_structure, drop_tm and drop_background are exactly the candidates whose measured value
    passes the tie of the rule, and the dropped counts are the sums of their multiplicities."""
    from catch_amd import engine
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.filter.composition_filter import CompositionFilter
    from catch_amd.filter.tm_filter import TmFilter
    targets, concat, base, (pos0, mult0, grp0, strs0) = device_lists(L)
    tf = TmFilter()
    bf = BackgroundFilter(["".join(strs0[:40])], kmer=12)
    index = bf._device_index(ctx)

    def check(drop_mask, call, label):
        c = engine.Candidates(ctx, targets, L, L)
        try:
            dropped = call(c)
            assert c.positions().tolist() == pos0[~drop_mask].tolist(), label
            assert c.multiplicities().tolist() == mult0[~drop_mask].tolist(), label
            return dropped
        finally:
            c.close()
    try:
        tm_c = base.measure(what="tm", tm=(tf._q(L), tf.offset_c), values=True, histograms=False)["tm_c"].astype(np.int64)
        hits = base.measure(what="hits", index=index, values=True, histograms=False)["hits"].astype(np.int64)
        seen = collections.Counter()
        for P in PS:
            v = base.measure(what="structure", min_loop=P, values=True, histograms=False)
            stem, dimer = v["stem"].astype(np.int64), v["dimer"].astype(np.int64)
            for K in KS:
                d = check(stem > K, lambda c: c.drop_structure(K, P, -1), ("stem", K, P))
                assert d == [int(mult0[stem > K].sum()), 0, int(mult0[stem > K].sum())]
                seen["stem", bool((stem > K).any())] += 1
            for D in DS if P == 3 else ():
                d = check(dimer > D, lambda c: c.drop_structure(-1, 3, D), ("dimer", D))
                assert d == [0, int(mult0[dimer > D].sum()), int(mult0[dimer > D].sum())]
                both = (stem > 3) | (dimer > D)
                d = check(both, lambda c: c.drop_structure(3, 3, D), ("both", D))
                assert d == [int(mult0[stem > 3].sum()), int(mult0[dimer > D].sum()), int(mult0[both].sum())]
        v = base.measure(what="composition", dust_window=64, values=True, histograms=False)
        gc, run, dust = (v[name].astype(np.int64) for name in FIVE[:3])
        for H in (1, 3, 6):
            d = check(run > H, lambda c: c.drop_composition(max_run=H), ("homopolymer", H))
            assert d == [0, int(mult0[run > H].sum()), 0, int(mult0[run > H].sum())]
        for X in (0, 20, 60):
            d = check(dust > X, lambda c: c.drop_composition(dust_x10=X, dust_window=64), ("dust", X))
            assert d == [0, 0, int(mult0[dust > X].sum()), int(mult0[dust > X].sum())]
            seen["dust", bool((dust > X).any()), bool((dust <= X).any())] += 1
        for gc_range in (("0.4", "0.6"), ("1/3", "1")):
            lo, hi = CompositionFilter(gc_range=gc_range)._gc_bounds(L)
            out = (gc < lo) | (gc > hi)
            d = check(out, lambda c: c.drop_composition(gc_lo=lo, gc_hi=hi), ("gc", gc_range))
            assert d == [int(mult0[out].sum()), 0, 0, int(mult0[out].sum())] and out.any() and not out.all()
        lo_c, hi_c = 6000, 8000
        out = (tm_c < lo_c) | (tm_c > hi_c)
        d, _ = check(out, lambda c: c.drop_tm(tf._q(L), tf.offset_c, lo_c, hi_c, histogram=False), "tm")
        assert d == [int(mult0[tm_c < lo_c].sum()), int(mult0[tm_c > hi_c].sum()), int(mult0[out].sum())] and out.any() and not out.all()
        for H in (0, 5):
            d, _ = check(hits > H, lambda c: c.drop_background(index, H, histogram=False), ("hits", H))
            assert d == int(mult0[hits > H].sum()) and (hits > H).any() and not (hits > H).all()
        assert seen["stem", True] >= 3 and seen["dust", True, True] >= 2, seen
    finally:
        bf.close()


@pytest.mark.gpu
def test_measure_kernel_grouped_empty_and_errors(ctx):
    """Three groups, the first and third sharing strings; then an empty list, an empty mask, the bad arguments
    (CATCHHIP_EINVAL, a ValueError here), an index built on another context of the device and the call after a
    near-duplicate filter."""
    from catch_amd import engine
    q = Q()
    L = 40
    rng = random.Random(9)
    pool = ["".join(rng.choice("ACGT") for _ in range(L)) for _ in range(500)]
    genomes = [["".join(pool[:300])], ["".join("AC" * (L // 2) for _ in range(50))], ["".join(pool[200:])]]
    concat = "".join(s for g in genomes for s in g)
    targets = engine.Targets(ctx, genomes)
    try:
        targets.set_groups(np.arange(3))
        c = engine.Candidates(ctx, targets, L, L)
        pos0, mult0, grp0, strs0 = _snapshot(c, concat, L)
        assert set(grp0.tolist()) == {0, 1, 2} and mult0.max() == 50
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        got = c.measure(min_loop=3, dust_window=16, values=True, histograms=True)
        want = q.measure_equal_length(strs0, L, 3, 16)
        for k, name in enumerate(FIVE):
            assert got[name].tolist() == want[:, k].tolist(), name
            assert got["histograms"][name].tolist() == _hist_of(want[:, k], mult0.astype(np.float64)).tolist(), name
        prof = q.QualityProfile(3, 16)
        prof._apply_to_candidates(c)
        prof._apply_to_candidates(c)
        assert prof.histograms.tolist() == [(2 * got["histograms"][name]).tolist() for name in FIVE]
        pos, mult, grp, _ = _snapshot(c, concat, L)
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (pos0.tolist(), mult0.tolist(), grp0.tolist())
        # an empty mask is valid and computes nothing
        none = c.measure(what=(), values=True, histograms=True)
        assert none == {"histograms": {}}
        assert c.measure(what=(), min_loop=-5, dust_window=1, values=False, histograms=False) == {}
        for bad in (dict(min_loop=-1), dict(dust_window=2), dict(dust_window=257)):
            with pytest.raises(ValueError, match="candidates_measure"):
                c.measure(**bad)
        assert sorted(c.measure(what="composition", min_loop=-1, values=True, histograms=False)) == sorted(FIVE[:3])
        assert sorted(c.measure(what="structure", dust_window=0, values=True, histograms=False)) == sorted(FIVE[3:])
        with pytest.raises(ValueError, match="q must be"):
            c.measure(what="tm", tm=(-8199, 27315), values=True)
        for bad in (dict(what="tm"), dict(what="hits"), dict(what="gc"), dict(what=("structure", "dust"))):
            with pytest.raises(ValueError, match="measure"):
                c.measure(**bad)
        # an index built on another context of the same device serves
        other = engine.Context(ctx.device)
        index = engine.KmerIndex(other, [concat[:2000]], 10)
        other.close()
        try:
            hits = c.measure(what="hits", index=index, values=True, histograms=False)["hits"]
            assert hits[:20].tolist() == [L - 9] * 20 and (hits == 0).any()
        finally:
            index.close()
        c.close()
    finally:
        targets.close()
    targets = engine.Targets(ctx, [["AT" * 400]])
    try:
        c = engine.Candidates(ctx, targets, L, L // 2)
        n = c.n
        got = c.measure(values=True, histograms=True)
        assert got["dimer"].tolist() == [L] * n and got["histograms"]["dimer"][L] == c.ncandidates
        c.ndf_hamming(np.arange(10, dtype=np.int32).reshape(1, 10), 0)
        with pytest.raises(ValueError, match="near-duplicate filter was already applied"):
            c.measure()
        c.close()
        # an empty list: every candidate is (AT)20, which the self-dimer rule drops
        e = engine.Candidates(ctx, targets, L, L // 2)
        assert e.drop_structure(-1, 3, 1)[1] == e.ncandidates and e.n == 0
        got = e.measure(values=True, histograms=True)
        assert all(got[name].size == 0 for name in FIVE) and all(not got["histograms"][name].any() for name in FIVE)
        assert e.measure(what=("tm",), tm=(-100000, 27315), values=True, histograms=False)["tm_c"].size == 0
        e.close()
    finally:
        targets.close()


# ------------------------------------------------------------------ the command line
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
GRID_BASE = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", "out"]


def _write_records(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _report_inputs(tmp_path, lengths=(2, 40, 100, 300)):
    rng = random.Random(2)
    recs = [("p%d" % i, "".join(rng.choice("ACGT") for _ in range(L))) for i, L in enumerate(list(lengths) * 3)]
    recs += [("one", "G"), ("lower", "acgtacgtacgtacgtacgt"), ("hairpin", "ACCACACCAGG" + "xxx" + "CCTGGTGTGGT"),
             ("two n", "ACGTNNACGT" * 4), ("again", recs[1][1]), ("at", "AT" * 20), ("poly", "A" * 40)]
    probes = _write_records(tmp_path / "probes.fasta", recs)
    bg = _write_records(tmp_path / "bg.fasta", [("b", recs[3][1][:150] + "NN" + _revcomp(recs[2][1][10:60]))])
    return recs, probes, bg


THRESHOLDS = ["--filter-gc", "0.3", "0.6", "--max-homopolymer", "5", "--filter-low-complexity", "60",
              "--max-hairpin-stem", "9", "--hairpin-min-loop", "3", "--max-self-dimer", "11", "--filter-tm", "40", "85",
              "--background-max-hits", "0"]


def test_probe_report_on_the_host_path(tmp_path, monkeypatch, capsys):
    """probe_report end to end under CATCHHIP_HOST_FRONT_END=1: lengths 1, 2, 40, 100, 300, lower case, a duplicate; every
    cell against the definitions, the verdicts against the ties, the kept and failed files."""
    from catch_amd import probe_report
    from catch_amd.filter.background_filter import BackgroundFilter
    from catch_amd.filter.composition_filter import CompositionFilter
    from catch_amd.filter.tm_filter import TmFilter
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    recs, probes, bg = _report_inputs(tmp_path)
    out, kept, failed = (str(tmp_path / n) for n in ("r.tsv", "kept.fasta", "failed.fasta"))
    argv = ["-f", probes, "-o", out, "--background", bg, "--background-kmer", "12", "--low-complexity-window", "32",
            "--tm-sodium", "100", "--write-kept", kept, "--write-failed", failed] + THRESHOLDS
    probe_report.main(probe_report.parse_args(argv))
    rows = [line.split("\t") for line in open(out).read().splitlines()]
    assert rows[0] == ["probe", "length", "gc", "homopolymer", "dust", "stem", "dimer", "tm_c", "background_hits", "verdict"]
    assert [r[0] for r in rows[1:]] == [h for h, _ in recs]
    tf = TmFilter(tm_range=("40", "85"), sodium_mm="100")
    bf = BackgroundFilter(list(__import__("catch_amd.utils.seq_io", fromlist=["x"]).read_fasta(bg).values()), kmer=12)
    verdicts = collections.Counter()
    for (h, s), r in zip(recs, rows[1:]):
        five = Q().measure(s, 3, 32)
        tm = tf._tm_c(s)
        assert r[1:7] == [str(len(s))] + [str(v) for v in five], h
        assert r[7] == ("NA" if tm is None else str(tm)) and r[8] == str(bf._hits(s)), h
        lo, hi = CompositionFilter(gc_range=("0.3", "0.6"))._gc_bounds(len(s))
        want = [name for name, bad in (
            ("gc", not lo <= five[0] <= hi), ("homopolymer", five[1] > 5), ("low-complexity", five[2] > 60),
            ("hairpin", five[3] > 9), ("self-dimer", five[4] > 11), ("tm", tf._side(tm) != 0),
            ("background", bf._hits(s) > 0)) if bad]
        assert r[9] == (",".join(want) if want else "ok"), (h, r)
        for name in want or ["ok"]:
            verdicts[name] += 1
    assert all(verdicts[name] >= 1 for name in probe_report.RULES + ("ok",)), verdicts
    assert dict(zip(*[[r[0] for r in rows[1:]], [r[7] for r in rows[1:]]]))["one"] == "NA"
    ok = [rec for rec, r in zip(recs, rows[1:]) if r[9] == "ok"]
    assert probe_report.read_records(kept) == ok and len(ok) + len(probe_report.read_records(failed)) == len(recs)
    assert capsys.readouterr().out == "%d records, %d pass\n" % (len(recs), len(ok))
    # without thresholds and without a background: no verdict, NA hits, the report on standard output
    probe_report.main(probe_report.parse_args(["-f", probes]))
    printed = capsys.readouterr()
    lines = printed.out.splitlines()
    assert lines[0].split("\t")[-1] == "background_hits" and len(lines) == len(recs) + 1
    assert all(line.split("\t")[8] == "NA" for line in lines[1:]) and printed.err == "%d records\n" % len(recs)
    assert [line.split("\t")[2:7] for line in lines[1:]] == [[str(v) for v in Q().measure(s)] for _, s in recs]


def test_options_parse_and_refuse_bad_values(capsys, tmp_path, monkeypatch):
    from catch_amd import design, design_grid, probe_report
    for parse, base in ((design.parse_args, ["x.fasta"]), (design_grid.parse_args, GRID_BASE)):
        a = parse(base)
        assert a.write_candidate_profile is None and Q().from_args(a) is None
        a = parse(base + ["--write-candidate-profile", "p.tsv"])
        assert (Q().from_args(a).min_loop, Q().from_args(a).dust_window) == (3, 64)
        # the loop and the window become legal with the option; without it today's errors stay
        a = parse(base + ["--write-candidate-profile", "p.tsv", "--hairpin-min-loop", "7", "--low-complexity-window", "16"])
        assert (Q().from_args(a).min_loop, Q().from_args(a).dust_window) == (7, 16)
        for bad in (["--hairpin-min-loop", "3"], ["--write-candidate-profile"],
                    ["--write-candidate-profile", "p", "--hairpin-min-loop", "-1"],
                    ["--write-candidate-profile", "p", "--low-complexity-window", "2"]):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert "error:" in capsys.readouterr().err, bad
    assert design.parse_args(["x.fasta", "--write-probe-report", "r.tsv"]).write_probe_report == "r.tsv"
    with pytest.raises(SystemExit):
        design_grid.parse_args(GRID_BASE + ["--write-probe-report", "r.tsv"])
    capsys.readouterr()
    ok = probe_report.parse_args(["-f", "p.fasta"] + THRESHOLDS[:-2])
    assert ok.max_hairpin_stem == 9 and ok.write_report is None
    for bad in ([], ["-f", "p", "--write-kept", "k"], ["-f", "p", "--write-failed", "k"], ["-f", "p", "--filter-gc", "0.7", "0.2"],
                ["-f", "p", "--filter-gc", "x", "1"], ["-f", "p", "--max-homopolymer", "0"], ["-f", "p", "--filter-low-complexity", "-1"],
                ["-f", "p", "--low-complexity-window", "2"], ["-f", "p", "--max-hairpin-stem", "0"], ["-f", "p", "--hairpin-min-loop", "-1"],
                ["-f", "p", "--max-self-dimer", "0"], ["-f", "p", "--filter-tm", "90", "40"], ["-f", "p", "--tm-sodium", "0"],
                ["-f", "p", "--tm-formamide", "101"], ["-f", "p", "--background-kmer", "12"], ["-f", "p", "--background-max-hits", "1"],
                ["-f", "p", "--background", "b", "--background-kmer", "7"], ["-f", "p", "--background", "b", "--background-max-hits", "-1"],
                ["-f", "p", "--write-tm-histogram", "h"], ["-f", "p", "--background", "b", "--write-background-histogram", "h"]):
        with pytest.raises(SystemExit):
            probe_report.parse_args(bad)
        assert "error:" in capsys.readouterr().err, bad
    # the profile stands right after the poly(A) filter and before the composition filter, and the strings path takes it
    from catch_amd.filter import probe_designer
    made = []
    monkeypatch.setattr(probe_designer.ProbeDesigner, "design", lambda self: made.append(self) or setattr(self, "final_probes", []))
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    prof = str(tmp_path / "p.tsv")
    design.main(design.parse_args([fa, "-o", str(tmp_path / "o.fasta"), "--filter-polya", "12", "2", "--filter-from-fasta", fa,
                                   "--max-homopolymer", "6", "--max-self-dimer", "11", "--write-candidate-profile", prof]))
    pd = made[0]
    assert [type(f).__name__ for f in pd.filters] == [
        "FastaFilter", "PolyAFilter", "QualityProfile", "CompositionFilter", "StructureFilter", "DuplicateFilter", "SetCoverFilter"]
    assert pd._strings_path_ok(pd.filters) and pd._strings_prefix(pd.filters) == 7
    assert open(prof).read() == "quantity\tvalue\tcandidates\tcandidates_above\n"
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    assert pd._device_front_end_mode(pd.genomes, pd.filters[5], pd.filters[6], pd.filters[1:5]) == "per group"
    assert pd._device_front_end_mode(pd.genomes, pd.filters[5], pd.filters[6], pd.filters[:5]) is None
    capsys.readouterr()


def _run_design(argv, seed, capsys):
    from catch_amd import design
    random.seed(seed)
    np.random.seed(seed)
    capsys.readouterr()
    pb = design.main(design.parse_args(argv))
    return pb, capsys.readouterr().out


def _ebola_records(n):
    import gzip
    recs = []
    with gzip.open(EBOLA, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if len(recs) == n:
                    break
                recs.append([line[1:], ""])
            else:
                recs[-1][1] += line
    return recs


def _profile_of_windows(seqs, L, stride, P=3, W=64):
    """The profile file's rows from the definition's NumPy form over the sliding windows of the sequences."""
    from catch_amd.filter import candidate_probes
    cands = candidate_probes.candidate_strings_from_sequences(seqs, L, stride)
    prof = Q().QualityProfile(P, W)
    prof._filter_strs(cands)
    return prof, len(cands)


@pytest.mark.gpu
def test_design_writes_the_candidate_profile(tmp_path, monkeypatch, capsys):
    """--write-candidate-profile on the first 5 Ebola genomes: the device front end and the host front end write the
    same file, so do the duplicate filter and --filter-with-lsh-hamming 2, the file is the definition's over the sliding
    windows, and the probes are those of a run without the option."""
    from catch_amd import engine
    plain = [EBOLA, "--limit-target-genomes", "5"] + BASE
    calls = []
    real = engine.Candidates.measure
    monkeypatch.setattr(engine.Candidates, "measure", lambda self, *a, **k: calls.append(self.n) or real(self, *a, **k))
    files = {}
    for front, extra in (("device", []), ("host", []), ("hamming", ["--filter-with-lsh-hamming", "2"])):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        before = len(calls)
        out, prof = tmp_path / (front + ".fasta"), tmp_path / (front + ".tsv")
        _run_design(plain + extra + ["-o", str(out), "--write-candidate-profile", str(prof), "--max-self-dimer", "12"], 5, capsys)
        assert len(calls) - before == (0 if front == "host" else 1), front        # one measure call per candidate list
        files[front] = (prof.read_text(), open(out).read())
        without = tmp_path / (front + ".plain.fasta")
        _run_design(plain + extra + ["-o", str(without), "--max-self-dimer", "12"], 5, capsys)
        assert open(without).read() == files[front][1], front
    assert files["device"][0] == files["host"][0] == files["hamming"][0]
    assert files["device"][1] == files["host"][1]
    want, ncand = _profile_of_windows([s for _, s in _ebola_records(5)], 100, 50)
    path = tmp_path / "want.tsv"
    want.write_profile(str(path))
    assert files["device"][0] == path.read_text() and ncand > 1500
    rows = [line.split("\t") for line in files["device"][0].splitlines()[1:]]
    assert [q for q, _ in __import__("itertools").groupby(r[0] for r in rows)] == list(FIVE)
    for name in FIVE:
        mine = [r for r in rows if r[0] == name]
        assert sum(int(r[2]) for r in mine) == ncand and int(mine[0][2]) + int(mine[0][3]) == ncand and len(mine) >= 4
    # the README's structure tables come out of this one file: what --max-self-dimer 12 drops is its candidates_above
    structure = [f for f in _run_design(plain + ["-o", str(tmp_path / "x.fasta"), "--max-self-dimer", "12"], 5, capsys)[0].filters
                 if type(f).__name__ == "StructureFilter"][0]
    assert structure.dropped[1] == int([r for r in rows if r[0] == "dimer" and r[1] == "12"][0][3]) > 0


@pytest.mark.gpu
def test_design_grid_counts_a_dataset_once(tmp_path, capsys):
    from catch_amd import design_grid
    fa = _write_records(tmp_path / "ebola5.fasta", _ebola_records(5))
    prof = tmp_path / "p.tsv"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "1", "2", "--grid-cover-extension", "0", "-o", str(tmp_path / "out"),
                                             "-pl", "100", "-ps", "50", "--write-candidate-profile", str(prof),
                                             "--hairpin-min-loop", "0", "--low-complexity-window", "16"]))
    capsys.readouterr()
    want, ncand = _profile_of_windows([s for _, s in _ebola_records(5)], 100, 50, 0, 16)
    path = tmp_path / "want.tsv"
    want.write_profile(str(path))
    assert prof.read_text() == path.read_text() and int(want.histograms[0].sum()) == ncand


@pytest.mark.gpu
def test_probe_report_device_equals_host_and_design_writes_it(tmp_path, monkeypatch, capsys):
    """probe_report on a FASTA of mixed lengths with a background, device path against host path; and design
    --add-adapters --write-probe-report against probe_report -f on the FASTA it wrote, byte for byte."""
    from catch_amd import engine, probe_report
    recs, probes, bg = _report_inputs(tmp_path)
    calls = []
    real = engine.Candidates.measure
    monkeypatch.setattr(engine.Candidates, "measure", lambda self, *a, **k: calls.append(self.L) or real(self, *a, **k))
    argv = ["-f", probes, "--background", bg, "--background-kmer", "12", "--tm-formamide", "20"] + THRESHOLDS
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    probe_report.main(probe_report.parse_args(argv + ["-o", str(tmp_path / "device.tsv")]))
    assert sorted(calls) == [2, 20, 25, 40, 100, 300]            # one call per length of 2 and more
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    probe_report.main(probe_report.parse_args(argv + ["-o", str(tmp_path / "host.tsv")]))
    assert len(calls) == 6
    text = (tmp_path / "device.tsv").read_text()
    assert text == (tmp_path / "host.tsv").read_text() and text.count("\n") == len(recs) + 1
    assert any(line.endswith("\tok") for line in text.splitlines()) and "background" in text
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    capsys.readouterr()
    out, rep = tmp_path / "probes.out.fasta", tmp_path / "design.tsv"
    options = ["--max-hairpin-stem", "9", "--filter-gc", "0.3", "0.6", "--low-complexity-window", "32"]
    _run_design([EBOLA, "--limit-target-genomes", "5"] + BASE + ["--add-adapters", "-o", str(out), "--write-probe-report", str(rep)]
                + options, 5, capsys)
    probe_report.main(probe_report.parse_args(["-f", str(out), "-o", str(tmp_path / "again.tsv")] + options))
    assert rep.read_text() == (tmp_path / "again.tsv").read_text()
    rows = [line.split("\t") for line in rep.read_text().splitlines()]
    assert len(rows) - 1 == len(probe_report.read_records(str(out))) > 50 and all(r[1] == "140" for r in rows[1:])
    assert rows[0][-1] == "verdict" and {r[-1] for r in rows[1:]} >= {"ok"}
