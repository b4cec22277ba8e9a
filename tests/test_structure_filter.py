"""The secondary-structure filters of the design command -- hairpin stems and self-dimers (--max-hairpin-stem,
--hairpin-min-loop, --max-self-dimer; not in the reference).  The rule exists three times in
catch_amd/filter/structure_filter.py: _keeps (the definition: the oracle), the NumPy form of the host path and the
kernel of the device front end (catchhip_candidates_drop_structure).  Here: the quantifiers of the definition, word for
word, and hand-made cases against _keeps; NumPy against _keeps; the kernel against _keeps, candidate by candidate; and
the design command on both front ends.

A rule whose shortest structure does not fit the candidates (L < 2 K + 2 + P, L < D + 1) can drop nothing: those cases
assert that it drops exactly nothing.  Every other case asserts that _keeps itself drops and keeps at least one
candidate through each rule that is on, so that a kernel that flags nothing, or everything, cannot pass."""
import collections
import functools
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")
BASE = ["-pl", "100", "-ps", "50", "-m", "2", "-e", "50"]
# of the 1,888 candidates of the first 5 genomes _keeps drops some through each rule at these values (asserted below)
EBOLA_OPTIONS = ["--max-hairpin-stem", "9", "--max-self-dimer", "11"]
PARTNER = dict(A="T", C="G", G="C", T="A")


def SF(*a, **k):
    from catch_amd.filter.structure_filter import StructureFilter
    return StructureFilter(*a, **k)


def _revcomp(u):
    return "".join(PARTNER[c] for c in reversed(u))


# ------------------------------------------------------------------ the definition, word for word
def _pairs(s, x, y):
    return s[x] in PARTNER and s[y] == PARTNER[s[x]]


def _literal(s, K, P, D):
    """(hairpin, self-dimer) by the quantifiers of the rules as they are stated, nothing rearranged."""
    L = len(s)
    hairpin = K is not None and any(
        all(_pairs(s, i + t, j - t) for t in range(K + 1)) and (j - K) - (i + K) - 1 >= P
        for i in range(L) for j in range(i + 1, L) if i + K < L and j - K >= 0)
    dimer = D is not None and any(
        all(_pairs(s, a + t, b - t) for t in range(D + 1))
        for a in range(L) for b in range(L) if a + D <= L - 1 and b - D >= 0)
    return hairpin, dimer


def test_definition_equals_its_quantifiers():
    """_fails looks for an arm's reverse complement with str.find; the rules are stated with quantifiers over positions."""
    rng = random.Random(11)
    seen = collections.Counter()
    for _ in range(1500):
        L = rng.randrange(0, 27)
        s = "".join(rng.choice(rng.choice(["AT", "ACGT", "ACGTN", "ACGTNa-"])) for _ in range(L))
        K, P, D = rng.choice([1, 2, 3, 5]), rng.choice([0, 1, 3, 7]), rng.choice([1, 2, 3, 4, 7])
        got = SF(K, P, D)._fails(s)
        assert got == _literal(s, K, P, D), (s, K, P, D)
        seen[got] += 1
        assert got[1] or not got[0] or D > K          # every hairpin stem is a self-dimer stretch too
    assert min(seen.get(k, 0) for k in ((False, False), (True, True), (False, True), (True, False))) > 20, seen


# ------------------------------------------------------------------ host: the definition, by hand
def test_tightest_hairpin_and_loop_one_short():
    for K, P in ((1, 0), (1, 3), (3, 3), (4, 1), (9, 7), (2, 5)):
        arm = ("ACCAACACCA" * 2)[:K + 1]                     # A and C only: the arm pairs with nothing of itself
        s = arm + "N" * P + _revcomp(arm)
        assert len(s) == 2 * K + 2 + P
        f = SF(max_hairpin_stem=K, hairpin_min_loop=P)
        assert f._fails(s) == (True, False) and not f._keeps(s)
        if P:
            assert f._keeps(arm + "N" * (P - 1) + _revcomp(arm))          # the same arms, one character too close
            assert f._keeps(arm + "N" * (P - 1) + _revcomp(arm) + "N")    # (not for being shorter)
        assert f._keeps(s[:-1] + "N") and f._keeps("N" + s[1:])           # a pair less
        assert SF(max_hairpin_stem=K + 1, hairpin_min_loop=P)._keeps(s)
        assert not SF(max_hairpin_stem=K, hairpin_min_loop=P)._keeps("NN" + s + "N")
        assert SF(max_hairpin_stem=K, hairpin_min_loop=P + 1)._keeps(s)
    # a longer loop is fine, and the stem's outer ends may be positions 0 and L - 1
    s = "ACCA" + "N" * 40 + "TGGT"
    assert not SF(max_hairpin_stem=3)._keeps(s) and SF(max_hairpin_stem=4)._keeps(s)
    assert SF(max_hairpin_stem=3)._fails(s) == (True, False)
    assert not SF(max_hairpin_stem=3, hairpin_min_loop=40)._keeps(s) and SF(max_hairpin_stem=3, hairpin_min_loop=41)._keeps(s)


def test_n_and_lower_case_break_an_arm():
    s = "ACCAC" + "NNNN" + "GTGGT"
    f = SF(max_hairpin_stem=4, max_self_dimer=4)
    assert f._fails(s) == (True, True)
    for at in (0, 2, 4, 9, 11, 13):
        for c in ("N", s[at].lower(), "-", "U"):
            broken = s[:at] + c + s[at + 1:]
            assert f._fails(broken) == (False, False), broken
    assert f._keeps(s.lower()) and f._keeps("N" * 30) and f._keeps("acgt" * 10)
    # a mismatch inside, too: the stretch is of consecutive pairs
    assert f._keeps("ACCAC" + "NNNN" + "GTTGT") and SF(max_hairpin_stem=1)._fails("ACCAC" + "NNNN" + "GTTGT")[0]


def test_adjacent_arms_with_no_loop():
    f0, f1 = SF(max_hairpin_stem=1, hairpin_min_loop=0), SF(max_hairpin_stem=1, hairpin_min_loop=1)
    assert not f0._keeps("ACGT") and f1._keeps("ACGT")               # AC | GT, nothing between
    assert not f0._keeps("NNACGTNN") and f1._keeps("NNACGTNN")
    assert not f1._keeps("ACNGT") and f0._keeps("ACG") and f0._keeps("CGT")
    assert SF(max_hairpin_stem=2, hairpin_min_loop=0)._keeps("ACGT")   # L = 4 < 2 K + 2
    assert not SF(max_hairpin_stem=2, hairpin_min_loop=0)._keeps("AACGTT")


def test_self_dimer_by_hand():
    assert not SF(max_self_dimer=3)._keeps("ACGT") and SF(max_self_dimer=4)._keeps("ACGT")      # one stretch of 4
    assert SF(max_self_dimer=3)._fails("ACGT") == (False, True)
    # a stretch that is no hairpin: GAATTC pairs with itself end to end, its arms overlap
    s = "NNGAATTCNN"
    assert not SF(max_self_dimer=5)._keeps(s) and SF(max_self_dimer=6)._keeps(s)
    assert SF(max_hairpin_stem=5, hairpin_min_loop=0)._keeps(s) and SF(max_hairpin_stem=3, hairpin_min_loop=0)._keeps(s)
    assert not SF(max_hairpin_stem=2, hairpin_min_loop=0)._keeps(s)           # GAA | TTC
    # odd length: the middle character would pair with itself, which never holds
    assert SF(max_self_dimer=2)._keeps("NACTGTN") and SF(max_self_dimer=1)._keeps("NGATCN") is False
    assert SF(max_self_dimer=4)._keeps("GACGTC") is False and SF(max_self_dimer=4)._keeps("GACNGTC")
    # two separate places: a and b are unrelated
    s = "AACCA" + "N" * 20 + "TGGTT"
    assert SF(max_self_dimer=4)._fails(s) == (False, True) and SF(max_self_dimer=5)._keeps(s)
    # with D < K the hairpin rule adds nothing
    rng = random.Random(5)
    for _ in range(300):
        t = "".join(rng.choice("ACGT") for _ in range(40))
        fh, fd = SF(max_hairpin_stem=4, hairpin_min_loop=0, max_self_dimer=3)._fails(t)
        assert fd or not fh


def test_thresholds_beyond_the_length_and_tiny_strings():
    for L in (0, 1, 2, 3, 10):
        for s in ("AT" * L, "ACGT" * L, "A" * L + "T" * L):
            s = s[:L]
            for big in (L, L + 1, 10 ** 9):
                if big >= 1:
                    assert SF(max_hairpin_stem=big, hairpin_min_loop=0, max_self_dimer=big)._fails(s) == (False, False)
    f = SF(max_hairpin_stem=1, hairpin_min_loop=0, max_self_dimer=1)
    assert f._keeps("") and f._keeps("A") and f._keeps("N") and f._keeps("AA") and f._keeps("AC") and f._keeps("NN")
    assert f._fails("AT") == (False, True) and f._fails("CG") == (False, True) and f._fails("TA") == (False, True)
    assert f._filter_strs(["", "A", "AT", "AA", "", "GC"]) == ["", "A", "AA", ""] and f.dropped == [0, 2, 2]
    assert f._filter_strs(["AT", "AT", "AC", "AT"]) == ["AC"] and f.dropped == [0, 5, 5]
    assert f._filter_strs(["A", "T", "N"]) == ["A", "T", "N"] and f._filter_strs([]) == []


def test_arguments_are_validated():
    for bad in (dict(max_hairpin_stem=0), dict(max_hairpin_stem=-1), dict(max_hairpin_stem=2.5), dict(max_hairpin_stem="9"),
                dict(max_hairpin_stem=True), dict(hairpin_min_loop=-1), dict(hairpin_min_loop=1.5),
                dict(hairpin_min_loop=None), dict(max_self_dimer=0), dict(max_self_dimer=-4), dict(max_self_dimer="11")):
        with pytest.raises(ValueError):
            SF(**bad)
    f = SF(max_hairpin_stem=np.int64(9), hairpin_min_loop=0, max_self_dimer=11)
    assert (f.max_hairpin_stem, f.hairpin_min_loop, f.max_self_dimer, f.dropped) == (9, 0, 11, [0, 0, 0])
    g = SF()
    assert (g.max_hairpin_stem, g.hairpin_min_loop, g.max_self_dimer) == (None, 3, None) and g._keeps("AT" * 200)
    assert SF(max_self_dimer=3, hairpin_min_loop=50)._fails("ACGT") == (False, True)      # P is idle without K


# ------------------------------------------------------------------ inputs
def _planted(rng, L, R, loop, start, filler="x"):
    """A stem of exactly R pairs -- an arm over A and C from `start`, `loop` fillers, its reverse complement -- in a
    background that pairs with nothing; None where it does not fit."""
    if start < 0 or start + 2 * R + loop > L:
        return None
    arm = "".join(rng.choice("AC") for _ in range(R))
    s = filler * start + arm + filler * loop + _revcomp(arm)
    return s + filler * (L - len(s))


KS, PS, DS = (1, 3, 9), (0, 3, 7), (1, 4, 12)


def _candidates(L):
    """2,000 candidates of L characters (400 beyond L = 300), a third of them duplicates: random over AT, ACGT, ACGTN (N isolated:
    two in a row would cut the window) and AC (no pairs at all), and stems of exactly K and K + 1 (D and D + 1) pairs
    planted at both ends of the candidate and across every 64-character boundary, with loops of P - 1 and P."""
    rng = random.Random(1000 + L)
    total = 2000 if L <= 300 else 400
    planted = []
    for R in sorted({x for K in KS for x in (K, K + 1)} | {x for D in DS for x in (D, D + 1)}):
        for loop in sorted({p for P in PS for p in (P - 1, P) if p >= 0}):
            span = 2 * R + loop
            starts = {0, L - span} | {b - R // 2 for b in range(64, L, 64)} | {b - R - loop - R // 2 for b in range(64, L, 64)}
            for start in sorted(starts):
                s = _planted(rng, L, R, loop, start, rng.choice("xn-"))
                if s is not None:
                    planted.append(s)
    rng.shuffle(planted)
    planted = planted[:total // 3]
    out = list(planted)
    nrandom = max(total * 2 // 3 - len(out), total // 3)
    for k in range(nrandom):
        alpha = ("AT", "ACGT", "ACGTN", "AC", "ACGTNNNN")[k % 5]
        s = "".join(rng.choice(alpha) for _ in range(L))
        out.append(re.sub("NN", "Nn", re.sub("NN", "Nn", s)))
    out += [rng.choice(out) for _ in range(total - len(out))]           # duplicates, for the multiplicities
    rng.shuffle(out)
    assert not any("NN" in s for s in out) and all(len(s) == L for s in out)
    return out


@functools.lru_cache(maxsize=None)
def _unique(L):
    c = collections.Counter(_candidates(L))
    return tuple(sorted(c)), c


@functools.lru_cache(maxsize=None)
def _oracle(L, rule, a, b=0):
    """_fails of one rule over the unique candidates of length L, as a dict: computed once per (L, rule, thresholds)."""
    f = SF(max_hairpin_stem=a, hairpin_min_loop=b) if rule == "hairpin" else SF(max_self_dimer=a)
    k = 0 if rule == "hairpin" else 1
    return {s: f._fails(s)[k] for s in _unique(L)[0]}


def _can_fire(L, K=None, P=3, D=None):
    return K is not None and L >= 2 * K + 2 + P, D is not None and L >= D + 1


def _expected(L, K, P, D):
    """({candidate: (hairpin, self-dimer)}, non-vacuous or exactly idle: asserted)"""
    hair = _oracle(L, "hairpin", K, P) if K is not None else None
    dimer = _oracle(L, "dimer", D) if D is not None else None
    uniq = _unique(L)[0]
    for name, table, can in (("hairpin", hair, _can_fire(L, K, P, D)[0]), ("dimer", dimer, _can_fire(L, K, P, D)[1])):
        if table is None:
            continue
        dropped = sum(table.values())
        if can:
            assert 1 <= dropped <= len(uniq) - 1, (name, L, K, P, D, dropped, len(uniq))
        else:
            assert dropped == 0, (name, L, K, P, D)
    return {s: (bool(hair and hair[s]), bool(dimer and dimer[s])) for s in uniq}


LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300]
# the kernel's workgroup by candidate length (csrc/structure.hip): 6 W + 7 words of LDS per candidate, W = ceil(L / 32);
# as many of 256 / 128 / 64 candidates as fit 64 KB, and the planes in global memory when 64 do not
TIER_EDGES = [288, 289, 640, 641, 1312, 1313]


def _structure_workgroup(L):
    """(candidates per workgroup, bytes of dynamic LDS) of the kernel's launch; (256, 0): planes in global memory."""
    per = (6 * ((L + 31) // 32) + 7) * 4
    for rows in (256, 128, 64):
        if rows * per <= 65536:
            return rows, rows * per
    return 256, 0


def test_tier_edges_sit_on_the_workgroup_sizes_claimed():
    assert [_structure_workgroup(L) for L in TIER_EDGES] == [
        (256, 62464), (128, 34304), (128, 65024), (64, 34048), (64, 64768), (256, 0)]
    assert all(_structure_workgroup(L)[0] == 256 for L in LENGTHS[:-1]) and _structure_workgroup(300)[0] == 128
RULE_SETS = {
    "hairpin": [(K, P, None) for K in KS for P in PS],
    "dimer": [(None, 3, D) for D in DS],
    # both rules in one launch: the pairs in step, D < K (the hairpin rule idle), and the extremes crossed
    "both": [(1, 0, 1), (3, 3, 4), (9, 7, 12), (9, 3, 4), (1, 7, 12), (3, 0, 1)],
}


@pytest.mark.parametrize("L", [2, 3, 31, 33, 64, 100])
def test_kernel_test_inputs_are_not_vacuous(L):
    """No GPU: the alphabet and stems chosen for the kernel test drop and keep something through every rule that can
    fire at that length (the other lengths are checked where they run)."""
    uniq, counts = _unique(L)
    assert len(uniq) >= min(300, 4 ** L // 2) and sum(counts.values()) == 2000 and max(counts.values()) > 1
    assert sum(_unique(641)[1].values()) == 400
    for sets in RULE_SETS.values():
        for K, P, D in sets:
            _expected(L, K, P, D)
    assert _can_fire(3, 1, 0, 1) == (False, True) and _can_fire(31, 9, 7, 12) == (True, True)
    assert _can_fire(27, 9, 7) == (True, False) and _can_fire(26, 9, 7) == (False, False)


# ------------------------------------------------------------------ host: NumPy against the definition
@pytest.mark.parametrize("alphabet", ["AT", "ACGT", "ACGTN"])
def test_numpy_rule_equals_definition(alphabet):
    """_filter_strs (NumPy, equal lengths) against [s for s in strs if _keeps(s)] at every length 1 .. 70 and 100, 255,
    256, 257, and `dropped` against counts taken from _fails -- duplicates counted."""
    rng = random.Random(len(alphabet))
    hits = collections.Counter()
    for L in list(range(1, 71)) + [100, 255, 256, 257]:
        n = 60 if L <= 100 else 16
        strs = ["".join(rng.choice(alphabet) for _ in range(L)) for _ in range(n)]
        for R in (2, 4, 10):                 # and a few planted stems, so that the long thresholds see both answers
            s = _planted(rng, L, R, rng.choice([0, 2, 3, 7]), rng.randrange(0, max(1, L - 2 * R - 7)))
            strs += [s, s] if s else []
        settings = {"AT": ((5, 3, 9), (9, 0, 12), (12, 7, 5)), "ACGT": ((1, 0, 1), (3, 3, 4), (4, 7, 5), (9, 3, 12)),
                    "ACGTN": ((1, 3, 1), (2, 0, 3), (3, 7, 4), (9, 0, None), (None, 3, 12))}[alphabet]
        for K, P, D in settings:
            f = SF(max_hairpin_stem=K, hairpin_min_loop=P, max_self_dimer=D)
            fails = [f._fails(s) for s in strs]
            got = f._filter_strs(strs)
            assert got == [s for s, x in zip(strs, fails) if not any(x)], (L, K, P, D)
            assert f.dropped == [sum(x[0] for x in fails), sum(x[1] for x in fails), sum(any(x) for x in fails)]
            assert f._filter_strs(got) == got
            for x in fails:
                hits[x] += 1
    assert all(hits[k] > 100 for k in ((False, False), (True, True), (False, True))), hits


def test_numpy_rule_in_chunks_mixed_lengths_order_and_duplicates():
    from catch_amd import probe
    rng = random.Random(3)
    a = ["".join(rng.choice("ACGT") for _ in range(24)) for _ in range(3000)]
    a = a + a[:1500]                                             # more than one chunk of 4,096, a third duplicates
    rng.shuffle(a)
    kwargs = dict(max_hairpin_stem=3, hairpin_min_loop=3, max_self_dimer=4)
    f, g = SF(**kwargs), SF(**kwargs)
    got = f._filter_strs(a)
    want = [s for s in a if g._keeps(s)]
    assert got == want and 0.05 * len(a) < len(got) < 0.95 * len(a)       # order and duplicates as they came
    assert len(got) > len(set(got)) and f.dropped[2] == len(a) - len(got)
    fails = [g._fails(s) for s in a]
    assert f.dropped == [sum(x[0] for x in fails), sum(x[1] for x in fails), sum(any(x) for x in fails)]
    assert f.dropped[0] > 0 and f.dropped[1] > f.dropped[0] and f.dropped[2] < f.dropped[0] + f.dropped[1]
    # mixed lengths: string by string
    mixed = a[:400] + ["".join(rng.choice("ACGTN") for _ in range(rng.randrange(0, 60))) for _ in range(400)]
    rng.shuffle(mixed)
    f = SF(**kwargs)
    fails = [f._fails(s) for s in mixed]
    assert f._filter_strs(mixed) == [s for s, x in zip(mixed, fails) if not any(x)]
    assert f.dropped == [sum(x[0] for x in fails), sum(x[1] for x in fails), sum(any(x) for x in fails)]
    assert all(0.05 * len(mixed) < d < 0.95 * len(mixed) for d in f.dropped)
    # Probe objects: the same rule, counted the same way
    h = SF(**kwargs)
    probes = [probe.Probe.from_str(s) for s in mixed[:300] if s]
    left = h._filter(probes)
    assert [p.seq_str for p in left] == [p.seq_str for p in probes if h._keeps(p.seq_str)]
    assert h.dropped[2] == len(probes) - len(left) > 0 and h._filter([]) == []


# ------------------------------------------------------------------ host: the option surface
def _write_records(path, records):
    with open(path, "w") as f:
        for h, s in records:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


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


def _design_without_designing(monkeypatch, argv):
    """design.main up to ProbeDesigner.design: returns the designer it built."""
    from catch_amd import design
    from catch_amd.filter import probe_designer
    made = []

    def fake_design(self):
        made.append(self)
        self.final_probes = []
    monkeypatch.setattr(probe_designer.ProbeDesigner, "design", fake_design)
    design.main(design.parse_args(argv))
    return made[0]


GRID_BASE = ["a.fasta", "--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", "out"]


def _help_of(design):
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        design.parse_args(["--help"])
    return " ".join(buf.getvalue().split())


def test_options_parse_and_refuse_bad_values(capsys):
    from catch_amd import design, design_grid, design_large
    assert design_large.design is design
    for parse, base in ((design.parse_args, ["x.fasta"]), (design_grid.parse_args, GRID_BASE)):
        a = parse(base)
        assert (a.max_hairpin_stem, a.hairpin_min_loop, a.max_self_dimer) == (None, None, None)
        a = parse(base + ["--max-hairpin-stem", "9", "--hairpin-min-loop", "0", "--max-self-dimer", "11"])
        assert (a.max_hairpin_stem, a.hairpin_min_loop, a.max_self_dimer) == (9, 0, 11)
        assert parse(base + ["--max-self-dimer", "1"]).max_self_dimer == 1
        assert parse(base + ["--max-hairpin-stem", "1"]).hairpin_min_loop is None
        for bad in (["--max-hairpin-stem", "0"], ["--max-hairpin-stem", "-2"], ["--max-hairpin-stem", "2.5"],
                    ["--max-hairpin-stem", "9", "--hairpin-min-loop", "-1"], ["--hairpin-min-loop", "3"],
                    ["--hairpin-min-loop", "3", "--max-self-dimer", "11"], ["--max-self-dimer", "0"],
                    ["--max-self-dimer", "-1"], ["--max-self-dimer", "x"], ["--max-hairpin-stem"]):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert "error:" in capsys.readouterr().err, bad
    text = _help_of(design)
    for opt in ("--max-hairpin-stem", "--hairpin-min-loop", "--max-self-dimer"):
        assert opt in text


def test_from_args_builds_the_filter():
    from catch_amd import design
    from catch_amd.filter import structure_filter
    assert structure_filter.from_args(design.parse_args(["x.fasta"])) is None
    f = structure_filter.from_args(design.parse_args(["x.fasta", "--max-hairpin-stem", "9"]))
    assert (f.max_hairpin_stem, f.hairpin_min_loop, f.max_self_dimer) == (9, 3, None)
    f = structure_filter.from_args(design.parse_args(["x.fasta", "--max-self-dimer", "11", "--max-hairpin-stem", "8",
                                                      "--hairpin-min-loop", "5"]))
    assert (f.max_hairpin_stem, f.hairpin_min_loop, f.max_self_dimer) == (8, 5, 11)
    args = design.parse_args(["x.fasta"])
    args.max_self_dimer = 0
    with pytest.raises(ValueError, match="--max-self-dimer"):
        structure_filter.from_args(args)


def test_filter_order_and_strings_path(tmp_path, monkeypatch, capsys):
    fa = _write_records(tmp_path / "in.fasta", [("g%d" % i, "ACGT" * 30 + "ACGTA"[i:]) for i in range(5)])
    out = str(tmp_path / "o.fasta")
    every = ["--max-hairpin-stem", "9", "--hairpin-min-loop", "4", "--max-self-dimer", "11"]
    for first, name in ((["--filter-with-lsh-hamming", "0"], "NearDuplicateFilterWithHammingDistance"),
                        (["--filter-with-lsh-minhash", "0.6"], "NearDuplicateFilterWithMinHash"), ([], "DuplicateFilter")):
        pd = _design_without_designing(monkeypatch, [
            fa, "-o", out, "--add-adapters", "--filter-polya", "12", "2", "--filter-from-fasta", fa,
            "--max-homopolymer", "6"] + every + first)
        assert [type(f).__name__ for f in pd.filters] == [
            "FastaFilter", "PolyAFilter", "CompositionFilter", "StructureFilter", name, "SetCoverFilter", "AdapterFilter"]
        assert pd._strings_path_ok(pd.filters) and pd._strings_prefix(pd.filters) == 6
        sf = pd.filters[3]
        assert (sf.max_hairpin_stem, sf.hairpin_min_loop, sf.max_self_dimer) == (9, 4, 11)
    # either option adds ONE filter; without them the list is what it was
    for opts in (every[:2], every[:4], every[4:]):
        pd = _design_without_designing(monkeypatch, [fa, "-o", out] + opts)
        assert [type(f).__name__ for f in pd.filters] == ["StructureFilter", "DuplicateFilter", "SetCoverFilter"]
    assert pd.filters[0].max_hairpin_stem is None and pd.filters[0].max_self_dimer == 11
    pd = _design_without_designing(monkeypatch, [fa, "-o", out])
    assert [type(f).__name__ for f in pd.filters] == ["DuplicateFilter", "SetCoverFilter"]
    capsys.readouterr()


def test_strings_path_and_front_end_mode(tmp_path, monkeypatch):
    from catch_amd import genome
    from catch_amd.filter import probe_designer
    from catch_amd.filter.composition_filter import CompositionFilter
    from catch_amd.filter.duplicate_filter import DuplicateFilter
    from catch_amd.filter.fasta_filter import FastaFilter
    from catch_amd.filter.near_duplicate_filter import NearDuplicateFilterWithHammingDistance
    from catch_amd.filter.polya_filter import PolyAFilter
    from catch_amd.filter.set_cover_filter import SetCoverFilter
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    PD = probe_designer.ProbeDesigner
    sf, cf, paf, dup = SF(max_self_dimer=11), CompositionFilter(max_homopolymer=5), PolyAFilter(12, 2), DuplicateFilter()
    ff = FastaFilter(str(tmp_path / "none.fasta"))
    ndf = NearDuplicateFilterWithHammingDistance(2, 100)
    scf = SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=50)
    genomes = [[genome.Genome.from_one_seq("ACGT" * 100)]]
    pd = PD(genomes, [sf, dup, scf], probe_length=100, probe_stride=50)
    for filters in ([sf, dup, scf], [paf, cf, sf, ndf, scf], [ff, paf, cf, sf, dup, scf]):
        assert PD._strings_path_ok(filters), filters
    for filters in ([sf, dup], [sf, scf], [dup, sf, scf], [sf]):
        assert not PD._strings_path_ok(filters), filters
    plain = pd._device_front_end_mode(genomes, dup, scf)
    assert plain == "per group"
    assert pd._device_front_end_mode(genomes, dup, scf, [sf]) == plain
    assert pd._device_front_end_mode(genomes, dup, scf, [paf, cf, sf]) == plain
    assert pd._device_front_end_mode(genomes, ndf, scf, [sf]) == pd._device_front_end_mode(genomes, ndf, scf)
    many = [[genome.Genome.from_one_seq("ACGT" * 100)] for _ in range(9)]
    assert pd._device_front_end_mode(many, dup, scf, [sf]) == pd._device_front_end_mode(many, dup, scf) == "union"
    assert pd._device_front_end_mode(genomes, dup, scf, [ff, sf]) is None
    monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    assert pd._device_front_end_mode(genomes, dup, scf, [sf]) is None


def test_symbol_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib, engine
    name = "catchhip_candidates_drop_structure"
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    at = re.search(r"\b%s\s*\(" % name, hdr)
    assert at and "NOT IN THE REFERENCE" in hdr[:at.start()].rsplit("/*", 1)[1]
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 7
    assert hasattr(_lib.lib(), name)
    assert hasattr(engine.Candidates, "drop_structure")
    assert "structure.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------ GPU: the kernel against _keeps
def _snapshot(cands, concat, L):
    pos = cands.positions()
    return pos, cands.multiplicities().copy(), cands.groups().copy(), [concat[p:p + L] for p in pos.tolist()]


@pytest.fixture(scope="module")
def device_lists(ctx):
    """Per length: the targets (one sequence per candidate, stride = L: the windows are the candidates) and the
    unfiltered unique list, made once and shared by the three rule-set cases of that length."""
    from catch_amd import engine
    made = {}

    def get(L):
        if L not in made:
            seqs = _candidates(L)
            targets = engine.Targets(ctx, [[s] for s in seqs])
            base = engine.Candidates(ctx, targets, L, L)
            snap = _snapshot(base, "".join(seqs), L)
            base.close()
            made[L] = (targets, "".join(seqs), snap)
        return made[L]
    yield get
    for targets, _, _ in made.values():
        targets.close()


def _set_plane_budget(monkeypatch, L, rules):
    """At L = 1,313 and both rules: a plane buffer of 100 candidates, so that the list takes several launches."""
    if L == 1313 and rules == "both":
        monkeypatch.setenv("CATCHHIP_STRUCT_PLANE_BYTES", str(100 * _PLANE_BYTES_1313))


_PLANE_BYTES_1313 = (6 * 42 + 7) * 4


@pytest.mark.gpu
@pytest.mark.parametrize("rules", sorted(RULE_SETS))
@pytest.mark.parametrize("L", LENGTHS + TIER_EDGES)
def test_drop_structure_kernel_equals_definition(ctx, device_lists, monkeypatch, L, rules):
    """catchhip_candidates_drop_structure against _fails, candidate by candidate, for every (K, P, D) of the rule set:
    the surviving positions, multiplicities and groups are the unfiltered list's, masked, and the three counts are the
    failing candidates' multiplicities -- about 2,000 candidates, several workgroups, the last one partial."""
    from catch_amd import engine
    if L == 1:
        # the device front end makes no candidates of one character (probe_length >= 2): the host rule is all there is
        targets = engine.Targets(ctx, [["ACGT"]])
        with pytest.raises(ValueError):
            engine.Candidates(ctx, targets, 1, 1)
        targets.close()
        for K, P, D in RULE_SETS[rules]:
            f = SF(max_hairpin_stem=K, hairpin_min_loop=P, max_self_dimer=D)
            assert f._filter_strs(list("ACGTN")) == list("ACGTN") and f.dropped == [0, 0, 0]
        return
    targets, concat, (pos0, mult0, grp0, strs0) = device_lists(L)
    _set_plane_budget(monkeypatch, L, rules)
    uniq, counts = _unique(L)
    n = len(strs0)
    assert sorted(strs0) == list(uniq) and [counts[s] for s in strs0] == mult0.tolist()
    assert mult0.max() > 1 and (n > 256 or L <= 3)
    for K, P, D in RULE_SETS[rules]:
        table = _expected(L, K, P, D)
        fails = np.array([table[s] for s in strs0], dtype=bool).reshape(n, 2)
        drop = fails[:, 0] | fails[:, 1]
        keep = ~drop
        want = [int(mult0[fails[:, 0]].sum()), int(mult0[fails[:, 1]].sum()), int(mult0[drop].sum())]
        f = SF(max_hairpin_stem=K, hairpin_min_loop=P, max_self_dimer=D)
        c = engine.Candidates(ctx, targets, L, L)
        try:
            ncand = c.ncandidates
            f._apply_to_candidates(c)
            print((K, P, D), L, n, "kept", c.n, "dropped", f.dropped, "want", want)
            pos, mult, grp, _ = _snapshot(c, concat, L)
            wrong = sorted(set(pos0[keep].tolist()) ^ set(pos.tolist()))
            assert not wrong, ((K, P, D), [(concat[p:p + L], table[concat[p:p + L]]) for p in wrong[:3]])
            assert f.dropped == want, (K, P, D)
            assert c.n == int(keep.sum()) and c.ncandidates == ncand
            assert pos.tolist() == pos0[keep].tolist(), (K, P, D)
            assert mult.tolist() == mult0[keep].tolist(), (K, P, D)
            assert grp.tolist() == grp0[keep].tolist(), (K, P, D)
            if (K, P, D) == RULE_SETS[rules][-1]:      # a second call on the filtered list: valid, and nothing more goes
                assert c.drop_structure(-1 if K is None else K, P, -1 if D is None else D) == [0, 0, 0]
                assert c.positions().tolist() == pos.tolist()
        finally:
            c.close()


@pytest.mark.gpu
def test_drop_structure_kernel_grouped_and_errors(ctx):
    """Three groups, the first and third sharing strings; then an empty list, the bad arguments (CATCHHIP_EINVAL, a
    ValueError here), thresholds beyond the length and the call after a near-duplicate filter."""
    from catch_amd import engine
    L = 40
    rng = random.Random(9)
    pool = ["".join(rng.choice("ACGT") for _ in range(L)) for _ in range(500)]
    genomes = [["".join(pool[:300])], ["".join("AC" * (L // 2) for _ in range(50))], ["".join(pool[200:])]]
    concat = "".join(s for g in genomes for s in g)
    f = SF(max_hairpin_stem=3, hairpin_min_loop=3, max_self_dimer=4)
    targets = engine.Targets(ctx, genomes)
    try:
        targets.set_groups(np.arange(3))
        base = engine.Candidates(ctx, targets, L, L)
        pos0, mult0, grp0, strs0 = _snapshot(base, concat, L)
        base.close()
        assert set(grp0.tolist()) == {0, 1, 2}
        assert set(s for s, g in zip(strs0, grp0) if g == 0) & set(s for s, g in zip(strs0, grp0) if g == 2)
        fails = np.array([f._fails(s) for s in strs0], dtype=bool)
        drop = fails[:, 0] | fails[:, 1]
        assert 0.05 * len(strs0) < drop.sum() < 0.95 * len(strs0) and fails[:, 0].any() and fails[:, 1].any()
        c = engine.Candidates(ctx, targets, L, L)
        f._apply_to_candidates(c)
        pos, mult, grp, _ = _snapshot(c, concat, L)
        c.close()
        assert f.dropped == [int(mult0[fails[:, 0]].sum()), int(mult0[fails[:, 1]].sum()), int(mult0[drop].sum())]
        assert (pos.tolist(), mult.tolist(), grp.tolist()) == (
            pos0[~drop].tolist(), mult0[~drop].tolist(), grp0[~drop].tolist())
        assert {0, 1, 2} <= set(grp.tolist())            # (AC)n pairs with nothing: the second group stays whole
        assert (grp == 1).sum() == (grp0 == 1).sum()
    finally:
        targets.close()
    targets = engine.Targets(ctx, [["AT" * 400]])
    try:
        c = engine.Candidates(ctx, targets, L, L // 2)
        n, total = c.n, c.ncandidates
        assert total > n > 0
        assert c.drop_structure() == [0, 0, 0] and c.n == n                              # both rules off
        assert c.drop_structure(-1, -5, -1) == [0, 0, 0] and c.n == n                    # (the loop is not read: rule off)
        assert c.drop_structure(L, 0, L) == [0, 0, 0] and c.n == n                       # K, D >= L
        assert c.drop_structure(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == [0, 0, 0] and c.n == n
        assert c.drop_structure(18, 3, -1) == [0, 0, 0] and c.n == n                     # L = 40 < 2 K + 2 + P = 41
        for bad in ((0, 3, -1), (-2, 3, -1), (-1, 3, 0), (-1, 3, -2), (5, -1, -1), (5, -1, 5), (0, 3, 0)):
            with pytest.raises(ValueError, match="drop_structure"):
                c.drop_structure(*bad)
        assert c.n == n
        assert c.drop_structure(-1, 3, L - 1) == [0, total, total]                       # (AT)n pairs end to end
        assert c.n == 0 and c.positions().size == 0 and c.ncandidates == total
        assert c.drop_structure(3, 3, 4) == [0, 0, 0] and c.n == 0                       # an empty list is valid
        c.close()
        c = engine.Candidates(ctx, targets, L, L // 2)
        assert c.drop_structure(18, 2, -1) == [total, 0, total] and c.n == 0             # the tightest hairpin: L = 2 K + 2 + P
        c.close()
        c = engine.Candidates(ctx, targets, L, L // 2)
        c.ndf_hamming(np.arange(8, dtype=np.int32).reshape(2, 4), 1)
        with pytest.raises(ValueError, match="candidates_drop_structure: a near-duplicate filter was already applied"):
            c.drop_structure(3, 3, 4)
        c.close()
    finally:
        targets.close()


# ------------------------------------------------------------------ GPU: the design command
def _run_design(argv, seed, capsys):
    from catch_amd import design
    random.seed(seed)
    np.random.seed(seed)
    capsys.readouterr()
    pb = design.main(design.parse_args(argv))
    return pb, capsys.readouterr().out


def _read_sequences(path):
    with open(path) as f:
        return [line.strip() for line in f if not line.startswith(">")]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--filter-with-lsh-hamming", "2"]], ids=["dup", "hamming"])
def test_device_front_end_equals_host_front_end(tmp_path, monkeypatch, capsys, extra):
    """--max-hairpin-stem 9 --max-self-dimer 11 on the first 5 Ebola genomes: the kernel on the device's candidates and
    the host's strings give the same probes and the same counts; no probe written fails _keeps; the design differs
    from the one without the options."""
    from catch_amd import engine
    from catch_amd.filter.structure_filter import StructureFilter
    plain = [EBOLA, "--limit-target-genomes", "5"] + BASE + extra
    argv = plain + EBOLA_OPTIONS
    outs, dropped, calls = {}, {}, []
    real = engine.Candidates.drop_structure

    def counted(self, *a):
        calls.append(self.n)
        got = real(self, *a)
        calls.append(self.n)
        return got
    monkeypatch.setattr(engine.Candidates, "drop_structure", counted)
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn = tmp_path / (front + ".fasta")
        pb, printed = _run_design(argv + ["-o", str(fn)], 5, capsys)
        outs[front] = fn.read_bytes()
        assert int(printed.strip().splitlines()[-1]) == outs[front].count(b">") > 0
        sf = [f for f in pb.filters if type(f) is StructureFilter]
        assert len(sf) == 1
        dropped[front] = list(sf[0].dropped)
        if front == "device":
            assert len(calls) == 2 and calls[0] > calls[1] > 0, "the device front end did not run the kernel"
    assert len(calls) == 2, "the host front end must not touch the device's candidates"
    assert outs["device"] == outs["host"]
    assert dropped["device"] == dropped["host"]
    print("dropped", dropped["device"], "unique candidates", calls)
    ncand = 1888                                    # windows of the 5 genomes
    assert all(d >= 1 for d in dropped["device"]) and ncand - dropped["device"][2] >= ncand / 2
    f = SF(max_hairpin_stem=9, max_self_dimer=11)
    probes = _read_sequences(tmp_path / "device.fasta")
    assert probes and all(f._keeps(s) for s in probes)
    # and the filter matters: another selection without it
    monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "nofilter.fasta"
    _run_design(plain + ["-o", str(fn)], 5, capsys)
    assert fn.read_bytes() != outs["device"]
    assert not all(f._keeps(s) for s in _read_sequences(fn))


@pytest.mark.gpu
def test_grid_point_with_structure_equals_design(tmp_path, capsys):
    from catch_amd import design_grid
    fa = _write_records(tmp_path / "ebola5.fasta", _ebola_records(5))
    outdir = tmp_path / "grid"
    design_grid.main(design_grid.parse_args([fa, "--grid-mismatches", "2", "--grid-cover-extension", "50",
                                             "-o", str(outdir)] + EBOLA_OPTIONS))
    capsys.readouterr()
    single = tmp_path / "single.fasta"
    _run_design([fa] + BASE + ["-o", str(single)] + EBOLA_OPTIONS, 1, capsys)
    assert (outdir / "ebola5.m2.e50.fasta").read_bytes() == single.read_bytes()
    plain = tmp_path / "plain.fasta"
    _run_design([fa] + BASE + ["-o", str(plain)], 1, capsys)
    assert plain.read_bytes() != single.read_bytes()
    f = SF(max_hairpin_stem=9, max_self_dimer=11)
    assert all(f._keeps(s) for s in _read_sequences(single))


def test_ebola_options_drop_some_but_not_most_candidates():
    """No GPU: what the end-to-end test rests on -- of the windows of the first 5 genomes each rule drops some at
    K = 9, D = 11, and most candidates stay."""
    from catch_amd.filter import candidate_probes
    cands = [c for _, s in _ebola_records(5) for c in candidate_probes.candidate_strings_from_sequences([s], 100, 50)]
    assert len(cands) == 1888
    f = SF(max_hairpin_stem=9, max_self_dimer=11)
    kept = f._filter_strs(cands)
    assert f.dropped[0] >= 1 and f.dropped[1] >= 1 and len(kept) == 1888 - f.dropped[2] >= 944
