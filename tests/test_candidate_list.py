"""The device candidate list (csrc/candidates.hip): which windows it holds, how often each was seen, and the order a
near-duplicate filter leaves it in.  A candidate's position in that list is its set id and the greedy solver breaks
ties by set id, so every check here is an exact comparison of whole lists.

  A  a plain replay of the candidate rule (loops over one string), shown equal on the CPU to the host front end, to
     the reference's recorded output and to the host's skipping of short sequences
  B  every pattern over {x, N} of 4..12 bases (9..13 for probe lengths 8 and 9) at every (probe length, stride) of
     SWEEP: windows in list order and multiplicities, per sequence (one group each) and over the whole input, with
     truncated hashes and with interleaved groups; the CPU side counts the edges the inputs must hold
  C  the kept order after a near-duplicate filter on both sides of the 8,192 switch between the host's emulation of
     a CPython set and the device's, ungrouped and with host- and device-ordered groups mixed; expected lists come
     from the oracle (a real set of stand-ins with the PYTHONHASHSEED=0 hashes) and from nothing else

Everything is an integer or a string and is compared exactly."""
import collections
import functools
import itertools
import random

import numpy as np
import pytest

from util import load_golden

STRIDES = (1, 2, 3, 5, 13)
SHORT = [(L, s) for L in (2, 3, 4) for s in STRIDES]        # patterns of 4..12 bases
LONG = [(L, s) for L in (8, 9) for s in STRIDES]            # patterns of 9..13: cand_hash_kernel without / with a tail word
SWEEP = SHORT + LONG
SKIPS = (None, 5, 12)                                       # seq_length_to_skip; 12 skips every pattern of 4..12


# ------------------------------------------------------------------------------------------------ A. the plain replay
def n_runs(seq):
    """[a, b) of every maximal run of at least two N, left to right."""
    runs, i, n = [], 0, len(seq)
    while i < n:
        if seq[i] != "N":
            i += 1
            continue
        j = i
        while j < n and seq[j] == "N":
            j += 1
        if j - i >= 2:
            runs.append((i, j))
        i = j
    return runs


def holds_nn(seq, s, L):
    for i in range(s, s + L - 1):
        if seq[i] == "N" and seq[i + 1] == "N":
            return True
    return False


def replay_starts(seq, L, stride):
    """The rule in the header of candidates.hip: stride windows while start + L <= n, one tail window [n-L, n) iff
    n % stride != 0, then for every run of >= 2 N the window ending at its start and the window beginning at its end
    where they fit; every window that holds NN dropped."""
    n = len(seq)
    assert n >= L >= 2 and stride >= 1
    starts, s = [], 0
    while s + L <= n:
        starts.append(s)
        s += stride
    if n % stride != 0:
        starts.append(n - L)
    for a, b in n_runs(seq):
        if a - L >= 0:
            starts.append(a - L)
        if b + L <= n:
            starts.append(b)
    return [s for s in starts if not holds_nn(seq, s, L)]


def replay(seqs, L, stride, skip=None):
    out = []
    for seq in seqs:
        if skip is not None and len(seq) <= skip:
            continue
        out += [seq[s:s + L] for s in replay_starts(seq, L, stride)]
    return out


# ------------------------------------------------------------------------------------------------ B. the inputs
@functools.lru_cache(maxsize=None)
def patterns(L):
    """Every string over {x, N} of 4..12 letters (9..13 for L of 8 and 9), the shorter ones down to L letters (so that
    n == L exists for every L), and 300 random ones over {x, N, n}: a lower-case n is no N for the rule."""
    lo, hi = (4, 12) if L <= 4 else (9, 13)
    out = ["".join(p) for n in range(lo, hi + 1) for p in itertools.product("xN", repeat=n)]
    assert len(out) == 2 ** (hi + 1) - 2 ** lo and (lo != 4 or len(out) == 8176)
    out += ["".join(p) for n in range(L, lo) for p in itertools.product("xN", repeat=n)]
    rnd = random.Random(1000 + L)
    out += ["".join(rnd.choice("xxNn") for _ in range(rnd.randrange(lo, hi + 1))) for _ in range(300)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plain_form(L):
    """x = A: few distinct windows, each seen very often."""
    return tuple(p.replace("x", "A") for p in patterns(L))


@functools.lru_cache(maxsize=None)
def random_form(L):
    """Every x a base of its own."""
    rnd = random.Random(2000 + L)
    return tuple("".join(rnd.choice("ACGT") if ch == "x" else ch for ch in p) for p in patterns(L))


def edges(seq, L, stride):
    """Which exact edges of the rule one sequence holds."""
    n, kinds = len(seq), set()
    if n == L:
        kinds.add("n == L")
    elif stride > n - L:
        kinds.add("stride > n - L")
    if n % stride != 0 and (n - L) % stride == 0 and not holds_nn(seq, n - L, L):
        kinds.add("tail equal to the last stride window")
    for a, b in n_runs(seq):
        if a == 0:
            kinds.add("run at base 0")
        if b == n:
            kinds.add("run ending at the last base")
        if a == L and not holds_nn(seq, 0, L):
            kinds.add("left flank starting at lo")
        if b + L == n and not holds_nn(seq, b, L):
            kinds.add("right flank ending at hi")
        if (a >= L and holds_nn(seq, a - L, L)) or (b + L <= n and holds_nn(seq, b, L)):
            kinds.add("flank dropped for holding another run")
    for s in replay_starts(seq, L, stride):
        if "N" in seq[s:s + L]:
            kinds.add("window kept with a single N")
    return kinds


def boundary_kinds(prev, nxt):
    """What two sequences that follow each other in the input look like at their common boundary."""
    kinds = set()
    if prev[-1] == "N" and nxt[0] == "N":
        kinds.add("N|N")
        if not prev.endswith("NN") and not nxt.startswith("NN"):
            kinds.add("single N | single N")              # would be a run of two if the boundary were ignored
        if nxt.startswith("NN"):
            kinds.add("N | run at base 0")                # a run start whose left neighbour in memory is an N
    return kinds


def per_sequence(seqs, L, stride, skip=None, group_of=None):
    """What the device must hold: (ncandidates, [window], [group], [multiplicity]) with duplicates removed inside
    every group, groups given per sequence (default: all in group 0), first occurrences in candidate order."""
    count, order, ncand = collections.Counter(), {}, 0
    for q, seq in enumerate(seqs):
        g = 0 if group_of is None else group_of[q]
        for w in replay([seq], L, stride, skip):
            count[(g, w)] += 1
            order.setdefault((g, w), None)
            ncand += 1
    return ncand, [w for g, w in order], [g for g, w in order], [count[k] for k in order]


@pytest.mark.parametrize("L,stride", SWEEP)
def test_replay_equals_the_host_front_end_on_every_input(L, stride):
    from catch_amd.filter import candidate_probes
    for seqs in (plain_form(L), random_form(L)):
        full = replay(seqs, L, stride)
        assert full == candidate_probes.candidate_strings_from_sequences(list(seqs), L, stride)
        for skip in SKIPS[1:]:
            want = candidate_probes.candidate_strings_from_sequences(list(seqs), L, stride, seq_length_to_skip=skip)
            assert replay(seqs, L, stride, skip) == want
            skipped = sum(len(s) <= skip for s in seqs)
            if skipped == len(seqs):
                assert want == [] and L <= 4 and skip == 12
            elif skipped:
                assert 0 < len(want) < len(full)
            else:
                assert want == full


def test_replay_equals_the_recorded_reference_output():
    recs = load_golden("candidate_probes")
    assert recs
    for c in recs:
        assert replay(c["seqs"], c["probe_length"], c["probe_stride"]) == c["out"]


@pytest.mark.parametrize("L,stride", SWEEP)
def test_inputs_hold_every_edge_of_the_rule(L, stride):
    """The sweep cannot lose an edge unnoticed: every kind is counted over the sequences of the input and must be
    there.  Three kinds cannot exist at every (L, stride), by the rule itself:
      * a stride above n - L with n > L (one stride window, then the tail): never at stride 1;
      * the tail window equals the last stride window iff n % stride != 0 and (n - L) % stride == 0, that is
        n = L (mod stride) with L % stride != 0: never when the stride divides L (stride 1 included);
      * a flank [a-L, a) ends next to the run and [b, b+L) begins next to it, so a flank of two bases holds one
        non-N base next to the run and cannot hold NN: never at L = 2.
    There the count must be zero; everywhere else it must be positive."""
    seqs = plain_form(L)
    count = collections.Counter()
    for seq in seqs:
        count.update(edges(seq, L, stride))
    for prev, nxt in zip(seqs, seqs[1:]):
        count.update(boundary_kinds(prev, nxt))
    assert (count["stride > n - L"] > 0) == (stride > 1)           # (counted for n > L only)
    always = ["n == L", "run at base 0", "run ending at the last base", "left flank starting at lo",
              "right flank ending at hi", "window kept with a single N", "N|N", "single N | single N",
              "N | run at base 0"]
    for kind in always:
        assert count[kind] > 0, kind
    assert (count["tail equal to the last stride window"] > 0) == (L % stride != 0)
    assert (count["flank dropped for holding another run"] > 0) == (L > 2)
    # the doubled tail shows as a multiplicity of two inside one sequence
    if L % stride != 0:
        doubled = [s for s in random_form(L) if "tail equal to the last stride window" in edges(s, L, stride)]
        assert doubled
        for s in doubled:
            assert collections.Counter(replay([s], L, stride))[s[len(s) - L:]] >= 2
    # lower-case n: windows with nn, nN or Nn stay
    assert any("n" in w and ("nn" in w or "nN" in w or "Nn" in w) for w in replay(seqs, L, stride))


# ------------------------------------------------------------------------------------------------ B. on the device
def _engine():
    from catch_amd import engine
    return engine


def _built(ctx, genomes, L, stride, groups=None, skip=None):
    """(ncandidates, [window], [group], [multiplicity]) of a plain build."""
    engine = _engine()
    t = engine.Targets(ctx, genomes)
    c = None
    try:
        if groups is not None:
            t.set_groups(groups)
        c = engine.Candidates(ctx, t, L, stride, seq_length_to_skip=skip)
        flat = "".join(s for g in genomes for s in g)
        strs = [flat[p:p + L] for p in c.positions().tolist()]
        assert len(strs) == c.n
        return c.ncandidates, strs, c.groups().tolist(), c.multiplicities().tolist()
    finally:
        if c is not None:
            c.close()
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L,stride", SWEEP)
def test_every_sequence_its_own_group(ctx, L, stride):
    """One genome per pattern, each a group: de-duplication per sequence, so the list is every sequence's own unique
    windows in order, and a tail that equals the last stride window has multiplicity two."""
    seqs = random_form(L)
    group_of = list(range(len(seqs)))
    for skip in SKIPS:
        want = per_sequence(seqs, L, stride, skip, group_of)
        got = _built(ctx, [[s] for s in seqs], L, stride, groups=np.arange(len(seqs)), skip=skip)
        assert got[0] == want[0]                   # ncandidates: the sum of the replays' lengths
        assert got[2] == want[2]
        assert got[1] == want[1]
        assert got[3] == want[3]
        assert (want[0] == 0) == (L <= 4 and skip == 12)
        if skip is None and L % stride != 0:
            assert max(want[3]) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [None, "0", "3"])
@pytest.mark.parametrize("L,stride", SWEEP)
def test_whole_input_one_group(ctx, monkeypatch, L, stride, bits):
    """x = A, no groups: a few dozen distinct windows at the short probe lengths, each counted thousands of times (a
    few hundred, each counted about a hundred times, at 8 and 9); with 0 and 3 bits of the hash kept the
    representative is found by the walk over the run of equal hashes."""
    if bits is not None:
        monkeypatch.setenv("CATCHHIP_CAND_HASH_BITS", bits)
    seqs = plain_form(L)
    all_windows = replay(seqs, L, stride)
    count = collections.Counter(all_windows)
    uniq = list(dict.fromkeys(all_windows))
    ncand, strs, groups, mult = _built(ctx, [[s] for s in seqs], L, stride)
    assert ncand == len(all_windows)
    assert strs == uniq
    assert mult == [count[w] for w in uniq]
    assert sum(mult) == ncand and max(count.values()) > 50 and set(groups) == {0}


@pytest.mark.gpu
@pytest.mark.parametrize("L,stride", SWEEP)
def test_three_interleaved_groups(ctx, L, stride):
    """Genome i in group i % 3: equal windows of different groups are different candidates and are counted apart."""
    seqs = plain_form(L)
    group_of = [q % 3 for q in range(len(seqs))]
    want = per_sequence(seqs, L, stride, None, group_of)
    got = _built(ctx, [[s] for s in seqs], L, stride, groups=np.asarray(group_of))
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    assert got[3] == want[3]
    per_window = collections.Counter(want[1])
    assert max(per_window.values()) == 3 and sum(want[3]) == want[0]


@pytest.mark.gpu
def test_ids_outside_the_list_are_refused(ctx):
    engine = _engine()
    seqs = ["ACGTTNNAGGCTA", "TTGACA"]
    t = engine.Targets(ctx, [[s] for s in seqs])
    c = engine.Candidates(ctx, t, 4, 3)
    try:
        want = list(dict.fromkeys(replay(seqs, 4, 3)))
        assert c.n == len(want) >= 4
        assert c.positions([c.n - 1, 0]).tolist() == [c.positions().tolist()[c.n - 1], 0]
        for bad in (c.n, -1):
            with pytest.raises(IndexError):
                c.positions([0, bad])
    finally:
        c.close(); t.close()


# ------------------------------------------------------------------------------------------------ C. the kept order
PL = 20                                                    # probe length, stride 1
DEVICE_FROM = 8192                                         # kept candidates of one group from which the device orders
POSITIONS = [list(range(0, 8)), list(range(12, 20))]       # two tables; a pair at distance 1 shares a key in one
MIXED = (300, DEVICE_FROM, 1, DEVICE_FROM - 1, 9000, 40)   # host, device, host, host, device, host
FRONT = (DEVICE_FROM, DEVICE_FROM, 5)                      # two device groups in a row, a host run last
MINHASH_KMER = 8
MINHASH_PARAMS = [[(1103515245, 12345), (69069, 1)], [(1664525, 1013904223), (22695477, 1)]]
# Windows one base apart share 12 of their 13 + 13 - 12 = 14 distinct 8-mers: Jaccard distance 1/7.  At a threshold
# from 1/7 on every kept window drops its neighbours and about half of 9,000 stay, less than 8,192; below it the oracle
# keeps all of them but a handful, which is what the test asserts before it uses the lists.
MINHASH_THRES = 0.125


@functools.lru_cache(maxsize=None)
def chain_genome(n, seed):
    """One sequence with n windows of PL bases at stride 1 and, from 100 windows on, a copy of a stretch of it as a
    second sequence: those 50 windows have multiplicity two and come first in the filters' priority order."""
    rnd = random.Random(seed)
    s = "".join(rnd.choice("ACGT") for _ in range(n + PL - 1))
    seqs = [s]
    if n >= 100:
        at = n // 3
        seqs.append(s[at:at + 50 + PL - 1])
    windows = replay(seqs, PL, 1)
    assert len(windows) == n + (50 if n >= 100 else 0) and len(set(windows)) == n
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def planted_genome(n, pairs, seed):
    """n windows from one sequence and `pairs` windows more, each one substitution away from a window of the first
    sequence, as sequences of PL bases given twice.  The later member of every pair so has multiplicity two."""
    rnd = random.Random(seed)
    s = "".join(rnd.choice("ACGT") for _ in range(n + PL - 1))
    step = n // pairs
    assert step >= 1
    earlier, later = [], []
    for j in range(pairs):
        w = s[j * step:j * step + PL]
        at = (7 * j) % PL
        earlier.append(w)
        later.append(w[:at] + "ACGT"[("ACGT".index(w[at]) + 1 + j % 3) % 4] + w[at + 1:])
    seqs = [s] + later + later
    windows = replay(seqs, PL, 1)
    assert len(windows) == n + 2 * pairs and len(set(windows)) == n + pairs
    return tuple(seqs), tuple(earlier), tuple(later)


_ORACLE_LISTS = {}


def _oracle_list(oracle, key, seqs, kind, thres):
    """list(to_include) of one group, computed once per module."""
    k = (key, kind, thres)
    if k not in _ORACLE_LISTS:
        windows = replay(seqs, PL, 1)
        if kind == "hamming":
            _ORACLE_LISTS[k] = tuple(oracle.ndf_hamming_c(windows, thres, POSITIONS))
        else:
            _ORACLE_LISTS[k] = tuple(oracle.ndf_minhash(windows, thres, MINHASH_PARAMS, kmer_size=MINHASH_KMER))
    return list(_ORACLE_LISTS[k])


def _kept(ctx, genomes, grouped, apply):
    """[(group, window)] of the list a near-duplicate filter leaves."""
    engine = _engine()
    t = engine.Targets(ctx, [list(g) for g in genomes])
    c = None
    try:
        if grouped:
            t.set_groups(np.arange(len(genomes)))
        c = engine.Candidates(ctx, t, PL, 1)
        apply(c)
        flat = "".join(s for g in genomes for s in g)
        strs = [flat[p:p + PL] for p in c.positions().tolist()]
        assert len(strs) == c.n
        return list(zip(c.groups().tolist(), strs))
    finally:
        if c is not None:
            c.close()
        t.close()


def _assert_groups_in_oracle_order(got, want):
    groups = [g for g, w in got]
    assert groups == sorted(groups)
    for gi, w in enumerate(want):
        assert [s for g, s in got if g == gi] == w, gi
    assert len(got) == sum(map(len, want))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [DEVICE_FROM - 1, DEVICE_FROM, DEVICE_FROM + 1])
def test_kept_order_of_one_group_round_the_switch(ctx, oracle, n):
    """No groups, threshold 0: everything is kept, 8,191 by the host's set and 8,192 / 8,193 by the device's."""
    seqs = chain_genome(n, 100 + n)
    want = _oracle_list(oracle, ("chain", n, 100 + n), seqs, "hamming", 0)
    assert len(want) == n and want != list(dict.fromkeys(replay(seqs, PL, 1)))
    got = _kept(ctx, [seqs], False, lambda c: c.ndf_hamming(POSITIONS, 0))
    assert [w for g, w in got] == want


def _mixed_genomes(sizes):
    return [chain_genome(n, 300 + 10 * i + n) for i, n in enumerate(sizes)]


def _mixed_want(oracle, sizes, kind, thres):
    return [_oracle_list(oracle, ("chain", n, 300 + 10 * i + n), chain_genome(n, 300 + 10 * i + n), kind, thres)
            for i, n in enumerate(sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [MIXED, FRONT], ids=["mixed", "device-first"])
def test_kept_order_with_host_and_device_groups_mixed(ctx, oracle, sizes):
    """Threshold 0 through ndf_hamming_many: a device-ordered group after a host run, a host run between two device
    groups and a host run last; then two device groups in a row at the front."""
    want = _mixed_want(oracle, sizes, "hamming", 0)
    assert [len(w) for w in want] == list(sizes)
    got = _kept(ctx, _mixed_genomes(sizes), True,
                lambda c: c.ndf_hamming_many([POSITIONS] * len(sizes), 0))
    _assert_groups_in_oracle_order(got, want)


@pytest.mark.gpu
def test_kept_order_when_the_filter_drops_candidates(ctx, oracle):
    """Threshold 1: in the large group 200 windows have a neighbour one substitution away that was seen twice; the
    neighbour is kept and the window dropped, and what stays is still ordered on the device."""
    planted = [planted_genome(60, 3, 501), planted_genome(9800, 200, 502), planted_genome(500, 10, 503)]
    want = [_oracle_list(oracle, ("planted", i), p[0], "hamming", 1) for i, p in enumerate(planted)]
    assert len(want[1]) >= DEVICE_FROM and len(want[0]) < DEVICE_FROM and len(want[2]) < DEVICE_FROM
    for (seqs, earlier, later), w in zip(planted, want):
        kept = set(w)
        assert not kept & set(earlier) and set(later) <= kept
        assert len(w) <= len(set(replay(seqs, PL, 1))) - len(earlier)
    got = _kept(ctx, [p[0] for p in planted], True, lambda c: c.ndf_hamming_many([POSITIONS] * 3, 1))
    _assert_groups_in_oracle_order(got, want)


@pytest.mark.gpu
def test_kept_order_through_minhash(ctx, oracle):
    """The same groups through ndf_minhash_many (8-mers, two tables of two fixed functions): cand_apply_keep and the
    order are shared with the Hamming filter, the way to them is not."""
    want = _mixed_want(oracle, MIXED, "minhash", MINHASH_THRES)
    kept = [len(w) for w in want]
    assert kept[4] >= DEVICE_FROM and all(k <= n for k, n in zip(kept, MIXED)) and kept[3] == DEVICE_FROM - 1
    assert 0 < sum(MIXED) - sum(kept) < 10           # (a few windows with repeats inside are within the threshold)
    got = _kept(ctx, _mixed_genomes(MIXED), True,
                lambda c: c.ndf_minhash_many(MINHASH_KMER, [MINHASH_PARAMS] * len(MIXED), MINHASH_THRES))
    _assert_groups_in_oracle_order(got, want)


def test_windows_round_the_switch_are_distinct_and_the_oracle_orders_them(oracle):
    """On the CPU: the chain genomes give exactly n distinct windows (asserted where they are built), and the
    oracle's list is a permutation of them that is neither the input order nor the priority order."""
    for n in (DEVICE_FROM - 1, DEVICE_FROM, DEVICE_FROM + 1):
        seqs = chain_genome(n, 100 + n)
        windows = replay(seqs, PL, 1)
        want = _oracle_list(oracle, ("chain", n, 100 + n), seqs, "hamming", 0)
        assert sorted(want) == sorted(set(windows)) and len(want) == n
        assert want != list(dict.fromkeys(windows))
        assert want != oracle.ndf_hamming_c(windows, 0, POSITIONS, inclusion_order=True)
