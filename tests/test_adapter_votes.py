"""The two device consumers of the first-seen row table, catchhip_adapter_votes (the av_* kernels of csrc/scan.hip)
and catchhip_rows_first_seen_per_set (csrc/analysis.hip), against a plain replay of the same operation on the same
rows, at the smallest inputs that cross every launch edge:

  av_schedule_kernel   64 threads per workgroup, one thread per universe   -> 150 universes, three workgroups
  av_tally_kernel      one workgroup of 1,024, strided through the voters  -> a universe with 2,271 voters, three trips
  av_lower / hkeys     universes without rows, the first and the last ones among them

The replay is shown equal to the oracle's restatement of the reference and to the reference's own recorded votes
on the CPU, so it is a reference and not a second copy of the kernels.  Everything is an integer and is compared
exactly."""
import random
import sys

import numpy as np
import pytest

from util import load_golden, np_state_from_json, rows_as_tuples

L = 30
NUNIV = 150
PLANTED_EMPTY = (0, 7, 64, 149)
SETTINGS = {"A": dict(m=1, thres=30, seed=1),      # pigeonhole k = 15, seed path
            "B": dict(m=2, thres=24, seed=2)}      # random anchors, k = 10, ranges of varying length


# ------------------------------------------------------------------------------------------------ the plain replay
def replay_votes(set_id, univ, start, end, first_key, mult, nuniv):
    """AdapterFilter._make_votes_across_target_genomes on a fetched row table: [(A, B)] per set id < len(mult), and
    facts about the input (which edges it crosses).  Loops over Python integers, nothing else."""
    num_sets = len(mult)
    mult = [int(w) for w in mult]
    per_univ = [[] for _ in range(nuniv)]
    for r, (s, u, a, b, k) in enumerate(zip(set_id, univ, start, end, first_key)):
        s, u = int(s), int(u)
        assert 0 <= s < num_sets and 0 <= u < nuniv
        per_univ[u].append((int(b), int(k), int(a), s, r))
    cum_a, cum_b = [0] * num_sets, [0] * num_sets
    facts = dict(voters=[], empty_universes=[], swaps=0, non_swaps=0, ties=0, touching=0, taken_non_head=0,
                 taken_only_through_non_head=0, equal_end_pairs=0, ties_only_the_key_breaks=0, sets_without_rows=0)
    has_rows = [False] * num_sets
    for u in range(nuniv):
        rows = sorted(per_univ[u])                     # by (end, first-seen key)
        group_start = {}                               # first row of every (set, universe) group: smallest start
        for b, k, a, s, r in rows:
            group_start[s] = min(group_start.get(s, a), a)
            has_rows[s] = True
        facts["voters"].append(len(group_start))
        if not rows:
            facts["empty_universes"].append(u)
            continue
        i = 0
        while i < len(rows):                           # rows of different sets that end together
            j = i
            while j < len(rows) and rows[j][0] == rows[i][0]:
                j += 1
            sets_here = [r[3] for r in rows[i:j]]
            for x in range(len(sets_here)):
                for y in range(x + 1, len(sets_here)):
                    if sets_here[x] != sets_here[y]:
                        facts["equal_end_pairs"] += 1
            i = j
        ending_at = {}
        for row in rows:
            ending_at.setdefault(row[0], []).append(row)
        taken, taken_head, last_end = set(), set(), None
        non_head = []
        for b, k, a, s, r in rows:
            if last_end is None or a >= last_end:
                if last_end is not None and a == last_end:
                    facts["touching"] += 1
                # another set's row ends here too, could be taken as well, and comes first in the table
                if any(b2 == b and s2 != s and r2 < r and (last_end is None or a2 >= last_end)
                       for b2, k2, a2, s2, r2 in ending_at[b]):
                    facts["ties_only_the_key_breaks"] += 1
                if a == group_start[s]:
                    taken_head.add(s)
                else:
                    facts["taken_non_head"] += 1
                    non_head.append(s)
                taken.add(s)
                last_end = b
        facts["taken_only_through_non_head"] += len(set(non_head) - taken_head)
        plain = swapped = 0
        for s in group_start:
            a, b = (1, 0) if s in taken else (0, 1)
            base = max(cum_a[s], cum_b[s])
            plain += mult[s] * (max(cum_a[s] + a, cum_b[s] + b) - base)
            swapped += mult[s] * (max(cum_a[s] + b, cum_b[s] + a) - base)
        if swapped > plain:
            facts["swaps"] += 1
        elif swapped == plain:
            facts["ties"] += 1
        else:
            facts["non_swaps"] += 1
        for s in group_start:
            a, b = (1, 0) if s in taken else (0, 1)
            if swapped > plain:
                a, b = b, a
            cum_a[s] += a
            cum_b[s] += b
    facts["sets_without_rows"] = has_rows.count(False)
    return list(zip(cum_a, cum_b)), facts


def replay_first_seen_per_set(set_id, univ, first_key, num_sets):
    """(first universe, its first-seen key) per set id < num_sets; (-1, 0) for a set without rows."""
    out = [(-1, 0)] * num_sets
    for s, u, k in zip(set_id, univ, first_key):
        s, u, k = int(s), int(u), int(k)
        if s < num_sets and (out[s][0] < 0 or u < out[s][0]):
            out[s] = (u, k)
    return out


# --------------------------------------------------------------------------------------------------------- inputs
def make_recipe(seed):
    """(unique probes, 150 sequences, one multiplicity per probe, the root S)."""
    rnd = random.Random(seed)

    def bases(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))

    S, R = bases(2300), bases(1500)
    probes = [S[i:i + L] for i in range(len(S) - L + 1)]
    assert len(probes) == 2271
    probes += [R[i:i + L] for i in range(0, len(R) - L + 1, 15)]
    uniq = list(dict.fromkeys(probes))
    seqs = []
    for u in range(NUNIV):
        if u in PLANTED_EMPTY:
            seqs.append(bases(rnd.randrange(30, 200)))
        elif u == 1:
            seqs.append(S)
        elif u == 5:                                   # a probe gets two rows in one universe
            a = rnd.randrange(0, len(S) - 150 + 1)
            seqs.append(S[a:a + 150] + "TT" + S[a:a + 150])
        else:
            root = S if u % 4 == 2 else R
            n = rnd.randrange(30, 500)
            a = rnd.randrange(0, len(root) - n + 1)
            rate = rnd.choice((0.0, 0.01, 0.03))
            seqs.append("".join(rnd.choice("ACGT") if rnd.random() < rate else c for c in root[a:a + n]))
    mult = [rnd.choice([1, 1, 1, 2, 3, 7]) for _ in uniq]
    return uniq, seqs, mult, S


def oracle_rows(oracle, uniq, entries, k, seqs, m, thres, ent_rank):
    """The row table the oracle gives, sorted as the device's: (set, universe, start, end, first-seen key) columns,
    and per universe the probes in the order the oracle's scan first meets them."""
    rows, met = [], []
    for u, s in enumerate(seqs):
        cov = oracle.scan_sequence(s, uniq, entries, k, m, thres, 0, merge=True)
        first = oracle.scan_first_seen(s, uniq, entries, k, m, thres, 0, ent_rank)
        assert set(cov) == set(first)
        for p, ranges in cov.items():
            key = (first[p][0] << 32) | ent_rank[first[p][1]]
            rows += [(p, u, a, b, key) for a, b in ranges]
        met.append(sorted(cov, key=lambda p: (first[p][0], ent_rank[first[p][1]])))
    rows.sort()
    return [list(c) for c in zip(*rows)] if rows else [[], [], [], [], []], met


class Input:
    pass


_inputs = {}


def make_input(oracle, name):
    """Setting A or B, built once: the recipe, the anchors as in test_first_seen_keys_match_oracle, and the
    oracle's rows and keys.  Nothing here is changed afterwards."""
    if name in _inputs:
        return _inputs[name]
    cfg = SETTINGS[name]
    inp = Input()
    inp.m, inp.thres = cfg["m"], cfg["thres"]
    inp.uniq, inp.seqs, inp.mult, inp.S = make_recipe(cfg["seed"])
    np.random.seed(3)
    inp.k, inp.entries, _draws = oracle.anchor_table(inp.uniq, inp.m, inp.thres, min_k=10, k=10, with_draws=True)
    seen, inp.ent_rank = {}, []
    for p, pos in inp.entries:                         # distinct ranks inside a k-mer's entry list
        km = inp.uniq[p][pos:pos + inp.k]
        inp.ent_rank.append(seen.get(km, 0))
        seen[km] = inp.ent_rank[-1] + 1
    inp.cols, inp.met = oracle_rows(oracle, inp.uniq, inp.entries, inp.k, inp.seqs, inp.m, inp.thres, inp.ent_rank)
    # one set weighs 10**6 and alone decides the swaps of its universes: of the sets with rows in the most
    # universes, the first whose weight changes the outcome
    ones = [1] * len(inp.uniq)
    in_universes = {}
    for s, u in zip(inp.cols[0], inp.cols[1]):
        in_universes.setdefault(s, set()).add(u)
    plain = replay_votes(*inp.cols, ones, NUNIV)[0]
    for s in sorted(in_universes, key=lambda s: (-len(in_universes[s]), s))[:40]:
        inp.heavy = ones[:s] + [10 ** 6] + ones[s + 1:]
        if replay_votes(*inp.cols, inp.heavy, NUNIV)[0] != plain:
            break
    _inputs[name] = inp
    return inp


def mult_vectors(inp):
    return (("ones", [1] * len(inp.uniq)), ("drawn", inp.mult), ("heavy", inp.heavy))


def assert_crosses_every_edge(name, votes, facts):
    """The conditions the device tests rely on, from the replay's facts."""
    assert max(facts["voters"]) > 2048                 # three trips of the tally loop
    assert len(facts["voters"]) > 128                  # three workgroups of the schedule
    empty = facts["empty_universes"]
    assert len(empty) >= 4 and empty[0] == 0 and empty[-1] == len(facts["voters"]) - 1
    assert set(PLANTED_EMPTY) <= set(empty)
    assert facts["swaps"] >= 10 and facts["non_swaps"] >= 10
    assert facts["ties"] >= 2
    assert facts["touching"] >= 100
    assert facts["taken_non_head"] >= 1
    assert facts["sets_without_rows"] >= 1
    assert sum(1 for a, b in votes if a > b) >= 10 and sum(1 for a, b in votes if b >= a and a + b) >= 10
    if name == "B":
        assert facts["equal_end_pairs"] >= 50
        assert facts["ties_only_the_key_breaks"] >= 1


# ------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("name", ["A", "B"])
def test_inputs_cross_every_edge(oracle, name):
    """From the oracle alone: the recipe crosses every launch edge and decision edge the device tests are about."""
    inp = make_input(oracle, name)
    assert inp.k == (15 if name == "A" else 10)
    votes, facts = replay_votes(*inp.cols, inp.mult, NUNIV)
    print(name, {k: v for k, v in facts.items() if k != "voters"}, "rows", len(inp.cols[0]),
          "largest universe", max(facts["voters"]), "A > B", sum(1 for a, b in votes if a > b))
    assert_crosses_every_edge(name, votes, facts)
    # a group chosen only through a row that is not its first: group_chosen must be written at the head
    assert facts["taken_only_through_non_head"] >= 1
    # the heavy set's multiplicity decides swaps that go the other way without it
    decided = {n: replay_votes(*inp.cols, w, NUNIV)[0] for n, w in mult_vectors(inp)}
    assert decided["ones"] != decided["heavy"]
    # and the first-seen read-out has sets without rows, and sets for which "first" chooses among several universes
    first = replay_first_seen_per_set(inp.cols[0], inp.cols[1], inp.cols[4], len(inp.uniq))
    assert sum(1 for u, _ in first if u < 0) == facts["sets_without_rows"]
    assert len({(s, u) for s, u in zip(inp.cols[0], inp.cols[1]) if u != first[s][0]}) >= 100


def test_replay_equals_the_oracle(oracle):
    """replay_votes on the oracle's rows == oracle.adapter_votes, which takes the multiplicities from repeated
    probe strings: input A with every probe repeated as often as its drawn multiplicity says."""
    inp = make_input(oracle, "A")
    strs = list(inp.uniq)
    for p, w in zip(inp.uniq, inp.mult):
        strs += [p] * (w - 1)
    np.random.seed(3)
    want = oracle.adapter_votes(strs, inp.seqs, inp.m, inp.thres, 0, 10, hash_fn=hash)
    np.random.seed(3)
    k, entries, draws = oracle.anchor_table(strs, inp.m, inp.thres, min_k=10, k=10, with_draws=True)
    assert oracle._unique_last(strs)[0] == inp.uniq and entries == inp.entries
    ent_rank = oracle.kmer_entry_ranks(strs, entries, draws, k, hash)
    cols, _met = oracle_rows(oracle, inp.uniq, entries, k, inp.seqs, inp.m, inp.thres, ent_rank)
    votes, facts = replay_votes(*cols, inp.mult, NUNIV)
    assert max(inp.mult) > 1 and facts["swaps"] >= 10 and facts["non_swaps"] >= 10
    uidx = {p: i for i, p in enumerate(inp.uniq)}
    assert [votes[uidx[p]] for p in strs] == want


def test_replay_equals_the_reference_vectors(oracle):
    """replay_votes on the oracle's rows == the votes the reference itself recorded for its own test cases."""
    g = load_golden("adapter_filter")
    same_python = g["python"].split(".")[:2] == sys.version.split()[0].split(".")[:2]
    assert len(g["from_reference_tests"]) >= 4
    for c in g["from_reference_tests"]:
        strs, m, thres, kk = c["probes"], c["mismatches"], c["lcf_thres"], c["kmer_probe_map_k"]
        assert c.get("island", 0) == 0
        np.random.set_state(np_state_from_json(c["np_state"]))
        k, entries, draws = oracle.anchor_table(strs, m, thres, min_k=kk, k=kk, with_draws=True)
        uniq, _ = oracle._unique_last(strs)
        uidx = {p: i for i, p in enumerate(uniq)}
        ent_rank = oracle.kmer_entry_ranks(strs, entries, draws, k, oracle.pyhash_seed0)
        mult = [0] * len(uniq)
        for p in strs:
            mult[uidx[p]] += 1
        cols, _met = oracle_rows(oracle, uniq, entries, k, c["sequences"], m, thres, ent_rank)
        votes, _facts = replay_votes(*cols, mult, len(c["sequences"]))
        got = [votes[uidx[p]] for p in strs]
        assert [a + b for a, b in got] == [a + b for a, b in c["votes"]]
        if same_python:
            assert [list(v) for v in got] == c["votes"]


# ------------------------------------------------------------------------------------------------------ GPU tests
def _scan(ctx, uniq, entries, k, seqs, m, thres, ent_rank):
    from catch_amd import engine
    ep = np.array([e[0] for e in entries], dtype=np.int32)
    eo = np.array([e[1] for e in entries], dtype=np.int32)
    t = engine.Targets(ctx, [[s] for s in seqs])
    p = engine.Probes(ctx, uniq, np.arange(len(uniq), dtype=np.int32), ep, eo, k)
    try:
        return engine.Rows.scan_first_seen(ctx, p, t, m, thres, 0, 0, engine.SCAN_AUTO,
                                           np.asarray(ent_rank, dtype=np.uint32))
    finally:
        p.close()
        t.close()


@pytest.fixture(scope="module")
def device_rows(ctx, oracle):
    """name -> (input, the device's first-seen row table of it, its fetched columns); one scan per setting."""
    made = {}

    def get(name):
        if name not in made:
            inp = make_input(oracle, name)
            rows = _scan(ctx, inp.uniq, inp.entries, inp.k, inp.seqs, inp.m, inp.thres, inp.ent_rank)
            sid, univ, st, en = rows.fetch()
            made[name] = (inp, rows, (sid, univ, st, en, rows.fetch_first_seen()))
        return made[name]

    yield get
    for _inp, rows, _cols in made.values():
        rows.close()


def _pairs(a, b):
    return list(zip(a.tolist(), b.tolist()))


def _some_host_rows(ctx):
    from catch_amd import engine
    return engine.Rows.from_host(ctx, [0, 0, 2], [0, 1, 1], [0, 3, 5], [10, 20, 30], [40, 40])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_votes_equal_the_replay_of_the_fetched_rows(device_rows, name):
    """catchhip_adapter_votes == replay_votes of the very rows and keys the device holds, for three multiplicity
    vectors; the rows and keys themselves == the oracle's, so a failure says which half is wrong."""
    inp, rows, cols = device_rows(name)
    sid, univ, st, en, key = cols
    assert rows.ngenomes == NUNIV
    assert rows_as_tuples(sid, univ, st, en) == sorted(zip(*inp.cols[:4]))
    assert [int(x) for x in sid] == inp.cols[0] and [int(x) for x in univ] == inp.cols[1]      # same order, too
    assert [int(x) for x in key] == inp.cols[4]
    answers = {}
    for which, mult in mult_vectors(inp):
        want, facts = replay_votes(sid, univ, st, en, key, mult, NUNIV)
        if which == "drawn":
            assert_crosses_every_edge(name, want, facts)
        assert facts["swaps"] >= 10 and facts["non_swaps"] >= 10 and max(facts["voters"]) > 2048
        got = _pairs(*rows.adapter_votes(mult))
        bad = [(s, g, w) for s, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, "%s: %d sets differ, first (set, device, replay): %s" % (which, len(bad), bad[:5])
        answers[which] = got
    assert answers["ones"] != answers["heavy"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A"])
def test_votes_equal_the_oracle_end_to_end(ctx, oracle, name):
    """AdapterFilter over the 150 sequences, ordinary Probe objects, the first 20 probes given twice == the
    oracle's restatement with this interpreter's string hash."""
    from catch_amd import probe
    from catch_amd.filter.adapter_filter import AdapterFilter
    from catch_amd.genome import Genome
    inp = make_input(oracle, name)
    strs = inp.uniq + inp.uniq[:20]
    f = AdapterFilter(("AC", "GT"), ("TT", "GG"), inp.m, inp.thres, kmer_probe_map_k=10)
    np.random.seed(3)
    got = f._make_votes_across_target_genomes([probe.Probe.from_str(s) for s in strs],
                                              [[Genome.from_one_seq(s) for s in inp.seqs]])
    np.random.seed(3)
    want = oracle.adapter_votes(strs, inp.seqs, inp.m, inp.thres, 0, 10, hash_fn=hash)
    assert [tuple(v) for v in got] == want
    assert got[:20] == got[-20:]
    assert sum(1 for a, b in want if a > b) >= 10 and sum(1 for a, b in want if b >= a and a + b) >= 10


@pytest.mark.gpu
def test_votes_edges(ctx, oracle, device_rows):
    inp, rows, cols = device_rows("A")
    n = len(inp.uniq)
    want, _facts = replay_votes(*cols, inp.mult, NUNIV)
    # a repeated call on the same rows
    first = _pairs(*rows.adapter_votes(inp.mult))
    assert first == want and _pairs(*rows.adapter_votes(inp.mult)) == first
    # num_sets larger than the largest set id with rows
    longer = list(inp.mult) + [5] * 37
    got = _pairs(*rows.adapter_votes(longer))
    assert got[:n] == want and got[n:] == [(0, 0)] * 37
    # num_sets == 0
    a, b = rows.adapter_votes(np.zeros(0, dtype=np.int64))
    assert a.size == 0 and b.size == 0
    # one universe only: S itself
    one = _scan(ctx, inp.uniq, inp.entries, inp.k, [inp.S], inp.m, inp.thres, inp.ent_rank)
    try:
        sid, univ, st, en = one.fetch()
        want1, facts1 = replay_votes(sid, univ, st, en, one.fetch_first_seen(), inp.mult, 1)
        # from totals of zero either way round gains one per voter: an exact tie, nothing is swapped
        assert facts1["voters"] == [2271] and facts1["ties"] == 1
        assert 0 < sum(a for a, b in want1) < sum(b for a, b in want1)
        assert _pairs(*one.adapter_votes(inp.mult)) == want1
    finally:
        one.close()
    # every universe empty
    none = _scan(ctx, inp.uniq, inp.entries, inp.k, [inp.seqs[u] for u in PLANTED_EMPTY], inp.m, inp.thres,
                 inp.ent_rank)
    try:
        assert none.n == 0
        assert _pairs(*none.adapter_votes(inp.mult)) == [(0, 0)] * n
    finally:
        none.close()
    # rows without first-seen keys are refused before anything is launched
    host = _some_host_rows(ctx)
    try:
        with pytest.raises(ValueError, match="do not come from catchhip_cover_scan_first_seen"):
            host.adapter_votes([1, 1, 1])
    finally:
        host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_first_seen_per_set_equals_the_replay(ctx, oracle, device_rows, name):
    """catchhip_rows_first_seen_per_set == the replay on the fetched rows; its num_sets guard, its answer for sets
    and tables without rows, and the order the coverage analysis derives from it == the oracle's."""
    from catch_amd._lib import c_i32p, c_u64p, check
    from catch_amd.engine import _ptr
    inp, rows, cols = device_rows(name)
    sid, univ, st, en, key = cols
    n = len(inp.uniq)
    want = replay_first_seen_per_set(sid, univ, key, n)
    fu, fk = rows.first_seen_per_set(n)
    assert fu.dtype == np.int32 and fk.dtype == np.uint64
    assert _pairs(fu, fk) == want
    without = [s for s in range(n) if s not in set(inp.cols[0])]
    assert without and all(want[s] == (-1, 0) for s in without)
    assert sum(1 for u, _ in want if u < 0) == len(without)
    # num_sets below the largest set id present: the prefix, and nothing written past it
    half = n // 2
    assert half < max(inp.cols[0])
    hu, hk = rows.first_seen_per_set(half)
    assert _pairs(hu, hk) == want[:half]
    canary_u, canary_k = np.full(n, -7, dtype=np.int32), np.full(n, 0xC0FFEE, dtype=np.uint64)
    check(ctx._L.catchhip_rows_first_seen_per_set(ctx._h, rows._h, half, _ptr(canary_u, c_i32p),
                                                  _ptr(canary_k, c_u64p)))
    assert _pairs(canary_u[:half], canary_k[:half]) == want[:half]
    assert (canary_u[half:] == -7).all() and (canary_k[half:] == 0xC0FFEE).all()
    # num_sets == 0
    zu, zk = rows.first_seen_per_set(0)
    assert zu.size == 0 and zk.size == 0
    # the order Analyzer._map_count_order derives == the order the oracle's scans first meet each probe
    seen = np.flatnonzero(fu >= 0)
    order = seen[np.lexsort((fk[seen], fu[seen]))].tolist()
    met, known = [], set()
    for probes in inp.met:
        met += [p for p in probes if p not in known]
        known.update(probes)
    assert order == met and len(order) == n - len(without)
    # an empty table; rows without first-seen keys
    none = _scan(ctx, inp.uniq, inp.entries, inp.k, [inp.seqs[u] for u in PLANTED_EMPTY], inp.m, inp.thres,
                 inp.ent_rank)
    try:
        assert none.n == 0
        assert _pairs(*none.first_seen_per_set(5)) == [(-1, 0)] * 5
    finally:
        none.close()
    host = _some_host_rows(ctx)
    try:
        with pytest.raises(ValueError, match="do not come from catchhip_cover_scan_first_seen"):
            host.first_seen_per_set(3)
    finally:
        host.close()
