"""The pooling step (catch_amd.pool, catchhip_pool_solve in csrc/pool.hip): the exact budgeted choice of one
designed grid point per dataset.

The contract the tests restate (never import from the product):
  * datasets in sorted name order; a dataset's options are its table rows sorted by parameter tuple ascending;
  * option k of dataset d has count n_dk and loss l_dk = w_d * (c_0 v_0^2 + c_1 v_1^2 + ...), float64, v^2 formed
    first, terms added in column order;
  * f_0[b] = 0; f_i[b] = min over k with n_ik <= b of f_{i-1}[b - n_ik] + l_ik, float64, +inf where nothing fits,
    the smallest k among equal values; the answer is f_D[B] walked back from b = B.
"""
import gzip
import io
import itertools
import json
import os
import re

import numpy as np
import pytest

from catch_amd import pool          # every test of this file needs the feature

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "pool")
WAFR = os.path.join(GOLDEN, "num-probes.V-WAfr.201506.tsv")
VALL = os.path.join(GOLDEN, "num-probes.V-All.201606.tsv.gz")


# ------------------------------------------------------------------ the definition, restated
def _instance(counts, coeffs, weights=None):
    """[(name, [(params, count, loss)])] in the contract's order."""
    out = []
    for d in sorted(counts):
        w = 1.0 if weights is None else float(weights[d])
        opts = []
        for p in sorted(counts[d]):
            s = 0.0
            for c, v in zip(coeffs, p):
                s = s + c * (v * v)
            opts.append((p, int(counts[d][p]), w * s))
        out.append((d, opts))
    return out


def _restate(inst, B):
    """The dynamic programme in NumPy, from the definition.  Returns (option index per dataset, total, loss), or
    None when f_D[B] is +inf."""
    prev = np.zeros(B + 1, dtype=np.float64)
    table = []
    for _, opts in inst:
        cur = np.full(B + 1, np.inf, dtype=np.float64)
        ch = np.full(B + 1, 0xffff, dtype=np.uint16)
        for k, (_, n, l) in enumerate(opts):
            if n > B:
                continue
            cand = prev[:B + 1 - n] + l
            seg, cseg = cur[n:], ch[n:]
            better = cand < seg                       # strict: the smallest k keeps a tie
            seg[better] = cand[better]
            cseg[better] = k
        table.append(ch)
        prev = cur
    if not np.isfinite(prev[B]):
        return None
    b, choice = B, [0] * len(inst)
    for i in range(len(inst) - 1, -1, -1):
        k = int(table[i][b])
        choice[i] = k
        b -= inst[i][1][k][1]
    return choice, B - b, float(prev[B])


def _brute(inst, B):
    """Every combination: the minimum loss (added in dataset order) within the budget and, among the combinations
    that reach it, the one whose indices read last dataset first are lexicographically smallest."""
    best = None
    for combo in itertools.product(*[range(len(o)) for _, o in inst]):
        total = sum(inst[i][1][k][1] for i, k in enumerate(combo))
        if total > B:
            continue
        loss = 0.0
        for i, k in enumerate(combo):
            loss = loss + inst[i][1][k][2]
        key = (loss, tuple(reversed(combo)))
        if best is None or key < best[0]:
            best = (key, combo, total, loss)
    return None if best is None else (list(best[1]), best[2], best[3])


def _solve(ctx, inst, B):
    """The product's kernel on an instance given in the restatement's form."""
    from catch_amd import engine
    off = np.zeros(len(inst) + 1, dtype=np.int64)
    np.cumsum([len(o) for _, o in inst], out=off[1:])
    cnt = np.array([n for _, o in inst for _, n, _ in o], dtype=np.int64)
    loss = np.array([l for _, o in inst for _, _, l in o], dtype=np.float64)
    choice, total, best = engine.pool_solve(ctx, off, cnt, loss, B)
    return [int(k) for k in choice], total, best


def _read_counts(path):
    """The table by a reader of the test's own (gzip or plain)."""
    opener = gzip.open if path.endswith(".gz") else open
    d, names = {}, None
    with opener(path, "rt") as f:
        for line in f:
            ls = line.rstrip("\n").split("\t")
            if names is None:
                assert ls[0] == "dataset" and ls[-1] == "num_probes"
                names = tuple(ls[1:-1])
                continue
            d.setdefault(ls[0], {})[tuple(float(x) for x in ls[1:-1])] = int(ls[-1])
    return names, d


def _plain_copy(path, tmp_path):
    if not path.endswith(".gz"):
        return path
    out = tmp_path / os.path.basename(path)[:-3]
    with gzip.open(path, "rt") as f:
        out.write_text(f.read())
    return str(out)


# ------------------------------------------------------------------ host
def test_probe_count_table_round_trip(tmp_path):
    """What grid.write_probe_count_table writes, pool.read_probe_counts reads; the reference's own tables read the
    same through it as through the test's reader."""
    from catch_amd import grid
    rows = [("ebola", 0, 0, 120), ("ebola", 0, 25, 80), ("ebola", 1, 0, 60), ("lassa", 2, 50, 7)]
    fn = tmp_path / "num-probes.tsv"
    grid.write_probe_count_table(rows, str(fn))
    names, d = pool.read_probe_counts(str(fn))
    assert names == ("mismatches", "cover_extension")
    assert d == {"ebola": {(0.0, 0.0): 120, (0.0, 25.0): 80, (1.0, 0.0): 60}, "lassa": {(2.0, 50.0): 7}}
    names, d = pool.read_probe_counts(WAFR)
    assert (names, d) == _read_counts(WAFR)
    assert len(d) == 19 and {len(v) for v in d.values()} == {58, 60}
    three = tmp_path / "three.tsv"
    three.write_text("dataset\tmismatches\tcover_extension\tisland\tnum_probes\na\t1\t10\t3\t5\n")
    assert pool.read_probe_counts(str(three)) == (("mismatches", "cover_extension", "island"), {"a": {(1.0, 10.0, 3.0): 5}})
    for bad in ("name\tm\tnum_probes\n", "dataset\tm\tcount\n", "dataset\tm\tnum_probes\na\t1\n",
                "dataset\tm\tnum_probes\na\t1\t-4\n", "dataset\tm\tnum_probes\na\tx\t4\n", ""):
        three.write_text(bad)
        with pytest.raises(ValueError):
            pool.read_probe_counts(str(three))


def test_options_follow_the_contract():
    """Sorted datasets, rows sorted by parameter tuple, the loss of the definition (default coefficients 1 and 1/100,
    1 for any other parameter)."""
    counts = {"b": {(1.0, 10.0): 4, (0.0, 20.0): 9, (0.0, 10.0): 11}, "a": {(3.0, 50.0): 2}}
    names, off, params, cnt, loss = pool.options(counts, pool.default_loss_coeffs(("mismatches", "cover_extension")),
                                                 {"a": 2.5, "b": 1.0})
    assert names == ["a", "b"] and off.tolist() == [0, 1, 4]
    assert params == [(3.0, 50.0), (0.0, 10.0), (0.0, 20.0), (1.0, 10.0)]
    assert cnt.tolist() == [2, 11, 9, 4]
    assert loss.tolist() == [2.5 * (9.0 + 0.01 * 2500.0), 0.01 * 100.0, 0.01 * 400.0, 1.0 + 0.01 * 100.0]
    assert loss.tolist() == [l for _, o in _instance(counts, (1.0, 1.0 / 100.0), {"a": 2.5, "b": 1.0}) for _, _, l in o]
    assert pool.default_loss_coeffs(("mismatches", "island", "cover_extension")) == (1.0, 1.0, 0.01)


def test_write_params_is_read_by_combine_pooled(tmp_path):
    from catch_amd import combine_pooled
    fn = tmp_path / "params.tsv"
    pool.write_params(("mismatches", "cover_extension"), {"lassa": (2.0, 50.0), "ebola": (0.0, 0.0)}, str(fn))
    assert fn.read_text() == "dataset\tmismatches\tcover_extension\nebola\t0\t0\nlassa\t2\t50\n"
    assert combine_pooled.read_params(str(fn)) == [("ebola", 0, 0), ("lassa", 2, 50)]
    with pytest.raises(ValueError):
        pool.write_params(("mismatches", "cover_extension"), {"ebola": (0.5, 0.0)}, str(fn))
    with pytest.raises(ValueError):
        pool.write_params(("mismatches", "cover_extension"), {"ebola": (1.0,)}, str(fn))


def test_params_file_read_by_the_reference_reader(tmp_path):
    """The reference's own pool_probes_io (when its package is importable) writes byte for byte what write_params
    writes, and its readers take our weights and counts tables."""
    pool_probes_io = pytest.importorskip("catch.utils.pool_probes_io")
    ours, theirs = tmp_path / "ours.tsv", tmp_path / "theirs.tsv"
    chosen = {"lassa": (2.0, 50.0), "ebola": (0.0, 0.0), "zika": (5.0, 10.0)}
    pool.write_params(("mismatches", "cover_extension"), chosen, str(ours))
    pool_probes_io.write_param_values_across_datasets(("mismatches", "cover_extension"), chosen, str(theirs), type="int")
    assert ours.read_bytes() == theirs.read_bytes()
    assert pool.read_probe_counts(WAFR) == pool_probes_io.read_table_of_probe_counts(WAFR)
    w = tmp_path / "w.tsv"
    w.write_text("dataset\tweight\nebola\t2.5\nlassa\t1\n")
    assert pool.read_dataset_weights(str(w)) == pool_probes_io.read_table_of_dataset_weights(str(w))


def test_dataset_weights_reader(tmp_path):
    w = tmp_path / "w.tsv"
    w.write_text("dataset\tweight\nebola\t2.5\nlassa\t1\n")
    assert pool.read_dataset_weights(str(w), ["ebola", "lassa"]) == {"ebola": 2.5, "lassa": 1.0}
    with pytest.raises(ValueError, match="zika"):
        pool.read_dataset_weights(str(w), ["ebola", "zika"])
    for bad in ("dataset\tw\nebola\t1\n", "dataset\tweight\nebola\t1\nebola\t2\n", "dataset\tweight\nebola\tx\n",
                "dataset\tweight\textra\nebola\t1\t2\n"):
        w.write_text(bad)
        with pytest.raises(ValueError):
            pool.read_dataset_weights(str(w))


def test_cli_errors(tmp_path, capsys):
    """The command line's refusals, all before any device work."""
    out = str(tmp_path / "params.tsv")
    table = tmp_path / "t.tsv"
    table.write_text("dataset\tmismatches\tcover_extension\tnum_probes\na\t0\t0\t10\na\t1\t0\t5\nb\t0\t0\t7\n")
    weights = tmp_path / "w.tsv"
    weights.write_text("dataset\tweight\na\t2\n")
    dup = tmp_path / "dup.tsv"
    dup.write_text("dataset\tmismatches\tcover_extension\tnum_probes\na\t0\t0\t10\na\t0\t0\t5\n")
    cases = [
        ([str(table), "12", out, "--loss-coeffs", "1"], "coefficients"),
        ([str(table), "12", out, "--loss-coeffs", "1", "2", "3"], "coefficients"),
        ([str(table), "12", out, "--dataset-weights", str(weights)], "b needs a weight"),
        ([str(dup), "12", out], "more than once"),
        ([str(table), "12", out, "--round-params", "1", "10"], "--round-params.*grid point"),
        ([str(table), "12", out, "--use-nd"], "--use-nd.*grid point"),
        ([str(tmp_path / "missing.tsv"), "12", out], "missing.tsv"),
    ]
    for argv, message in cases:
        with pytest.raises(SystemExit) as exc:
            pool.main(argv)
        assert exc.value.code == 2, argv
        err = capsys.readouterr().err
        assert re.search(message, err), (argv, err)
        assert not os.path.exists(out)


def test_pool_symbol_declared_bound_and_built():
    from catch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    assert re.search(r"\bcatchhip_pool_solve\s*\(", hdr)
    assert "param_search.standard_search" in hdr and "_round_params" in hdr
    assert "catchhip_pool_solve" in _lib.PROTOTYPES
    assert "pool.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(REPO, "catch_amd", "pool.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|oracle)\b", src, re.M)


def test_restatement_equals_brute_force_on_the_host():
    """The two forms of the rule the GPU tests compare against agree with each other (no device involved)."""
    rng = np.random.default_rng(101)
    for _ in range(60):
        inst = _random_small(rng)
        lo = sum(min(n for _, n, _ in o) for _, o in inst)
        hi = sum(max(n for _, n, _ in o) for _, o in inst)
        for B in sorted({max(lo - 1, 0), lo, (lo + hi) // 2, hi, hi + 3}):
            assert _restate(inst, B) == _brute(inst, B), (inst, B)


# ------------------------------------------------------------------ GPU
# Weights and coefficients of the small random tables are sums of a few powers of two, so that every loss and every
# partial sum is exact in float64: two paths then tie exactly or not at all, and the brute force's "lexicographically
# smallest among the minima" is the same choice as the programme's "smallest k at every step".
_WEIGHTS = (1.0, 2.0, 3.0, 0.5, 0.75, 1.25, 2.5)


def _random_small(rng):
    D = int(rng.integers(1, 7))
    coeffs = [(1.0, 0.25), (1.0, 1.0), (0.5, 0.125)][int(rng.integers(0, 3))]
    tied = bool(rng.integers(0, 2))
    counts, weights = {}, {}
    for i in range(D):
        K = int(rng.integers(1, 6))
        ms = rng.integers(0, 3 if tied else 6, size=8)
        es = rng.integers(0, 3 if tied else 5, size=8) * (2 if tied else 10)
        pts = list(dict.fromkeys(zip(ms.tolist(), es.tolist())))[:K]
        d = "d%02d" % i
        # counts from a handful of values: equal counts, zeros, and losses that tie across options and datasets
        counts[d] = {(float(m), float(e)): int(rng.choice([0, 1, 2, 3, 5, 8, 13, 21])) for m, e in pts}
        weights[d] = 1.0 if tied else float(rng.choice(_WEIGHTS))
    return _instance(counts, coeffs, weights)


@pytest.mark.gpu
def test_brute_force_small_tables(ctx):
    """Up to 6 datasets x 5 options, budgets from infeasible to slack, integer and non-integer weights, tied losses:
    loss and total equal the minimum over every combination exactly, the options are the tie-break rule's, and an
    infeasible budget raises and names the smallest feasible one."""
    rng = np.random.default_rng(7)
    checked = ties = raised = 0
    for _ in range(120):
        inst = _random_small(rng)
        lo = sum(min(n for _, n, _ in o) for _, o in inst)
        hi = sum(max(n for _, n, _ in o) for _, o in inst)
        for B in sorted({max(lo - 1, 0), lo, lo + 1, (lo + hi) // 2, max(hi - 1, 0), hi, hi + 1000}):
            want = _brute(inst, B)
            if want is None:
                assert B < lo
                with pytest.raises(ValueError, match=r"cannot be met.*smallest feasible budget is %d\b" % lo):
                    _solve(ctx, inst, B)
                raised += 1
                continue
            got = _solve(ctx, inst, B)
            assert got == want, (inst, B)
            assert got[1] <= B
            checked += 1
            minima = 0
            for combo in itertools.product(*[range(len(o)) for _, o in inst]):
                loss = 0.0
                for i, k in enumerate(combo):
                    loss = loss + inst[i][1][k][2]
                if loss == want[2] and sum(inst[i][1][k][1] for i, k in enumerate(combo)) <= B:
                    minima += 1
            ties += minima > 1
    assert checked >= 500 and ties >= 50 and raised >= 20


def _random_table(rng, D, kmin, kmax, nparams, count_pool, weights=True):
    """A seeded table of D datasets with kmin..kmax rows each; counts drawn from `count_pool` values (many repeats)."""
    counts, w = {}, {}
    for i in range(D):
        K = int(rng.integers(kmin, kmax + 1))
        pts = set()
        while len(pts) < K:
            need = K - len(pts)
            cols = [rng.integers(0, 12, size=2 * need)] + [rng.integers(0, 60, size=2 * need) * 5
                                                           for _ in range(nparams - 1)]
            pts.update(zip(*[c.astype(float).tolist() for c in cols]))
        pts = sorted(pts)[:K] if rng.integers(0, 2) else list(pts)[:K]
        d = "set%04d" % i
        counts[d] = {p: int(rng.choice(count_pool)) for p in pts}
        w[d] = float(rng.choice([1.0, 1.0, 0.3, 2.0, 1.7])) if weights else 1.0
    return counts, w


RESTATEMENT_CASES = [
    # name, D, kmin, kmax, parameters, distinct count values, largest count, budget
    ("wide_budget", 80, 10, 30, 2, 40, 30000, 1000000),
    ("many_datasets", 400, 20, 60, 2, 25, 1500, 150000),
    ("many_options", 60, 900, 2500, 3, 300, 900, 12000),
    ("three_parameters_tight", 200, 30, 90, 3, 12, 600, 0),        # budget 0: 5% of the way from the smallest total
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RESTATEMENT_CASES, ids=[c[0] for c in RESTATEMENT_CASES])
def test_restatement_mid_size(ctx, case):
    """Seeded mid-size tables, option by option against the NumPy programme written above from the definition."""
    name, D, kmin, kmax, nparams, nvals, cmax, B = case
    rng = np.random.default_rng(sum(map(ord, name)))
    count_pool = np.unique(rng.integers(0, cmax + 1, size=nvals))
    counts, w = _random_table(rng, D, kmin, kmax, nparams, count_pool)
    coeffs = (1.0, 1.0 / 100.0, 0.5)[:nparams]
    inst = _instance(counts, coeffs, w)
    lo = sum(min(n for _, n, _ in o) for _, o in inst)
    hi = sum(max(n for _, n, _ in o) for _, o in inst)
    if B == 0:
        B = lo + (hi - lo) // 20
    assert lo <= B < hi
    want = _restate(inst, B)
    got = _solve(ctx, inst, B)
    print("%s: D=%d options=%d budget=%d -> total %d loss %r" % (name, D, sum(len(o) for _, o in inst), B, got[1], got[2]))
    assert got[1] == want[1] and got[2] == want[2]
    assert got[0] == want[0]
    # ... and through the library: the same rows, by parameter values
    chosen, total, loss = pool.pool(counts, B, loss_coeffs=coeffs, dataset_weights=w, ctx=ctx)
    assert (total, loss) == (want[1], want[2])
    assert chosen == {d: o[k][0] for (d, o), k in zip(inst, want[0])}


def _reference_runs(table, budget):
    with open(os.path.join(GOLDEN, "reference_runs.json")) as f:
        d = json.load(f)
    return [r for r in d["runs"] if r["table"] == table and r["budget"] == budget]


def _qualifying(runs, counts, budget):
    """Recorded reference runs whose parameters are all rows of the table and whose recounted total fits."""
    out = []
    for r in runs:
        if r["status"] != "ok":
            continue
        params = {d: tuple(float(v) for v in p) for d, p in r["params"].items()}
        if set(params) != set(counts) or any(params[d] not in counts[d] for d in counts):
            continue
        if sum(counts[d][params[d]] for d in counts) > budget:
            continue
        out.append(r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [90000, 60000, 45000])
def test_v_wafr_at_least_as_good_as_the_reference(ctx, budget):
    """V-WAfr (19 datasets, the reference's own table) at the reference README's 90,000 and two tighter budgets: every
    choice is a row of the table, the total fits, the loss is the restatement's, and it is <= the loss of every
    recorded run of the reference's search (--round-params 1 10) that stayed on the grid and within the budget --
    at least 3 such runs per budget, or the comparison would say nothing."""
    names, counts = _read_counts(WAFR)
    chosen, total, loss = pool.pool(counts, budget, ctx=ctx)
    assert set(chosen) == set(counts)
    assert all(chosen[d] in counts[d] for d in counts)
    assert total == sum(counts[d][chosen[d]] for d in counts) <= budget
    inst = _instance(counts, (1.0, 1.0 / 100.0))
    want = _restate(inst, budget)
    assert (total, loss) == (want[1], want[2])
    assert chosen == {d: o[k][0] for (d, o), k in zip(inst, want[0])}
    runs = _reference_runs("V-WAfr", budget)
    ok = _qualifying(runs, counts, budget)
    print("V-WAfr at %d: exact loss %r with %d probes; reference losses %s (%d of %d runs qualify)"
          % (budget, loss, total, sorted(r["loss"] for r in ok), len(ok), len(runs)))
    assert len(ok) >= 3
    for r in ok:
        assert loss <= r["loss"], r["seed"]


@pytest.mark.gpu
def test_v_all_equals_the_restatement(ctx):
    """V-All (296 datasets x 36 points) at 350,000 against the restatement, and against the reference's recorded run
    when reference_runs.json holds one that finished on the grid within the budget (it says so when none did)."""
    names, counts = _read_counts(VALL)
    assert len(counts) == 296
    budget = 350000
    chosen, total, loss = pool.pool(counts, budget, ctx=ctx)
    assert all(chosen[d] in counts[d] for d in counts)
    assert total == sum(counts[d][chosen[d]] for d in counts) <= budget
    inst = _instance(counts, (1.0, 1.0 / 100.0))
    want = _restate(inst, budget)
    assert (total, loss) == (want[1], want[2])
    assert chosen == {d: o[k][0] for (d, o), k in zip(inst, want[0])}
    runs = _reference_runs("V-All", budget)
    assert runs, "reference_runs.json must record what became of the V-All run"
    for r in _qualifying(runs, counts, budget):
        assert loss <= r["loss"], r["seed"]


@pytest.mark.gpu
def test_solver_refusals(ctx):
    """CATCHHIP_EINVAL (ValueError) with a message: more than 65,535 options, a negative count, a choice table
    larger than the device-memory cache may hold, a dataset without options."""
    from catch_amd import engine
    with pytest.raises(ValueError, match="65535"):
        engine.pool_solve(ctx, [0, 65536], np.ones(65536, np.int64), np.zeros(65536), 10)
    with pytest.raises(ValueError, match="negative count"):
        engine.pool_solve(ctx, [0, 2, 3], [4, -1, 2], [0.0, 1.0, 2.0], 10)
    D = 50000
    off = np.arange(D + 1, dtype=np.int64) * 2
    cnt = np.tile(np.array([0, 100000], dtype=np.int64), D)
    with pytest.raises(ValueError, match="choice table"):
        engine.pool_solve(ctx, off, cnt, np.tile([1.0, 0.0], D), 4000000000)
    with pytest.raises(ValueError, match="no options"):
        engine.pool_solve(ctx, [0, 1, 1], [3], [0.0], 10)
    with pytest.raises(ValueError, match="not finite"):
        engine.pool_solve(ctx, [0, 1], [3], [float("nan")], 10)
    # a budget far above every total costs no more cells than the largest total
    choice, total, loss = engine.pool_solve(ctx, [0, 2, 4], [5, 9, 1, 7], [1.0, 0.5, 2.0, 0.25], 1 << 40)
    assert (choice.tolist(), total, loss) == ([1, 1], 16, 0.75)
    assert engine.pool_solve(ctx, [0], [], [], 5)[1:] == (0, 0.0)


def _write_fasta(path, genomes):
    with open(path, "w") as f:
        for j, g in enumerate(genomes):
            f.write(">g%d\n%s\n" % (j, "".join(g)))
    return str(path)


@pytest.mark.gpu
def test_design_grid_pool_combine_end_to_end(ctx, tmp_path, capsys):
    """Three tiny synthetic datasets through the three commands: the pooled FASTA holds exactly the reported number
    of probes, within the budget."""
    from catch_amd import combine_pooled, design_grid
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(41))
    files = [_write_fasta(tmp_path / "sp_a.fasta", synthetic.make_species(rng, [2400], 5, 2, 0.05, 0.01)),
             _write_fasta(tmp_path / "sp_b.fasta", synthetic.make_species(rng, [1800], 4, 3, 0.06, 0.02)),
             _write_fasta(tmp_path / "sp_c.fasta", synthetic.make_species(rng, [1500], 6, 2, 0.04, 0.015))]
    outdir, table, params = tmp_path / "grid", tmp_path / "num-probes.tsv", tmp_path / "params.tsv"
    design_grid.main(design_grid.parse_args(
        files + ["--grid-mismatches", "0", "2", "4", "--grid-cover-extension", "0", "20", "40", "-o", str(outdir),
                 "-pl", "75", "-ps", "25", "--write-probe-count-table", str(table)]))
    names, counts = _read_counts(str(table))
    assert len(counts) == 3 and all(len(v) == 9 for v in counts.values())
    lo = sum(min(v.values()) for v in counts.values())
    hi = sum(max(v.values()) for v in counts.values())
    assert lo < hi
    budget = (lo + hi) // 2
    capsys.readouterr()
    chosen, total, loss = pool.main([str(table), str(budget), str(params)])
    out = capsys.readouterr().out.splitlines()
    assert out == ["Number of probes: %d" % total, "Loss: %f" % loss]
    assert lo <= total <= budget
    want = _restate(_instance(counts, (1.0, 1.0 / 100.0)), budget)
    assert (total, loss) == (want[1], want[2])
    pooled = tmp_path / "pooled.fasta"
    n = combine_pooled.main([str(params), str(outdir), "-o", str(pooled)])
    headers = sum(1 for line in pooled.read_text().splitlines() if line.startswith(">"))
    assert headers == n == total <= budget
    # below the smallest total the command refuses and names the smallest feasible budget
    with pytest.raises(SystemExit):
        pool.main([str(table), str(lo - 1), str(tmp_path / "never.tsv")])
    assert re.search(r"smallest feasible budget is %d\b" % lo, capsys.readouterr().err)
    assert not (tmp_path / "never.tsv").exists()
