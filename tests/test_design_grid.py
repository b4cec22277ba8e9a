"""Grid design (catch_amd.grid, catch_amd.design_grid, catch_amd.combine_pooled)
and the rows-at-several-extensions kernel behind it (catchhip_rows_extend,
catchhip_setcover_grid)."""
import hashlib
import io
import json
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EBOLA = os.path.join(GOLDEN, "ebola_zaire_100.fasta.gz")


# ------------------------------------------------------------------ host
def _normalise(ranges):
    """catch/utils/interval.py:288-316: sort, merge overlapping or touching."""
    out = []
    for s, t in sorted(ranges):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], t)
        else:
            out.append([s, t])
    return [tuple(x) for x in out]


def _extend_raw(ranges, seq_off, e):
    """Every raw range extended by e and clipped to its own sequence, then normalised."""
    out = []
    for s, t in ranges:
        q = int(np.searchsorted(seq_off, s, side="right")) - 1
        out.append((max(seq_off[q], s - e), min(seq_off[q + 1], t + e)))
    return _normalise(out)


def _extend_rows(rows0, seq_off, e):
    """The identity the kernel uses: the e = 0 rows, each end clipped to the sequence that holds it."""
    out = []
    for s, t in rows0:
        qs = int(np.searchsorted(seq_off, s, side="right")) - 1
        qt = int(np.searchsorted(seq_off, t - 1, side="right")) - 1
        out.append((max(seq_off[qs], s - e), min(seq_off[qt + 1], t + e)))
    return _normalise(out)


def test_extension_identity_host_model():
    """Extending the merged e = 0 rows (each end clipped to its own sequence) equals extending and clipping every
    raw range -- with short sequences, ranges at both ends of a sequence and runs across a boundary."""
    rng = np.random.default_rng(5)
    for _ in range(400):
        lens = rng.integers(1, 60, size=int(rng.integers(1, 6)))
        seq_off = np.concatenate([[0], np.cumsum(lens)]).tolist()
        raw = []
        for q in range(len(lens)):
            for _ in range(int(rng.integers(0, 5))):
                a = int(rng.integers(seq_off[q], seq_off[q + 1]))
                b = int(rng.integers(a + 1, seq_off[q + 1] + 1))
                raw.append((a, b))
        rows0 = _normalise(raw)
        for e in (0, 1, 2, 7, 50, 200):
            assert _extend_rows(rows0, seq_off, e) == _extend_raw(raw, seq_off, e)


def test_probe_count_table_passes_the_reader_rules():
    from catch_amd import grid
    counts = [("ebola", 0, 0, 120), ("ebola", 0, 25, 80), ("lassa", 2, 50, 7)]
    buf = io.StringIO()
    grid.write_probe_count_table(counts, buf)
    lines = buf.getvalue().splitlines()
    header = lines[0].split("\t")
    assert header[0] == "dataset" and header[-1] == "num_probes"
    assert header == ["dataset", "mismatches", "cover_extension", "num_probes"]
    seen = set()
    for line in lines[1:]:
        ls = line.split("\t")
        assert len(ls) == len(header)
        key = (ls[0], tuple(float(x) for x in ls[1:-1]))
        assert key not in seen
        seen.add(key)
        assert str(int(ls[-1])) == ls[-1]
    assert len(seen) == 3
    with pytest.raises(ValueError):
        grid.write_probe_count_table(counts + [("ebola", 0, 0, 1)], io.StringIO())


def test_probe_count_table_read_by_the_reference_reader(tmp_path):
    """The reference's own reader (when its package is importable) reads the table."""
    pool_probes_io = pytest.importorskip("catch.utils.pool_probes_io")
    from catch_amd import grid
    fn = tmp_path / "num-probes.tsv"
    grid.write_probe_count_table([("a", 0, 0, 10), ("a", 0, 10, 9), ("b", 1, 0, 4)], str(fn))
    names, d = pool_probes_io.read_table_of_probe_counts(str(fn))
    assert tuple(names) == ("mismatches", "cover_extension")
    assert d == {"a": {(0.0, 0.0): 10, (0.0, 10.0): 9}, "b": {(1.0, 0.0): 4}}


def _fake_grid_dir(tmp_path):
    out = tmp_path / "grid"
    out.mkdir()
    for d in ("ebola", "lassa"):
        for m in (0, 1):
            for e in (0, 10):
                (out / ("%s.m%d.e%d.fasta" % (d, m, e))).write_text(">%s_%d_%d\nACGT\n" % (d, m, e))
    return out


def test_combine_pooled_integer_and_integral_float_values(tmp_path):
    from catch_amd import combine_pooled
    out = _fake_grid_dir(tmp_path)
    for fmt in ("%d", "%f"):
        params = tmp_path / "params.tsv"
        params.write_text("dataset\tmismatches\tcover_extension\n" +
                          ("lassa\t" + fmt + "\t" + fmt + "\n") % (1, 10) +
                          ("ebola\t" + fmt + "\t" + fmt + "\n") % (0, 0))
        fa = tmp_path / "pooled.fasta"
        n = combine_pooled.combine(str(params), str(out), str(fa))
        assert n == 2
        assert fa.read_text() == ">lassa_1_10\nACGT\n>ebola_0_0\nACGT\n"


def test_combine_pooled_rejects_fractional_values_and_missing_points(tmp_path, capsys):
    from catch_amd import combine_pooled
    out = _fake_grid_dir(tmp_path)
    params = tmp_path / "params.tsv"
    params.write_text("dataset\tmismatches\tcover_extension\nebola\t0.000000\t4.500000\n")
    with pytest.raises(ValueError, match=r"ebola.*--round-params"):
        combine_pooled.combine(str(params), str(out), str(tmp_path / "x.fasta"))
    params.write_text("dataset\tmismatches\tcover_extension\nlassa\t3\t0\n")
    with pytest.raises(FileNotFoundError, match="lassa"):
        combine_pooled.combine(str(params), str(out), str(tmp_path / "x.fasta"))
    with pytest.raises(SystemExit):
        combine_pooled.main([str(params), str(out), "-o", str(tmp_path / "x.fasta")])
    assert "lassa" in capsys.readouterr().err


def test_dataset_names_and_refused_options(tmp_path):
    from catch_amd import design_grid, grid
    assert grid.dataset_name("/x/ebola.fasta") == "ebola"
    assert grid.dataset_name("ebola.fa.gz") == "ebola"
    assert grid.dataset_name("y/lassa.fna") == "lassa"
    assert grid.dataset_name("lassa.fasta.gz") == "lassa"
    assert grid.dataset_name("zika.txt") == "zika.txt"
    base = ["--grid-mismatches", "0", "1", "--grid-cover-extension", "0", "10", "-o", str(tmp_path)]
    args = design_grid.parse_args(["a/ebola.fasta", "b/lassa.fa.gz"] + base)
    assert args.names == ["ebola", "lassa"]
    bad = [
        ["a/ebola.fasta", "b/ebola.fa"] + base,                                     # same name
        ["a.fasta", "--grid-mismatches", "0", "0", "--grid-cover-extension", "0", "-o", "x"],
        ["a.fasta", "--grid-mismatches", "0", "--grid-cover-extension", "5", "5", "-o", "x"],
    ]
    for opt in (["-i"], ["--avoid-genomes", "x.fasta"], ["-mt", "3"], ["-lt", "80"],
                ["--island-of-exact-match-tolerant", "5"], ["--cluster-and-design-separately", "0.1"],
                ["--cluster-from-fragments", "1000"], ["--add-adapters"], ["--print-analysis"],
                ["--write-analysis-to-tsv", "a.tsv"], ["--write-sliding-window-coverage", "s.tsv"],
                ["--write-probe-map-counts-to-tsv", "c.tsv"], ["-m", "2"], ["-e", "10"]):
        bad.append(["a.fasta"] + base + opt)
    for argv in bad:
        with pytest.raises(SystemExit):
            design_grid.parse_args(argv)
    with pytest.raises(ValueError):
        grid.check_grid_values("m", [1, 2, 1])


def test_grid_symbols_declared_and_bound():
    from catch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name in ("catchhip_rows_extend", "catchhip_setcover_grid", "catchhip_rows_fetch_gain0",
                 "catchhip_ctx_last_grid_counters"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
    assert "grid.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------ GPU
def _multichrom_targets():
    """Genomes of several chromosomes: sequences shorter than 2e, sequences shorter than a probe, repeats that put
    hits at both ends of a sequence and runs that touch across a boundary."""
    rng = np.random.default_rng(17)
    unit = "".join(rng.choice(list("ACGT"), size=120))
    genomes = []
    for gi in range(5):
        seqs = []
        for ln in rng.integers(40, 400, size=4):
            body = "".join(rng.choice(list("ACGT"), size=int(ln)))
            seqs.append(unit[:60] + body + unit[-60:])    # a probe's window at both ends
        seqs.append(unit[60:])                             # 60 bases: shorter than 2e at e >= 31
        seqs.append(unit[:60])                             # touches the next sequence's start (unit[60:])
        seqs.append(unit[60:] + unit)
        genomes.append(seqs)
    probes = sorted({unit[i:i + 40] for i in range(0, 81, 8)} |
                    {s[j:j + 40] for g in genomes for s in g[:2] for j in range(0, len(s) - 40, 37)})
    return genomes, probes


def _fetch_sorted(rows):
    si, un, st, en = rows.fetch()
    return np.stack([si.astype(np.int64), un.astype(np.int64), st, en], axis=1)


def _ebola(n):
    from catch_amd.utils import seq_io
    return [g.seqs for g in seq_io.read_genomes_from_fasta(EBOLA)[:n]]


@pytest.mark.gpu
def test_rows_extend_equals_scan_at_each_extension(ctx):
    """catchhip_rows_extend(scan at 0, e) == catchhip_cover_scan at e, row for row, with the same gain0, for every
    scan mode that takes the input."""
    from catch_amd import engine, probe
    genomes, probes_ = _multichrom_targets()
    cases = [(genomes, probes_, 2, 40)]
    eb = _ebola(6)
    cands = list(dict.fromkeys(s[j:j + 100] for g in eb for s in g for j in range(0, len(s) - 100, 50)))
    cases.append((eb, cands, 3, 100))
    longest = max(len(s) for g, _, _, _ in cases for gg in g for s in gg)
    exts = [0, 1, 7, 50, 200, longest + 1]
    modes_run = 0
    for genomes_, strs, m, L in cases:
        k, uniq, owner, ep, eo = probe.anchor_table(strs, m, L, min_k=20, k=20)
        targets = engine.Targets(ctx, genomes_)
        probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
        try:
            for mode in (engine.SCAN_AUTO, engine.SCAN_GENERAL, engine.SCAN_FAST, engine.SCAN_SEED):
                try:
                    r0 = engine.Rows.scan(ctx, probes, targets, m, L, 0, 0, mode)
                except ValueError:
                    continue                      # the mode does not take this input
                modes_run += 1
                try:
                    derived = r0.extend(targets, exts)
                    for e, rd in zip(exts, derived):
                        rs = engine.Rows.scan(ctx, probes, targets, m, L, 0, e, mode)
                        try:
                            assert rd.n == rs.n, (mode, e)
                            assert np.array_equal(_fetch_sorted(rd), _fetch_sorted(rs)), (mode, e)
                            gs, gd = rs.fetch_gain0(len(uniq)), rd.fetch_gain0(len(uniq))
                            if gs is not None and gd is not None:
                                n = min(len(gs), len(gd))
                                assert np.array_equal(gs[:n], gd[:n]), (mode, e)
                            _, _, st, en = rd.fetch()
                            si = rd.fetch()[0]
                            want = np.bincount(si, weights=(en - st), minlength=len(uniq))
                            if gd is not None:
                                assert np.array_equal(gd[:len(uniq)].astype(np.int64),
                                                      want[:len(gd)].astype(np.int64)), (mode, e)
                            assert rd.greedy(len(uniq)) == rs.greedy(len(uniq)), (mode, e)
                        finally:
                            rs.close()
                            rd.close()
                finally:
                    r0.close()
        finally:
            probes.close()
            targets.close()
    assert modes_run >= 4


@pytest.mark.gpu
def test_rows_extend_rejects_bad_input(ctx):
    from catch_amd import engine, probe
    genomes, strs = _multichrom_targets()
    k, uniq, owner, ep, eo = probe.anchor_table(strs, 1, 40, min_k=20, k=20)
    targets = engine.Targets(ctx, genomes)
    probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
    try:
        r0 = engine.Rows.scan(ctx, probes, targets, 1, 40, 0, 0)
        r5 = engine.Rows.scan(ctx, probes, targets, 1, 40, 0, 5)
        try:
            with pytest.raises(ValueError):
                r0.extend(targets, [3, -1])
            with pytest.raises(ValueError):
                r5.extend(targets, [10])          # not scanned at e = 0
            grouped_p = engine.Probes(ctx, uniq, owner, ep, eo, k)
            grouped_t = engine.Targets(ctx, genomes)
            grouped_p.set_groups(np.zeros(len(uniq), dtype=np.int32))
            grouped_t.set_groups(np.zeros(len(genomes), dtype=np.int32))
            rg = engine.Rows.scan(ctx, grouped_p, grouped_t, 1, 40, 0, 0)
            try:
                with pytest.raises(ValueError):
                    rg.extend(grouped_t, [10])    # a union scan
            finally:
                rg.close()
                grouped_p.close()
                grouped_t.close()
        finally:
            r0.close()
            r5.close()
    finally:
        probes.close()
        targets.close()


def _write_fasta(path, genomes):
    with open(path, "w") as f:
        for j, g in enumerate(genomes):
            f.write(">g%d\n%s\n" % (j, "".join(g)))
    return str(path)


def _synthetic_fastas(tmp_path):
    from catch_amd.utils import synthetic
    rng = np.random.Generator(np.random.PCG64(23))
    a = synthetic.make_species(rng, [3000], 6, 2, 0.05, 0.01)
    b = synthetic.make_species(rng, [2200], 5, 3, 0.06, 0.02)
    return [_write_fasta(tmp_path / "sp_a.fasta", a), _write_fasta(tmp_path / "sp_b.fa", b)]


def _ebola_fasta(tmp_path, n=30):
    from catch_amd.utils import seq_io
    recs = list(seq_io.read_fasta(EBOLA).items())[:n]
    path = tmp_path / "ebola30.fasta"
    with open(path, "w") as f:
        for h, s in recs:
            f.write(">%s\n%s\n" % (h, s))
    return str(path)


def _run_grid_cli(files, ms, es, outdir, opts, seed=None, table=None):
    from catch_amd import design_grid
    argv = list(files) + ["--grid-mismatches"] + [str(m) for m in ms] + \
        ["--grid-cover-extension"] + [str(e) for e in es] + ["-o", str(outdir)] + list(opts)
    if table:
        argv += ["--write-probe-count-table", str(table)]
    if seed is not None:
        np.random.seed(seed)
        random.seed(seed)
    return design_grid.main(design_grid.parse_args(argv))


VARIANTS = [
    ("dup", ["-pl", "75", "-ps", "25"], 4),
    ("hamming", ["-pl", "75", "-ps", "25", "--filter-with-lsh-hamming", "2"], 5),
    ("minhash", ["-pl", "75", "-ps", "25", "--filter-with-lsh-minhash", "0.6"], 6),
    ("random_anchors", ["-pl", "75", "-ps", "25", "-l", "60"], 7),
    ("partial", ["-pl", "75", "-ps", "25", "-c", "0.9"], 8),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts,seed", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_grid_equals_separate_design_runs(ctx, tmp_path, capsys, name, opts, seed):
    """Every point's FASTA equals `catch_amd.design` run alone with the same options and seeds.  (-pl 75 at m = 3
    takes random anchors -- 4 x 20 > 75 -- so every variant seeds np.random and random before each run.)"""
    from catch_amd import design
    files = _synthetic_fastas(tmp_path)
    if name == "dup":
        files.append(_ebola_fasta(tmp_path))
    ms, es = [0, 1, 2, 3], [0, 25, 50]
    outdir = tmp_path / "grid"
    counts = _run_grid_cli(files, ms, es, outdir, opts, seed=seed, table=tmp_path / "t.tsv")
    capsys.readouterr()
    assert len(counts) == len(files) * len(ms) * len(es)
    from catch_amd import grid
    for fn in files:
        d = grid.dataset_name(fn)
        for m in ms:
            for e in es:
                single = tmp_path / ("single.%s.m%d.e%d.fasta" % (d, m, e))
                if seed is not None:
                    np.random.seed(seed)
                    random.seed(seed)
                design.main(design.parse_args([fn, "-m", str(m), "-e", str(e), "-o", str(single)] + opts))
                printed = int(capsys.readouterr().out.strip().splitlines()[-1])
                got = (outdir / ("%s.m%d.e%d.fasta" % (d, m, e))).read_bytes()
                assert got == single.read_bytes(), (d, m, e)
                assert (d, m, e, printed) in counts


@pytest.mark.gpu
def test_grid_equals_rescan_and_scans_once_per_dataset_and_m(ctx, tmp_path, monkeypatch):
    """CATCHHIP_GRID_RESCAN=1 (a scan at every e) selects the same probes; without it the scan runs once per
    (dataset, m) and every extension is derived."""
    from catch_amd import engine, grid
    from catch_amd.utils import seq_io
    files = _synthetic_fastas(tmp_path) + [_ebola_fasta(tmp_path, 12)]
    datasets = [seq_io.read_genomes_from_fasta(fn) for fn in files]
    ms, es = [0, 2, 3], [0, 10, 25, 50]
    calls = []
    real = engine.setcover_grid

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(engine, "setcover_grid", counting)
    st = {}
    np.random.seed(3)
    random.seed(3)
    got = grid.design_grid(datasets, ms, es, probe_length=75, probe_stride=25, stats=st)
    assert len(calls) == len(datasets) * len(ms)
    assert st["scans"] == len(datasets) * len(ms)
    assert st["derived"] == st["solves"] == len(datasets) * len(ms) * len(es)
    monkeypatch.setenv("CATCHHIP_GRID_RESCAN", "1")
    st2 = {}
    np.random.seed(3)
    random.seed(3)
    again = grid.design_grid(datasets, ms, es, probe_length=75, probe_stride=25, stats=st2)
    assert st2["scans"] == len(datasets) * len(ms) * len(es) and st2["derived"] == 0
    assert got == again
    assert sum(len(v) for v in got.values()) > 0


def _digest(strs):
    return hashlib.sha256(",".join(sorted(strs)).encode()).hexdigest()


@pytest.mark.gpu
def test_grid_points_equal_recorded_live_reference_runs(ctx):
    """Points of a grid over the Ebola records reproduce the live reference's recorded selections
    (tests/golden/real_runs.json) -- full and partial coverage, pigeonhole and random anchors."""
    from catch_amd import grid
    from catch_amd.utils import seq_io
    with open(os.path.join(GOLDEN, "real_runs.json")) as f:
        d = json.load(f)
    genomes_all = seq_io.read_genomes_from_fasta(EBOLA)
    checked = 0
    for r in d["runs"]:
        if r["records"] != 30:
            continue
        pl = r["probe_length"]
        ms = sorted({r["mismatches"], 0, 1})
        es = sorted({r["cover_extension"], 0, 25})
        if r["np_random_seed"] is not None:
            np.random.seed(r["np_random_seed"])
        got = grid.design_grid([genomes_all[:30]], ms, es, probe_length=pl, probe_stride=pl // 2,
                               lcf_thres=r["lcf_thres"], coverage=r["coverage"])
        sel = got[(0, r["mismatches"], r["cover_extension"])]
        assert len(sel) == r["probes_out"], r
        assert _digest(sel) == r["picks_sha256"], r
        checked += 1
    assert checked >= 4


@pytest.mark.gpu
def test_grid_table_equals_live_reference_grid(ctx, tmp_path, capsys):
    """The grid's table and picks over 30 Ebola records equal the live reference run at every point
    (tests/golden/grid_runs.json, made by tests/golden/make_grid_golden.py)."""
    with open(os.path.join(GOLDEN, "grid_runs.json")) as f:
        d = json.load(f)
    ms = sorted({p["mismatches"] for p in d["points"]})
    es = sorted({p["cover_extension"] for p in d["points"]})
    assert len(d["points"]) == len(ms) * len(es) == 12
    fn = _ebola_fasta(tmp_path, d["records"])
    outdir = tmp_path / "grid"
    table = tmp_path / "num-probes.tsv"
    _run_grid_cli([fn], ms, es, outdir, ["-pl", str(d["probe_length"]), "-ps", str(d["probe_stride"])],
                  table=table)
    lines = table.read_text().splitlines()
    want = ["dataset\tmismatches\tcover_extension\tnum_probes"] + [
        "ebola30\t%d\t%d\t%d" % (p["mismatches"], p["cover_extension"], p["num_probes"]) for p in d["points"]]
    assert lines == want
    from catch_amd.utils import seq_io
    for p in d["points"]:
        fa = outdir / ("ebola30.m%d.e%d.fasta" % (p["mismatches"], p["cover_extension"]))
        assert _digest(seq_io.read_fasta(str(fa)).values()) == p["picks_sha256"], p
