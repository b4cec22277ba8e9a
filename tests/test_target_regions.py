"""Target regions (--target-regions / --exclude-regions): the BED layer (catch_amd/target_regions.py), the base mask
and the two calls that read it (csrc/mask.hip: catchhip_basemask_*, catchhip_rows_restrict; csrc/gaps.hip:
catchhip_rows_uncovered_within), SetCoverFilter(target_regions=...), Analyzer(target_regions=...) and the two command
lines.

The build kernel takes a lane per 64-bit word of the bitmap: a wavefront holds 64 words = 4,096 bases, a workgroup
256 words = 16,384 bases.  The hand-made mask cases put intervals and universe boundaries on those two edges (and on
base 8,192, the workgroup edge of depth.hip's walk, which the counting was modelled on)."""
import inspect
import logging
import os
import random
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBOLA = os.path.join(REPO, "tests", "golden", "ebola_zaire_100.fasta.gz")


# ------------------------------------------------------------------ host models
def _offsets(glen):
    return np.concatenate([[0], np.cumsum(np.asarray(glen, dtype=np.int64))]).astype(np.int64)


def _wanted_bits(glen, iv):
    """bool per base of the concatenated universes: base lies in an interval of iv = [(universe, start, end)]."""
    off = _offsets(glen)
    w = np.zeros(int(off[-1]), dtype=bool)
    for u, s, e in iv:
        w[off[u] + s:off[u] + e] = True
    return w


def _np_words(wanted):
    """The bitmap the device builds: bit set = NOT wanted, the bits behind the last base set."""
    nw = (wanted.size + 63) // 64
    un = np.ones(nw * 64, dtype=bool)
    un[:wanted.size] = ~wanted
    return np.packbits(un, bitorder="little").view(np.uint64)


def _runs(bits):
    edge = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    return np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)


def _np_cut(rows, wanted, glen):
    """Every row (set, universe, start, end) cut into its maximal runs of wanted bases, in row order."""
    si, un, st, en = (np.asarray(a, dtype=np.int64) for a in rows)
    off = _offsets(glen)
    run_s, run_e = _runs(wanted)
    gs, ge = off[un] + st, off[un] + en
    k0 = np.searchsorted(run_e, gs, side="right")
    k1 = np.searchsorted(run_s, ge, side="left")
    cnt = np.maximum(k1 - k0, 0)
    row = np.repeat(np.arange(si.size), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(k0, cnt)
    ps, pe = np.maximum(run_s[k], gs[row]), np.minimum(run_e[k], ge[row])
    return si[row].astype(np.int32), un[row].astype(np.int32), ps - off[un[row]], pe - off[un[row]]


def _complement_table(wanted, glen):
    """The unwanted bases as the rows of one set, a table Rows.from_host takes."""
    off = _offsets(glen)
    out = []
    for u in range(len(glen)):
        s, e = _runs(~wanted[off[u]:off[u + 1]])
        out += [(0, u, int(a), int(b)) for a, b in zip(s, e)]
    return _table(out)


def _table(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].copy(), a[:, 3].copy()


def _normal_form(rng, length, most):
    """Up to `most` sorted intervals of [0, length), neither overlapping nor touching."""
    if length < 1 or most < 1:
        return []
    cuts = np.unique(rng.integers(0, length + 1, size=2 * int(rng.integers(0, most + 1))))
    cuts = cuts[:cuts.size // 2 * 2]
    return [(int(a), int(b)) for a, b in zip(cuts[0::2], cuts[1::2])]


def _mask(ctx, glen, iv):
    from catch_amd import engine
    a = np.array(iv, dtype=np.int64).reshape(-1, 3)
    return engine.BaseMask(ctx, glen, a[:, 0], a[:, 1], a[:, 2])


def _check_mask(ctx, glen, iv, tag):
    wanted = _wanted_bits(glen, iv)
    off = _offsets(glen)
    m = _mask(ctx, glen, iv)
    try:
        got = m.fetch()
        want = _np_words(wanted)
        assert got.dtype == np.uint64 and got.size == want.size, tag
        assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:5])
        per = [int(wanted[off[u]:off[u + 1]].sum()) for u in range(len(glen))]
        assert m.wanted.tolist() == per, tag
    finally:
        m.close()


# ------------------------------------------------------------------ without a GPU: BED reader
def _fasta(tmp_path, name="a.fasta", records=None):
    records = records or [("s1 first record", "ACGT" * 50), ("s2", "ACGT" * 25), ("third one", "A" * 64)]
    fa = tmp_path / name
    fa.write_text("".join(">%s\n%s\n" % r for r in records))
    return fa


def _regions(tmp_path, target=None, exclude=None, fasta=None):
    from catch_amd import target_regions as tr
    from catch_amd.utils import seq_io
    fa = fasta or _fasta(tmp_path)
    genomes, names = seq_io.read_named_genomes_from_fasta(str(fa))
    paths = []
    for tag, text in (("t", target), ("x", exclude)):
        if text is None:
            paths.append(None)
        else:
            p = tmp_path / ("%s.bed" % tag)
            p.write_text(text)
            paths.append([str(p)])
    return tr.TargetRegions.from_bed(paths[0], paths[1], [names], [genomes]), genomes, names


def test_read_named_genomes_keeps_the_headers(tmp_path):
    from catch_amd.utils import seq_io
    fa = _fasta(tmp_path)
    genomes, names = seq_io.read_named_genomes_from_fasta(str(fa))
    assert names == ["s1 first record", "s2", "third one"] == list(seq_io.read_fasta(str(fa)).keys())
    assert [g.seqs for g in genomes] == [g.seqs for g in seq_io.read_genomes_from_fasta(str(fa))]


def test_bed_reader_names_comments_columns_and_merging(tmp_path):
    bed = ("# a comment\ntrack name=x\nbrowser position s1:1-2\n\n"
           "s1\t10\t20\tgene\t0\t+\n"            # first token, tabs, extra columns
           "s1 first record\t15\t30\n"          # whole header (tab-separated: the name holds spaces)
           "s1 30 40\n"                          # touching, space-separated
           "s1 100 150\ns1 120 130\n"            # contained
           "s2 7 7\n"                            # empty: ignored
           "third 0 64\n")
    R, genomes, _names = _regions(tmp_path, target=bed)
    assert [a.tolist() for a in R.per_group[0]] == [[[0, 10, 40], [0, 100, 150]], [], [[0, 0, 64]]]
    assert R.summary(0, genomes) == (3, 30 + 50 + 64, 200 + 100 + 64, 2, 3)
    un, st, en = R.genome_intervals(0, genomes)
    assert (un.tolist(), st.tolist(), en.tolist()) == ([0, 0, 2], [10, 100, 0], [40, 150, 64])
    flat = [(0, j, g) for j, g in enumerate(genomes)]
    un, st, en = R.sequence_intervals(flat, rc=True)
    assert (un.tolist(), st.tolist(), en.tolist()) == ([0, 0, 2], [50, 160, 0], [100, 190, 64])


def test_bed_target_minus_exclude_and_exclude_alone(tmp_path):
    R, _g, _n = _regions(tmp_path, target="s1 10 100\ns2 0 100\n", exclude="s1 0 20\ns1 50 60\ns1 99 200\ns2 0 100\n")
    assert [a.tolist() for a in R.per_group[0]] == [[[0, 20, 50], [0, 60, 99]], [], []]
    X, _g, _n = _regions(tmp_path, exclude="s1 0 20\ns1 50 60\n")
    assert [a.tolist() for a in X.per_group[0]] == [[[0, 20, 50], [0, 60, 200]], [[0, 0, 100]], [[0, 0, 64]]]
    # a chrom applies to every record of every dataset it names
    from catch_amd import target_regions as tr
    from catch_amd.utils import seq_io
    g, n = seq_io.read_named_genomes_from_fasta(str(_fasta(tmp_path)))
    bed = tmp_path / "two.bed"
    bed.write_text("s2 1 9\n")
    both = tr.TargetRegions.from_bed([str(bed)], None, [n, n], [g, g])
    assert [[a.tolist() for a in grp] for grp in both.per_group] == [[[], [[0, 1, 9]], []]] * 2
    assert [a.tolist() for a in both.select([[1, 1, 0], [2]]).per_group[0]] == [[[0, 1, 9]], [[0, 1, 9]], []]


@pytest.mark.parametrize("line, what", [
    ("s1 20 10", "start 20 is greater than end 10"),
    ("s1 -5 10", "negative"),
    ("s1 1.5 10", "not integers"),
    ("s1 a 10", "not integers"),
    ("s2 0 101", "end 101 lies beyond the 100 bases"),
    ("nobody 0 10", "'nobody' names no sequence"),
    ("s1 10", "fewer than three columns"),
])
def test_bed_errors_name_file_and_line(tmp_path, line, what):
    with pytest.raises(ValueError, match=r"t\.bed:3: .*" + re.escape(what)):
        _regions(tmp_path, target="# header\ns1 0 10\n" + line + "\n")
    with pytest.raises(ValueError, match=r"x\.bed:3: .*" + re.escape(what)):
        _regions(tmp_path, exclude="# header\ns1 0 10\n" + line + "\n")


def test_bed_error_lists_at_most_five_offenders(tmp_path):
    with pytest.raises(ValueError) as info:
        _regions(tmp_path, target="".join("zz%d 0 1\n" % i for i in range(8)))
    msg = str(info.value)
    assert msg.count("names no sequence") == 5 and "t.bed:5" in msg and "t.bed:6" not in msg and "3 more" in msg


def test_interval_algebra_against_bit_vectors():
    from catch_amd import target_regions as tr
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 200))
        raw = [[(int(a), int(min(n, a + rng.integers(0, 30)))) for a in rng.integers(0, n, size=rng.integers(0, 8))]
               for _k in range(2)]
        bits = []
        for r in raw:
            b = np.zeros(n, dtype=bool)
            for s, e in r:
                b[s:e] = True
            bits.append(b)
        a, b = tr.union(raw[0]), tr.union(raw[1])
        for iv, bb in ((a, bits[0]), (b, bits[1]), (tr.subtract(a, b), bits[0] & ~bits[1])):
            s, e = _runs(bb)
            assert iv.tolist() == [[int(x), int(y)] for x, y in zip(s, e)]


# ------------------------------------------------------------------ without a GPU: sampling, refusals, surface
def test_sampling_with_replacement_carries_the_regions_and_draws_what_it_drew(tmp_path):
    from catch_amd import design
    recs = [("g%d" % i, "ACGT" * (30 + i)) for i in range(7)]
    fa = _fasta(tmp_path, "many.fasta", recs)
    R, genomes, _names = _regions(tmp_path, target="".join("g%d %d %d\n" % (i, i, 50 + i) for i in range(7)), fasta=fa)
    base = [str(fa), "-o", str(tmp_path / "o.fasta"), "--limit-target-genomes-randomly-with-replacement", "9"]
    random.seed(42)
    ref = random.choices(genomes, k=9)          # what the code drew before the option existed
    state_ref = random.getstate()
    random.seed(42)
    plain, none = design.limit_target_genomes(design.parse_args(base), [genomes], None)
    state_plain = random.getstate()
    random.seed(42)
    kept, regions = design.limit_target_genomes(design.parse_args(base + ["--target-regions", "x"]), [genomes], R)
    assert random.getstate() == state_plain == state_ref and none is None
    assert all(a is b and a is c for a, b, c in zip(ref, plain[0], kept[0])) and len(kept[0]) == 9
    idx = [genomes.index(g) for g in kept[0]]
    assert len(set(idx)) < 9
    assert [a.tolist() for a in regions.per_group[0]] == [[[0, i, 50 + i]] for i in idx]
    first, fr = design.limit_target_genomes(design.parse_args(base[:3] + ["--limit-target-genomes", "3"]), [genomes], R)
    assert first[0] == genomes[:3] and [a.tolist() for a in fr.per_group[0]] == [[[0, i, 50 + i]] for i in range(3)]


def test_command_line_refusals(tmp_path, capsys):
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd import design, design_grid
    fa = tmp_path / "t.fasta"
    fa.write_text(">a\n" + "ACGT" * 100 + "\n")
    bed = tmp_path / "r.bed"
    bed.write_text("a 10 200\n")
    base = [str(fa), "-o", str(tmp_path / "o.fasta")]
    for opt in ("--target-regions", "--exclude-regions"):
        with pytest.raises(Exception, match="Cannot use %s with --skip-set-cover" % opt):
            design.main(design.parse_args(base + [opt, str(bed), "--skip-set-cover"]))
        with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):
            design.main(design.parse_args(base + [opt, str(bed), "--cluster-and-design-separately", "0.1"]))
        with pytest.raises(Exception, match="--cluster-and-design-separately to 0"):     # design_large's default
            design.main(design.parse_args(base + [opt, str(bed)], args_type="large"))
        with pytest.raises(Exception, match="--cluster-from-fragments to 0"):     # design_large with clustering alone off
            design.main(design.parse_args(base + [opt, str(bed), "--cluster-and-design-separately", "0"],
                                          args_type="large"))
    # what the message advises parses
    args = design.parse_args(base + ["--target-regions", str(bed), "--cluster-and-design-separately", "0",
                                     "--cluster-from-fragments", "0"], args_type="large")
    assert not args.cluster_and_design_separately and not args.cluster_from_fragments
    # input errors are plain exceptions of main, before anything is designed
    bad = tmp_path / "bad.bed"
    bad.write_text("a 10 500\n")
    with pytest.raises(Exception, match=r"bad\.bed:1: end 500 lies beyond the 400 bases of 'a'"):
        design.main(design.parse_args(base + ["--target-regions", str(bad)]))
    assert not os.path.exists(str(tmp_path / "o.fasta"))
    # the other command lines do not know the options
    with pytest.raises(SystemExit):
        design_grid.parse_args([str(fa), "--grid-mismatches", "0", "--grid-cover-extension", "0", "-o",
                                str(tmp_path / "grid"), "--target-regions", str(bed)])
    assert "unrecognized arguments" in capsys.readouterr().err
    # the analysis takes them only for the uncovered-region outputs
    with pytest.raises(SystemExit):
        apc.parse_args(["-d", str(fa), "-f", str(fa), "-m", "0", "-l", "100", "--target-regions", str(bed)])
    assert "--write-uncovered-regions" in capsys.readouterr().err
    ok = apc.parse_args(["-d", str(fa), "-f", str(fa), "-m", "0", "-l", "100", "--exclude-regions", str(bed),
                         "--write-uncovered-fasta", str(tmp_path / "g.fasta")])
    assert ok.exclude_regions == [str(bed)]


def test_more_than_one_rank_is_refused(monkeypatch):
    from catch_amd import parallel
    from catch_amd.filter import set_cover_filter as scf

    class W:
        size = 2
    monkeypatch.setattr(parallel, "world", lambda: W())
    f = scf.SetCoverFilter(2, 100, target_regions=[[np.zeros((0, 3), dtype=np.int64)]])
    assert f.needs_rows
    with pytest.raises(NotImplementedError, match="target regions"):
        f._filter_strs([["ACGT" * 25]], [[]])


def test_symbols_are_declared_bound_and_wrapped():
    from catch_amd import _lib, coverage_analysis, engine, target_regions
    from catch_amd.filter import set_cover_filter as scf
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name, nargs in (("catchhip_basemask_create", 9), ("catchhip_basemask_fetch", 3),
                        ("catchhip_basemask_destroy", 1), ("catchhip_rows_restrict", 5),
                        ("catchhip_rows_uncovered_within", 10), ("catchhip_rows_uncovered", 9)):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert "mask.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    for attr in ("fetch", "close", "__del__"):
        assert callable(getattr(engine.BaseMask, attr))
    assert callable(engine.Rows.restrict)
    assert "mask" in inspect.signature(engine.Rows.uncovered).parameters
    assert list(inspect.signature(coverage_analysis.Analyzer.__init__).parameters)[-1] == "target_regions"
    assert callable(target_regions.add_arguments) and callable(target_regions.from_args)
    # the keyword is taken by the metaclass: __init__ stays the reference's argument list + fixed_probes
    params = list(inspect.signature(scf.SetCoverFilter.__init__).parameters)
    assert params[-1] == "fixed_probes" and "target_regions" not in params and len(params) == 16
    f = scf.SetCoverFilter(2, 100)
    assert f.target_regions is None and not f.needs_rows


# ------------------------------------------------------------------ gpu: the mask
def _hand_made_masks():
    big = 3_000_100
    return {
        "[0,1)": ([200], [(0, 0, 1)]),
        "[63,64)": ([200], [(0, 63, 64)]),
        "[63,65)": ([200], [(0, 63, 65)]),
        "[64,128)": ([200], [(0, 64, 128)]),
        "[0,total)": ([200], [(0, 0, 200)]),
        "three intervals inside one word": ([200], [(0, 65, 70), (0, 71, 72), (0, 120, 127)]),
        "five intervals inside one word": ([128], [(0, 64, 65), (0, 66, 67), (0, 70, 90), (0, 91, 92), (0, 126, 128)]),
        "32 intervals inside one word": ([64], [(0, 2 * i, 2 * i + 1) for i in range(32)]),
        "to the last base, total % 64 == 0": ([128], [(0, 100, 128)]),
        "to the last base, total % 64 == 1": ([129], [(0, 100, 129)]),
        "to the last base, total % 64 == 63": ([127], [(0, 64, 127)]),
        "universes 0, 1, 63, 64, 65": ([0, 1, 63, 64, 65], [(1, 0, 1), (2, 0, 63), (3, 0, 64), (4, 0, 65)]),
        "boundaries inside a word, an empty universe in the middle": (
            [1, 63, 0, 64, 65], [(0, 0, 1), (1, 1, 62), (3, 63, 64), (4, 0, 1), (4, 64, 65)]),
        "an empty universe last": ([65, 64, 0], [(0, 60, 65), (1, 0, 3)]),
        "empty universes first and last, nothing wanted in between": ([0, 0, 100, 0], []),
        "n = 0": ([300, 50], []),
        "no universe": ([], []),
        "only empty universes": ([0, 0], []),
        "one interval of 3,000,000 bases": ([big], [(0, 50, 3_000_050)]),
        "across base 4,096 (the wavefront's edge)": ([10000], [(0, 4000, 4097), (0, 4100, 4200)]),
        "across base 8,192": ([10000], [(0, 8191, 8193)]),
        "across base 16,384 (the workgroup's edge)": ([20000], [(0, 16000, 16385), (0, 16390, 19999)]),
        "universe boundaries around the wavefront's and the workgroup's edge": (
            [4090, 10, 4092, 1, 0, 8191, 7, 3000],
            [(0, 0, 4090), (1, 0, 10), (2, 5, 4092), (3, 0, 1), (5, 1, 8190), (6, 0, 7), (7, 0, 1), (7, 2999, 3000)]),
        "many short universes inside one wavefront": ([37] * 300, [(u, u % 30, 37 - u % 5) for u in range(0, 300, 2)]),
    }


@pytest.mark.gpu
def test_basemask_hand_made_cases(ctx):
    for tag, (glen, iv) in _hand_made_masks().items():
        _check_mask(ctx, glen, iv, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_basemask_random_cases(ctx, seed):
    rng = np.random.default_rng(seed)
    glen = [int(x) for x in rng.integers(0, 3001, size=300)]
    for u in rng.integers(0, 300, size=20):
        glen[int(u)] = 0
    iv = [(u, s, e) for u, n in enumerate(glen) for s, e in _normal_form(rng, n, 8)]
    assert len(iv) > 500
    _check_mask(ctx, glen, iv, seed)


@pytest.mark.gpu
def test_basemask_refusals(ctx):
    glen = [100, 50]
    for iv, what in (([(0, 20, 30), (0, 5, 10)], "interval 1 .* is out of order"),
                     ([(1, 0, 5), (0, 5, 10)], "interval 1 .* is out of order"),
                     ([(0, 5, 20), (0, 10, 30)], "interval 1 .* overlaps or touches"),
                     ([(0, 5, 20), (0, 20, 30)], "interval 1 .* overlaps or touches"),
                     ([(0, 5, 20), (1, 0, 51)], r"interval 1 \(universe 1, \[0, 51\)\) ends beyond its universe"),
                     ([(0, 7, 7)], "interval 0 .* is empty"),
                     ([(0, -1, 7)], "interval 0 .* is empty or negative"),
                     ([(2, 0, 1)], "interval 0 .* universe out of range"),
                     ([(-1, 0, 1)], "interval 0 .* universe out of range")):
        with pytest.raises(ValueError, match="basemask_create: " + what):
            _mask(ctx, glen, iv)


# ------------------------------------------------------------------ gpu: restrict
def _from_host(ctx, table, glen):
    from catch_amd import engine
    return engine.Rows.from_host(ctx, table[0], table[1], table[2], table[3], glen)


def _random_table(rng, nsets, glen, per, gap_hi, len_hi):
    nuniv = len(glen)
    g = rng.integers(1, gap_hi, size=(nsets, nuniv, per))
    ln = rng.integers(1, len_hi, size=(nsets, nuniv, per))
    en = np.cumsum(g + ln, axis=2)
    st = en - ln
    si = np.broadcast_to(np.arange(nsets)[:, None, None], st.shape)
    un = np.broadcast_to(np.arange(nuniv)[None, :, None], st.shape)
    keep = en <= np.asarray(glen)[None, :, None]
    return si[keep].astype(np.int32), un[keep].astype(np.int32), st[keep], en[keep]


def _check_restrict(ctx, rows, glen, iv, tag):
    wanted = _wanted_bits(glen, iv)
    R, M = _from_host(ctx, rows, glen), _mask(ctx, glen, iv)
    C = _from_host(ctx, _complement_table(wanted, glen), glen)
    held = [R, M, C]
    try:
        D = R.restrict(M)
        held.append(D)
        S = R.subtract(C)
        held.append(S)
        want, got, sub = _np_cut(rows, wanted, glen), D.fetch(), S.fetch()
        assert D.n == want[0].size == S.n, tag
        for g, w, s, name in zip(got, want, sub, ("set", "universe", "start", "end")):
            assert np.array_equal(g, w) and np.array_equal(g, s), (tag, name)
        nsets = int(rows[0].max()) + 1 if rows[0].size else 0
        g0 = D.fetch_gain0(nsets)
        if D.n:
            sums = np.bincount(want[0], weights=(want[3] - want[2]).astype(np.float64), minlength=nsets)
            assert g0 is not None and np.array_equal(g0.astype(np.int64), sums.astype(np.int64)), tag
        return got
    finally:
        for h in reversed(held):
            h.close()


@pytest.mark.gpu
def test_rows_restrict_hand_made_and_random_tables(ctx):
    cases = {
        "a region inside a row, a row inside a region, a row outside": (
            [300], [(0, 0, 10, 50), (0, 0, 60, 70), (1, 0, 100, 200), (2, 0, 250, 300)], [(0, 20, 30), (0, 55, 210)]),
        "regions touching a row's ends": ([300], [(0, 0, 10, 50)], [(0, 0, 10), (0, 50, 60)]),
        "every other base of 257": ([400], [(0, 0, 10, 267)], [(0, s, s + 1) for s in range(10, 267, 2)]),
        "a row of 400 bases over word boundaries, more than five words": (
            [1000], [(0, 0, 60, 460), (1, 0, 63, 65), (2, 0, 0, 64)], [(0, 62, 66), (0, 127, 129), (0, 191, 257), (0, 459, 470)]),
        "across universes": ([100, 100, 28], [(0, 0, 90, 100), (0, 1, 0, 10), (0, 2, 0, 28)],
                             [(0, 95, 100), (1, 0, 5), (2, 27, 28)]),
        "everything wanted": ([64, 100], [(0, 1, 60, 100), (1, 0, 0, 64)], [(0, 0, 64), (1, 0, 100)]),
        "nothing wanted": ([64, 100], [(0, 1, 60, 100), (1, 0, 0, 64)], []),
        "an empty table": ([300], [], [(0, 10, 50)]),
    }
    for tag, (glen, rows, iv) in cases.items():
        got = _check_restrict(ctx, _table(rows), glen, iv, tag)
        if tag.startswith("every other base"):
            assert got[0].size == 129
        if tag in ("nothing wanted", "an empty table"):
            assert got[0].size == 0
    rng = np.random.default_rng(17)
    for case in range(40):
        glen = [int(x) for x in rng.integers(1, 2500, size=int(rng.integers(1, 6)))]
        rows = _random_table(rng, int(rng.integers(1, 12)), glen, 12, 60, 401)
        iv = [(u, s, e) for u, n in enumerate(glen) for s, e in _normal_form(rng, n, 8)]
        _check_restrict(ctx, rows, glen, iv, case)
    # ~19,000 rows of 1 to 400 bases: both branches at five words, more than one workgroup
    glen = [40000, 35001, 63]
    rows = _random_table(rng, 55, glen, 180, 40, 401)
    assert 15000 < rows[0].size <= 20000 and (rows[3] - rows[2]).max() > 320 and (rows[3] - rows[2]).min() == 1
    iv = [(u, s, e) for u, n in enumerate(glen) for s, e in _normal_form(rng, n, 400)]
    got = _check_restrict(ctx, rows, glen, iv, "large")
    assert got[0].size > 10000


@pytest.mark.gpu
def test_rows_restrict_refuses_a_mask_over_another_space(ctx):
    R = _from_host(ctx, _table([(0, 0, 10, 50), (0, 1, 0, 5)]), [100, 50])
    try:
        for glen in ([100, 51], [150], [100, 50, 1], [50, 100]):
            M = _mask(ctx, glen, [(0, 1, 2)])
            try:
                with pytest.raises(ValueError, match="rows_restrict: the mask is not over the coordinate space"):
                    R.restrict(M)
                with pytest.raises(ValueError, match="rows_uncovered: the mask is not over the coordinate space"):
                    R.uncovered(mask=M)
            finally:
                M.close()
    finally:
        R.close()


# ------------------------------------------------------------------ gpu: uncovered within
def _host_within(base, wanted_iv, seqs, min_length, min_unambig):
    """Rows.uncovered() without a mask (every run: min_length 1, min_unambig 0) -> what it reports within the wanted
    intervals: intersected with them, split at their edges, recounted, filtered again."""
    univ, st, en, _ua, _per = base
    by_u = {}
    for u, s, e in wanted_iv:
        by_u.setdefault(u, []).append((s, e))
    out = []
    for u, a, b in zip(univ.tolist(), st.tolist(), en.tolist()):
        for s, e in by_u.get(u, ()):
            lo, hi = max(a, s), min(b, e)
            if lo < hi:
                ua = sum(seqs[u][lo:hi].count(c) for c in "ACGT")
                if hi - lo >= min_length and ua >= min_unambig:
                    out.append((u, lo, hi, ua))
    per = np.zeros((len(seqs), 3), dtype=np.int64)
    for u, lo, hi, _ua in out:
        per[u, 0] += 1
        per[u, 1] += hi - lo
        per[u, 2] = max(per[u, 2], hi - lo)
    return out, per


@pytest.mark.gpu
@pytest.mark.parametrize("min_depth", [1, 2])
def test_uncovered_within_equals_the_host_derivation(ctx, min_depth):
    from catch_amd import engine
    rng = np.random.default_rng(300 + min_depth)
    reported = 0
    for case in range(25):
        glen = [int(x) for x in rng.integers(1, 700, size=int(rng.integers(1, 7)))]
        if case == 0:
            glen = [64, 1, 128, 4096, 65]
        seqs = ["".join(rng.choice(list("ACGTN"), p=[0.22, 0.22, 0.22, 0.22, 0.12], size=n)) for n in glen]
        rows = _random_table(rng, int(rng.integers(1, 6)), glen, 8, 50, 60)
        iv = [(u, s, e) for u, n in enumerate(glen) for s, e in _normal_form(rng, n, 6)]
        T = engine.Targets(ctx, [[s] for s in seqs])
        R, M = _from_host(ctx, rows, glen), _mask(ctx, glen, iv)
        try:
            base = R.uncovered(T, min_depth, 1, 0)
            for min_length, min_unambig in ((1, 0), (1, 1), (5, 3), (12, 0)):
                un, st, en, ua, per = R.uncovered(T, min_depth, min_length, min_unambig, mask=M)
                want, want_per = _host_within(base, iv, seqs, min_length, min_unambig)
                assert list(zip(un.tolist(), st.tolist(), en.tolist(), ua.tolist())) == want, (case, min_length)
                assert np.array_equal(per, want_per), (case, min_length)
                reported += len(want)
            # without targets every base counts
            un, st, en, ua, _per = R.uncovered(None, min_depth, 1, 1, mask=M)
            want, _p = _host_within(base, iv, ["A" * n for n in glen], 1, 1)
            assert list(zip(un.tolist(), st.tolist(), en.tolist(), ua.tolist())) == want, case
        finally:
            for h in (M, R, T):
                h.close()
    assert reported > 300


# ------------------------------------------------------------------ gpu: the filter
_cache = {}


def _genomes():
    if "g" not in _cache:
        from catch_amd.filter import candidate_probes
        from catch_amd.utils import seq_io
        g = seq_io.read_genomes_from_fasta(EBOLA)[:5]
        c = []
        for x in g:
            c += candidate_probes.candidate_strings_from_sequences(list(x.seqs), 100, 50)
        _cache["g"] = (g, list(dict.fromkeys(c)))
    return _cache["g"]


def _filter(e, coverage=1.0, **kw):
    from catch_amd.filter import set_cover_filter as scf
    return scf.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=coverage, cover_extension=e, **kw)


def _everything(genomes):
    return [[np.array([[0, 0, g.size()]], dtype=np.int64) for g in genomes]]


_REAL = [(2000, 5000), (9000, 9100)]


def _real_regions(genomes):
    """[2000, 5000) and [9000, 9100) of genomes 0-3, nothing of genome 4."""
    per = [np.array([[0, s, e] for s, e in _REAL], dtype=np.int64) for _g in genomes[:4]]
    return [per + [np.zeros((0, 3), dtype=np.int64)]], [(u, s, e) for u in range(4) for s, e in _REAL]


def _scan_rows(ctx, strs, genomes, e):
    """The device scan's rows of `strs`, fetched (made once per (candidates, e))."""
    key = ("scan", id(strs), e)
    if key not in _cache:
        from catch_amd import engine, probe
        k, uniq, _owner, ep, eo = probe.anchor_table(strs, 2, 100, min_k=20, k=20)
        assert uniq == list(strs)
        targets = engine.Targets(ctx, [g.seqs for g in genomes])
        probes = engine.Probes(ctx, uniq, np.arange(len(uniq), dtype=np.int32), ep, eo, k)
        try:
            rows = engine.Rows.scan(ctx, probes, targets, 2, 100, 0, e)
            _cache[key] = (rows.fetch(), strs)
            rows.close()
        finally:
            probes.close()
            targets.close()
    return _cache[key][0]


def _plain_design(e, coverage):
    key = ("plain", e, coverage)
    if key not in _cache:
        g, c = _genomes()
        _cache[key] = _filter(e, coverage)._filter_strs([c], [g], assume_unique=True)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_with_everything_wanted_is_the_filter_without_regions(ctx, e, coverage):
    g, c = _genomes()
    f = _filter(e, coverage, target_regions=_everything(g))
    assert f._filter_strs([c], [g], assume_unique=True) == _plain_design(e, coverage)
    assert f.last_wanted_bases == [sum(x.size() for x in g)]
    t = f.last_timings
    assert t["rows_restricted"] == t["rows"] > 0 and t["restrict_ms"] > 0 and t["mask_ms"] > 0
    assert not {"mask_ms", "restrict_ms", "rows_restricted"} & set(_filter(e, coverage, prune_redundant=True).last_timings)


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["fixed_probes", "coverage_depth", "prune_redundant", "max_probes"])
def test_filter_with_everything_wanted_under_the_other_rows_options(ctx, option):
    g, c = _genomes()
    e = 50
    plain = _plain_design(e, 1.0)[0]
    kw = dict(fixed_probes=[c[i] for i in plain[:len(plain) // 2]], coverage_depth=2, prune_redundant=True,
              max_probes=100)
    kw = {option: kw[option]}
    a, b = _filter(e, **kw), _filter(e, target_regions=_everything(g), **kw)
    want = a._filter_strs([c], [g], assume_unique=True)
    assert b._filter_strs([c], [g], assume_unique=True) == want and len(want[0]) > 0
    assert b.last_layer_sizes == a.last_layer_sizes
    assert b.last_pruned == a.last_pruned and b.last_budget_kept == a.last_budget_kept
    if option == "max_probes":
        assert all(np.array_equal(x, y) for x, y in zip(a.last_pick_gains, b.last_pick_gains))
        assert a.last_coverage_curve == b.last_coverage_curve


@pytest.mark.gpu
@pytest.mark.parametrize("coverage", [1.0, 0.9])
@pytest.mark.parametrize("e", [0, 50])
def test_filter_with_real_regions_equals_the_oracle_on_cut_rows(ctx, oracle, e, coverage):
    from catch_amd import engine
    g, c = _genomes()
    glen = [x.size() for x in g]
    regions, iv = _real_regions(g)
    f = _filter(e, coverage, target_regions=regions)
    got = f._filter_strs([c], [g], assume_unique=True)[0]
    cut = _np_cut(_scan_rows(ctx, c, g, e), _wanted_bits(glen, iv), glen)
    want = oracle.approx_multiuniverse(*cut, len(c), len(g), universe_p=[coverage] * len(g))
    assert got == want and len(got) > 0
    assert len(got) < len(_plain_design(e, coverage)[0])
    assert f.last_wanted_bases == [4 * 3100] and f.last_timings["rows_restricted"] == cut[0].size
    assert set(got) <= set(cut[0].tolist())            # every pick owns a restricted row
    # the device's own restricted table, and the picks replayed over it
    rows = _scan_rows(ctx, c, g, e)
    R, M = _from_host(ctx, rows, glen), _mask(ctx, glen, iv)
    D = R.restrict(M)
    try:
        assert M.wanted.tolist() == [3100] * 4 + [0]
        for a, b in zip(D.fetch(), cut):
            assert np.array_equal(a, b)
        assert f.last_coverable_bases == [int(D.stats(len(g))[1].sum())]
        chk = D.cover_check(len(c), got, None if coverage == 1.0 else [coverage] * len(g))
        assert chk["universes_short"] == 0 and chk["picks_without_gain"] == 0 and chk["bad_pick_ids"] == 0, chk
    finally:
        for h in (D, M, R):
            h.close()


def _np_subtract(rows, covered, glen):
    off = _offsets(glen)
    d = np.zeros(int(off[-1]) + 1, dtype=np.int64)
    cu, cs, ce = (np.asarray(a, dtype=np.int64) for a in covered[1:])
    np.add.at(d, off[cu] + cs, 1)
    np.add.at(d, off[cu] + ce, -1)
    return _np_cut(rows, np.cumsum(d[:-1]) == 0, glen)


def _union_len(table, glen):
    off = _offsets(glen)
    b = np.zeros(int(off[-1]), dtype=bool)
    for u, s, e in zip(*(np.asarray(a, dtype=np.int64) for a in table[1:])):
        b[off[u] + s:off[u] + e] = True
    return [int(b[off[u]:off[u + 1]].sum()) for u in range(len(glen))]


@pytest.mark.gpu
@pytest.mark.parametrize("e", [0, 50])
def test_filter_with_real_regions_and_fixed_probes(ctx, oracle, e):
    """The model of test_extend_probes.py on cut rows: candidates' and fixed probes' rows cut to the wanted bases,
    subtracted in NumPy, the fractions restated, the oracle's greedy."""
    from catch_amd.filter.set_cover_filter import extension_fraction
    g, c = _genomes()
    glen = [x.size() for x in g]
    regions, iv = _real_regions(g)
    wanted = _wanted_bits(glen, iv)
    alone = _filter(e, 0.9, target_regions=regions)._filter_strs([c], [g], assume_unique=True)[0]
    fixed = [c[i] for i in alone[::2]]
    _cache[("fixed", e)] = fixed                       # (kept alive: _scan_rows caches by identity)
    f = _filter(e, 0.9, target_regions=regions, fixed_probes=fixed)
    got = f._filter_strs([c], [g], assume_unique=True)[0]
    rows, cov = _np_cut(_scan_rows(ctx, c, g, e), wanted, glen), _np_cut(_scan_rows(ctx, fixed, g, e), wanted, glen)
    reduced = _np_subtract(rows, cov, glen)
    q = [extension_fraction(a, b, 0.9) for a, b in zip(_union_len(reduced, glen), _union_len(cov, glen))]
    want = oracle.approx_multiuniverse(*reduced, len(c), len(g), universe_p=q)
    assert got == want and 0 < len(got) < len(alone)
    # (the filter scans the fixed probes as one set: its rows_fixed counts their merged rows, not one table per probe)
    assert f.last_timings["rows_reduced"] == reduced[0].size and 0 < f.last_timings["rows_fixed"] <= cov[0].size


@pytest.mark.gpu
def test_a_group_without_a_wanted_base_selects_nothing_and_warns(ctx, caplog):
    g, c = _genomes()
    regions, _iv = _real_regions(g)
    none = [np.zeros((0, 3), dtype=np.int64) for _x in g]
    f = _filter(0, target_regions=[none, regions[0]])
    with caplog.at_level(logging.WARNING):
        got = f._filter_strs([c, c], [g, g], assume_unique=True)
    assert got[0] == [] and len(got[1]) > 0
    assert f.last_wanted_bases == [0, 4 * 3100]
    assert any("leave no base to cover" in r.getMessage() and "Group 1 of 2" in r.getMessage() for r in caplog.records)


@pytest.mark.gpu
def test_analyzer_without_probes_reports_every_wanted_interval(ctx, tmp_path):
    """No probes: every wanted interval that passes the filters is one region, on both strands."""
    from catch_amd import coverage_analysis
    R, genomes, _names = _regions(
        tmp_path, target="s1 10 40\ns1 100 150\nthird 0 32\n", exclude="s1 20 25\n",
        fasta=_fasta(tmp_path, records=[("s1 first record", "ACGT" * 50), ("s2", "ACGT" * 25),
                                        ("third one", "N" * 32 + "ACGT" * 8)]))
    a = coverage_analysis.Analyzer([], 0, 100, [genomes], target_regions=R)
    a.run()
    got = a.uncovered_regions(1, 1, 1)[0]
    assert got[0] == {False: [(0, 10, 20, 10), (0, 25, 40, 15), (0, 100, 150, 50)],
                      True: [(0, 50, 100, 50), (0, 160, 175, 15), (0, 180, 190, 10)]}
    assert got[1] == {False: [], True: []} == got[2]           # nothing wanted; wanted, but not one A, C, G or T
    assert a.uncovered_regions(1, 11, 0)[0][2] == {False: [(0, 0, 32, 0)], True: [(0, 32, 64, 0)]}
    assert a.uncovered_summary[0][0][False] == (2, 65, 50)


# ------------------------------------------------------------------ gpu: the command lines
def _read_gaps(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["Genome", "Sequence", "Start", "End", "Length", "Unambig bases"]
    return [tuple(l.split("\t")) for l in lines[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("rc", [False, True])
def test_design_command_line(ctx, tmp_path, caplog, rc):
    from catch_amd import analyze_probe_coverage as apc
    from catch_amd import coverage_analysis, design, probe
    from catch_amd.utils import seq_io
    g, c = _genomes()
    names = list(seq_io.read_fasta(EBOLA).keys())[:5]
    glen = [x.size() for x in g]
    r, x = tmp_path / "r.bed", tmp_path / "x.bed"
    r.write_text("# wanted\n" + "".join("%s\t%d\t%d\tregion\n" % (n.split()[0], s, e) for n in names[:4] for s, e in _REAL))
    x.write_text("%s\t2500\t2600\n%s 9050 9100\n" % (names[0], names[1].split()[0]))
    wanted_iv = sorted(set((u, s, e) for u in range(4) for s, e in _REAL) - {(0, 2000, 5000), (1, 9000, 9100)}
                       | {(0, 2000, 2500), (0, 2600, 5000), (1, 9000, 9050)})
    out, gaps, gfa = tmp_path / "out.fasta", tmp_path / "gaps.tsv", tmp_path / "gaps.fasta"
    argv = [EBOLA, "--limit-target-genomes", "5", "-m", "2", "-e", "50", "--target-regions", str(r),
            "--exclude-regions", str(x), "-o", str(out), "--write-uncovered-regions", str(gaps),
            "--write-uncovered-fasta", str(gfa), "--verbose"] + (["--add-reverse-complements"] if rc else [])
    with caplog.at_level(logging.INFO):
        design.main(design.parse_args(argv))
    # the probes are the library call's
    per = [np.array([[0, s, e] for u, s, e in wanted_iv if u == j], dtype=np.int64).reshape(-1, 3) for j in range(5)]
    f = _filter(50, target_regions=[per])
    picks = [c[i] for i in f._filter_strs([c], [g], assume_unique=True)[0]]
    written = list(seq_io.read_fasta(str(out)).values())
    rc_of = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))      # noqa: E731
    assert sorted(written) == sorted(set(picks) | ({rc_of(s) for s in picks} if rc else set())) and picks
    # the log line's numbers are the BED's
    nwanted = sum(e - s for _u, s, e in wanted_iv)
    line = [m.getMessage() for m in caplog.records if "target regions:" in m.getMessage()]
    assert len(line) == 1 and ("target regions: %d intervals, %d wanted bases of %d in 4 of 5 sequences; %d coverable"
                               % (len(wanted_iv), nwanted, sum(glen), f.last_coverable_bases[0])) in line[0], line
    # every row of the gaps file lies inside a wanted interval, and is what the host derives from the whole-genome gaps
    rows = _read_gaps(str(gaps))
    base = os.path.basename(EBOLA)
    analyzer = coverage_analysis.Analyzer([probe.Probe.from_str(s) for s in written], 2, 100, [g], [base],
                                          cover_extension=50, kmer_probe_map_k=10, rc_too=rc)
    analyzer.run()
    whole = analyzer.uncovered_regions(1, 1, 0)
    want = []
    for j in range(5):
        n = glen[j]
        for strand in ((False, True) if rc else (False,)):
            iv = [(s, e) for u, s, e in wanted_iv if u == j]
            if strand:
                iv = sorted((n - e, n - s) for s, e in iv)
            seq = rc_of(g[j].seqs[0]) if strand else g[j].seqs[0]
            for _s, a, b, _ua in whole[0][j][strand]:
                for s, e in iv:
                    lo, hi = max(a, s), min(b, e)
                    ua = sum(seq[lo:hi].count(ch) for ch in "ACGT") if lo < hi else 0
                    if lo < hi and ua >= 1:
                        want.append(("%s, genome %d%s" % (base, j, " (rc)" if strand else ""), "0", str(lo), str(hi),
                                     str(hi - lo), str(ua)))
    assert rows == want
    # at -c 1.0 a gap is a run no candidate covers
    cand = _scan_rows(ctx, c, g, 50)
    fwd = [row for row in rows if "(rc)" not in row[0]]
    for row in fwd:
        j, a, b = int(row[0].split("genome ")[1]), int(row[2]), int(row[3])
        m = cand[1] == j
        assert not ((cand[2][m] < b) & (cand[3][m] > a)).any(), row
    if rc:      # the rc rows are the forward rows mirrored
        mirrored = sorted((row[0] + " (rc)", glen[int(row[0].split("genome ")[1])] - int(row[3]),
                           glen[int(row[0].split("genome ")[1])] - int(row[2])) for row in fwd)
        assert sorted((row[0], int(row[2]), int(row[3])) for row in rows if "(rc)" in row[0]) == mirrored
    recs = seq_io.read_fasta(str(gfa))
    assert len(recs) == len(fwd) and all(len(s) == int(row[4]) for s, row in zip(recs.values(), fwd))
    if rc:
        # the analysis command (both strands always) writes the same rows for the probes written
        again = tmp_path / "again.tsv"
        apc.main(apc.parse_args(["-d", EBOLA, "--limit-target-genomes", "5", "-f", str(out), "-m", "2", "-l", "100",
                                 "-e", "50", "--target-regions", str(r), "--exclude-regions", str(x),
                                 "--write-uncovered-regions", str(again)]))
        assert _read_gaps(str(again)) == rows
