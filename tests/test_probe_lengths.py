"""Probe lengths 131-256 and beyond on every kernel whose shape depends on the length.

The rest of the suite stops at 130 bases (150 in the redundancy graph).  Above that the scan instantiates its
verify / join / extension kernels for 6, 7 and 8 words of 32 bases, loses the four-seed verify kernel at 8 words and
the packed probe image above 256 bases; the MinHash filter takes its four-slot rank loop above 128 k-mers and stops
at 256; the anchors of the device front end become host-made entries when L - k + 1 > 256.  Every comparison here is
bit-exact against the CPU oracle.  The tests without the gpu mark check, with the oracle alone, that the inputs sit
on the branch points they are there for.  (The poly(A) staging tiers are in test_design_filters.py, the redundancy
graph at four full plane words in test_naive.py, the first-seen scan at 224 bases in test_gpu_parity.py.)
"""
import random

import numpy as np
import pytest

import test_design_filters as tdf
import test_gpu_parity as gp
from util import candidates, small_species

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------ scan inputs
def _scan_genomes():
    """Six strains of 3 kb in two clades, close enough that a probe of 160-300 bases covers a second strain."""
    return _cached("scan genomes", lambda: small_species(seed=21, d1=0.015, d2=0.004))


# (L, stride, m, ext), words of 32 bases per probe, pigeonhole k
THRESHOLD_CASES = [
    ((161, 80, 2, 10), 6, 23),       # tail word of 1 bit
    ((192, 64, 5, 0), 6, 32),        # full tail word; 6 anchors in the table: no join, the seed list runs
    ((192, 96, 1, 25), 6, 96),
    ((224, 112, 2, 20), 7, 56),      # the last instantiation of the four-seed verify kernel
    ((225, 75, 2, 0), 8, 75),        # no four-seed verify kernel: one seed per lane, unfiltered look-up
    ((255, 85, 3, 5), 8, 51),
    ((256, 128, 3, 50), 8, 64),      # rows longer than 257 bases
    ((256, 64, 0, 0), 8, 256),       # one anchor per probe, the probe itself
    ((256, 128, 4, 0), 8, 32),       # five anchors in the table: the join's maximum
]
JOIN_MAX_ANCHORS = 5                 # KJ_AMAX of csrc/scan_join.inc


def _join_eligible(L, k, m):
    """join_path_ok of csrc/scan.hip for a pigeonhole table: the anchors below (m + 1) k number at most five."""
    return min(L // k, m + 1) <= JOIN_MAX_ANCHORS


def _threshold_case(oracle, L, stride, m, ext):
    def make():
        genomes = _scan_genomes()
        probes = candidates(genomes, L, stride)
        k, entries = oracle.anchor_table(probes, m, L)
        return dict(genomes=genomes, probes=probes, k=k, entries=entries,
                    rows=gp._oracle_rows(oracle, probes, genomes, m, L, 0, ext))
    return _cached(("threshold", L, stride, m, ext), make)


# (L, stride, m, thres, island, ext, np.random seed)
GENERAL_CASES = [
    (193, 90, 2, 193, 0, 0, 21),     # prime length: random anchors, L - k > 96: unfiltered look-up; the seed modes too
    (200, 100, 3, 150, 0, 10, 22),   # threshold below L, extension over 7 words
    (256, 128, 2, 256, 100, 0, 23),  # island of exact match
    (257, 128, 2, 257, 0, 0, 24),    # no packed image: seeds from the sort of byte hashes
    (300, 150, 2, 300, 0, 25, 25),   # pigeonhole k = 100, but not a table
    (300, 150, 3, 240, 40, 10, 26),  # above 256 with a threshold below L, island and extension
]
SEED_LOOKUP_HALO = 96                # SL_HALO of csrc/scan.hip: random anchors are filtered at look-up while L - k <= 96


def _general_case(oracle, L, stride, m, thres, island, ext, seed):
    def make():
        genomes = _scan_genomes()
        probes = candidates(genomes, L, stride)
        np.random.seed(seed)
        k, entries = oracle.anchor_table(probes, m, thres)
        np.random.seed(seed)
        return dict(genomes=genomes, probes=probes, k=k, entries=entries,
                    rows=gp._oracle_rows(oracle, probes, genomes, m, thres, island, ext))
    return _cached(("general", L, stride, m, thres, island, ext, seed), make)


# ------------------------------------------------------------------ no GPU: the inputs sit where they are claimed to
def test_threshold_scan_cases_sit_on_their_branch_points(oracle):
    for (L, stride, m, ext), nw, k in THRESHOLD_CASES:
        c = _threshold_case(oracle, L, stride, m, ext)
        nuniq = len(set(c["probes"]))
        assert (L + 31) // 32 == nw and c["k"] == k and L % k == 0 and L // k > m, (L, m)
        per_probe = np.bincount([e[0] for e in c["entries"]], minlength=nuniq)
        assert (per_probe == L // k).all(), (L, m)
        assert 134 <= nuniq <= 245 and all(len(p) == L for p in c["probes"])
        assert len(c["rows"]) >= 1.4 * nuniq if m >= 1 else len(c["rows"]) > nuniq, (L, m, len(c["rows"]), nuniq)
    by_case = {c[0]: c for c in THRESHOLD_CASES}
    assert sorted({c[1] for c in THRESHOLD_CASES}) == [6, 7, 8]
    assert 161 % 32 == 1 and 192 % 32 == 0 and 256 % 32 == 0            # the tail mask: one bit, all ones
    assert [cs for cs, _, k in THRESHOLD_CASES if not _join_eligible(cs[0], k, cs[2])] == [(192, 64, 5, 0)]
    assert 192 // by_case[(192, 64, 5, 0)][2] == 6
    assert min(256 // by_case[(256, 128, 4, 0)][2], 4 + 1) == JOIN_MAX_ANCHORS
    assert 256 // by_case[(256, 64, 0, 0)][2] == 1
    assert by_case[(224, 112, 2, 20)][1] == 7 and by_case[(225, 75, 2, 0)][1] == 8      # either side of the last verify4
    rows = _threshold_case(oracle, 256, 128, 3, 50)["rows"]
    assert max(e - s for _, _, s, e in rows) > 257


def test_general_scan_cases_sit_on_their_branch_points(oracle):
    facts = {}
    for L, stride, m, thres, island, ext, seed in GENERAL_CASES:
        c = _general_case(oracle, L, stride, m, thres, island, ext, seed)
        nprobes = len(c["probes"])
        assert nprobes == len(set(c["probes"])) >= 100 and all(len(p) == L for p in c["probes"])
        assert len(c["rows"]) >= 1.4 * nprobes, (L, m, thres, len(c["rows"]), nprobes)
        per_probe = np.bincount([e[0] for e in c["entries"]], minlength=nprobes)
        pigeonhole = thres == L and oracle.pigeonhole_k(L, m, 20) is not None
        if pigeonhole:
            assert c["k"] == oracle.pigeonhole_k(L, m, 20) and (per_probe == L // c["k"]).all()
        else:
            # the reference's 20 draws per probe with replacement: a few coincide
            assert c["k"] == 20 and 12 <= per_probe.min() and per_probe.max() <= 20
            assert max(e[1] for e in c["entries"]) > L - 20 - 10            # anchors reach the probe's end
        facts[(L, thres, island)] = (c["k"], pigeonhole)
    assert facts == {(193, 193, 0): (20, False), (200, 150, 0): (20, False), (256, 256, 100): (64, True),
                     (257, 257, 0): (20, False), (300, 300, 0): (100, True), (300, 240, 40): (20, False)}
    assert 193 - 20 > SEED_LOOKUP_HALO                                  # the look-up does not filter these anchors
    assert (200 + 31) // 32 == 7
    assert 300 - 20 + 1 > 256                                           # the front end makes these anchors on the host


# ------------------------------------------------------------------ 1. scan, full-length threshold
@pytest.mark.gpu
@pytest.mark.parametrize("L,stride,m,ext", [c[0] for c in THRESHOLD_CASES])
def test_scan_modes_match_oracle_at_6_to_8_words(ctx, oracle, monkeypatch, L, stride, m, ext):
    """The tiled scan, the seed join with its extension, the seed scan (the key-grouped join where the table holds at
    most five anchors per probe) and the seed-list scan, at 161-256 bases: the oracle's rows from each."""
    engine = gp._engine()
    c = _threshold_case(oracle, L, stride, m, ext)
    genomes, probes, exp = c["genomes"], c["probes"], c["rows"]
    assert gp._scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_FAST) == exp
    assert gp._scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_GENERAL) == exp
    got = gp._scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_SEED)
    joined = ctx.counters()["join_hit_positions"]
    assert got == exp
    assert (joined > 0) == _join_eligible(L, c["k"], m)
    monkeypatch.setenv("CATCHHIP_SEED_LIST", "1")
    got = gp._scan_rows(ctx, probes, genomes, m, L, 0, ext, engine.SCAN_SEED)
    assert ctx.counters()["join_hit_positions"] == 0
    assert got == exp


# ------------------------------------------------------------------ 2. scan, general mode and L > 256
@pytest.mark.gpu
@pytest.mark.parametrize("L,stride,m,thres,island,ext,seed", GENERAL_CASES)
def test_scan_general_matches_oracle_at_long_probes(ctx, oracle, L, stride, m, thres, island, ext, seed):
    """Random anchors, thresholds below L, islands and extensions at 193-300 bases.  Above 256 bases the probes have
    no packed image: the automatic choice and CATCHHIP_SCAN_GENERAL give the oracle's rows through the sort of byte
    hashes, and the tiled scan and the seed scan, asked for by name, are refused.

    No work counter tells the table look-up from the byte-hash join: both leave their seeds in seed_hits (and the
    join's counters keep the values of the last seed scan).  What the counters do show above 256 bases is a seed
    count consistent with the general path and that the look-up's filter dropped nothing."""
    engine = gp._engine()
    c = _general_case(oracle, L, stride, m, thres, island, ext, seed)
    genomes, probes, exp = c["genomes"], c["probes"], c["rows"]
    np.random.seed(seed)
    assert gp._scan_rows(ctx, probes, genomes, m, thres, island, ext) == exp
    counters = ctx.counters()
    if L > 256:
        # one extension per seed, at most one range from each, merged into the rows; nothing dropped at a look-up
        assert counters["seed_hits"] >= counters["raw_hits"] >= len(exp) and counters["seeds_dropped"] == 0
        np.random.seed(seed)
        assert gp._scan_rows(ctx, probes, genomes, m, thres, island, ext, engine.SCAN_GENERAL) == exp
        for mode, what in ((engine.SCAN_FAST, "fast-path"), (engine.SCAN_SEED, "seed-filter")):
            np.random.seed(seed)
            with pytest.raises(ValueError, match=what + " preconditions do not hold"):
                gp._scan_rows(ctx, probes, genomes, m, thres, island, ext, mode)
    elif thres == L and island == 0:
        for mode in (engine.SCAN_SEED, engine.SCAN_GENERAL):
            np.random.seed(seed)
            assert gp._scan_rows(ctx, probes, genomes, m, thres, island, ext, mode) == exp


# ------------------------------------------------------------------ 3. near-duplicate filters
MINHASH_LENGTHS = (138, 139, 200, 265)
MINHASH_SETTINGS = ((0.6, 10, 5), (0.35, 12, 6))          # (dist_thres, kmer_size, seed of `random`)
MINHASH_MAX_KMERS = 256                                    # MH_MAXK of csrc/ndf.hip


def _ndf_genomes():
    return _cached("ndf genomes", lambda: small_species(seed=91, n=8, length=4000, d1=0.02, d2=0.005))


def _ndf_strs(L, mixed=True, planted_n=False):
    """Candidates of L bases at stride L // 4, duplicates kept; mixed: and 100 of them cut to L - 60; planted_n: an N in
    every third string."""
    def make():
        strs = candidates(_ndf_genomes(), L, L // 4, dedup=False)
        if mixed:
            strs = strs + [s[:L - 60] for s in strs[:100]]
        if planted_n:
            strs = [s if i % 3 else s[:(7 * i) % len(s)] + "N" + s[(7 * i) % len(s) + 1:] for i, s in enumerate(strs)]
        return strs
    return _cached(("ndf strs", L, mixed, planted_n), make)


def test_minhash_cases_sit_on_their_branch_points():
    nks = {(L, ks): L - ks + 1 for L in MINHASH_LENGTHS for _, ks, _ in MINHASH_SETTINGS}
    assert sorted(nks.values()) == [127, 128, 129, 130, 189, 191, 254, 256]      # round the loop switch at 128, up to the limit
    assert max(nks.values()) == MINHASH_MAX_KMERS and 266 - 10 + 1 == MINHASH_MAX_KMERS + 1
    for L in MINHASH_LENGTHS + (266,):
        strs = _ndf_strs(L)
        assert sorted(set(map(len, strs))) == [L - 60, L] and len(set(strs)) < len(strs)
        assert 400 <= len(set(strs)) <= 900
    for L in (200, 265):
        strs = _ndf_strs(L, planted_n=True)
        with_n = [s for s in set(strs) if "N" in s]
        assert len(with_n) >= len(set(strs)) // 4 and sum(len(s) - 12 + 1 > 128 for s in with_n) >= 100
    for L in (200, 256):
        assert set(map(len, _ndf_strs(L, mixed=False))) == {L}


def _minhash_by_strings(ctx, oracle, strs, dist, ks, seed):
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    random.seed(seed)
    f = ndf.NearDuplicateFilterWithMinHash(dist, ks)
    params = f._draw_params()
    f._draw_params = lambda: params
    got = sorted(p.seq_str for p in f.filter([probe.Probe.from_str(s) for s in strs]))
    assert got == sorted(oracle.ndf_minhash(strs, dist, params, ks))
    assert len(got) < len(set(strs))


@pytest.mark.gpu
@pytest.mark.parametrize("dist,ks,seed", MINHASH_SETTINGS)
@pytest.mark.parametrize("L", MINHASH_LENGTHS)
def test_ndf_minhash_matches_oracle_at_127_to_256_kmers(ctx, oracle, L, dist, ks, seed):
    _minhash_by_strings(ctx, oracle, _ndf_strs(L), dist, ks, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("L,dist,ks,seed", [(265, 0.6, 10, 5), (200, 0.35, 12, 6)])
def test_ndf_minhash_with_n_above_128_kmers(ctx, oracle, L, dist, ks, seed):
    """A probe with an N has no 2-bit codes: its k-mers are ranked by their 128-bit byte strings, here over three
    and four register slots."""
    _minhash_by_strings(ctx, oracle, _ndf_strs(L, planted_n=True), dist, ks, seed)


@pytest.mark.gpu
def test_ndf_minhash_refuses_257_kmers(ctx):
    """266 bases hold 257 k-mers of 10: one more than a wavefront sorts and than the 8-bit slot of the sort key
    counts.  Refused for equal and for mixed lengths, and through the filter class; 256 k-mers of 11 pass."""
    from catch_amd.filter import near_duplicate_filter as ndf
    random.seed(5)
    f = ndf.NearDuplicateFilterWithMinHash(0.6, 10)
    params = f._draw_params()
    for mixed in (False, True):
        strs = _ndf_strs(266, mixed=mixed)[:300] + _ndf_strs(266, mixed=mixed)[-50:]
        with pytest.raises(ValueError, match="more than 256 k-mers per probe"):
            ctx.ndf_minhash(strs, 10, params, 0.6)
        with pytest.raises(ValueError, match="more than 256 k-mers per probe"):
            f._filter_strs(strs)
        assert len(ctx.ndf_minhash(strs, 11, params, 0.6)) == len(strs)


def _kept_on_device(ctx, genomes, L, stride, apply):
    engine = gp._engine()
    t = engine.Targets(ctx, genomes)
    c = engine.Candidates(ctx, t, L, stride)
    try:
        apply(c)
        flat = "".join(s for g in genomes for s in g)
        return [flat[p:p + L] for p in c.positions().tolist()]
    finally:
        c.close(); t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [200, 256])
def test_ndf_hamming_matches_oracle_at_long_probes(ctx, oracle, L):
    """The Hamming filter at 200 and 256 bases, on probe objects, on strings and on the device's candidates."""
    from catch_amd import probe
    from catch_amd.filter import near_duplicate_filter as ndf
    genomes, strs = _ndf_genomes(), _ndf_strs(L, mixed=False)
    random.seed(99)
    pos = oracle.lsh_draw_positions(oracle.lsh_num_tables(3, L, 20), 20, L)
    exp = oracle.ndf_hamming(strs, 3, pos)
    assert 0 < len(exp) < len(set(strs))
    f = ndf.NearDuplicateFilterWithHammingDistance(3, L)
    random.seed(99)
    assert [p.seq_str for p in f.filter([probe.Probe.from_str(s) for s in strs])] == exp
    random.seed(99)
    assert f._filter_strs(strs) == exp

    def apply(c):
        random.seed(99)
        f._apply_to_candidates(c)
    assert _kept_on_device(ctx, genomes, L, L // 4, apply) == exp


@pytest.mark.gpu
@pytest.mark.parametrize("dist,ks,seed", MINHASH_SETTINGS)
@pytest.mark.parametrize("L", [200, 256, 265])
def test_ndf_minhash_on_device_candidates_at_long_probes(ctx, oracle, L, dist, ks, seed):
    """The MinHash filter on the device's candidates (up to the 256 k-mers at which the front end still chooses it)
    keeps what the oracle keeps of the candidate strings, in the same order, and so does the string path."""
    from catch_amd.filter import near_duplicate_filter as ndf
    genomes, strs = _ndf_genomes(), _ndf_strs(L, mixed=False)
    random.seed(seed)
    params = oracle.minhash_draw_params(oracle.minhash_num_tables(dist), 3)
    exp = oracle.ndf_minhash(strs, dist, params, ks)
    assert 0 < len(exp) < len(set(strs))
    f = ndf.NearDuplicateFilterWithMinHash(dist, ks)
    random.seed(seed)
    assert f._filter_strs(strs) == exp

    def apply(c):
        random.seed(seed)
        f._apply_to_candidates(c)
    assert _kept_on_device(ctx, genomes, L, L // 4, apply) == exp


# ------------------------------------------------------------------ 6. end to end
def _design_both_front_ends(argv, tmp_path, monkeypatch, capsys):
    """design on the first ten Ebola genomes through the device and the host front end: the two outputs (checked
    identical), the count printed, and the anchor forms the device front end asked for."""
    from catch_amd.filter import set_cover_filter as scf
    kinds = []
    real = scf._anchors_for_candidates

    def spied(*a, **k):
        out = real(*a, **k)
        kinds.append(out[1])
        return out
    monkeypatch.setattr(scf, "_anchors_for_candidates", spied)
    outs, printed = {}, {}
    for front in ("device", "host"):
        if front == "host":
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        else:
            monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
        fn = tmp_path / (front + ".fasta")
        text = tdf._run_design([tdf.EBOLA, "--limit-target-genomes", "10"] + argv + ["-o", str(fn)], 5, capsys)
        outs[front] = fn.read_bytes()
        printed[front] = int(text.strip().splitlines()[-1])
        assert printed[front] == outs[front].count(b">") > 0
        if front == "device":
            device_kinds = list(kinds)
    assert kinds == device_kinds, "the host front end must not ask for the device front end's anchors"
    assert outs["device"] == outs["host"]
    return str(tmp_path / "device.fasta"), printed["device"], device_kinds


def _ebola_genomes():
    return _cached("ebola", lambda: [[s] for _, s in tdf._ebola_records(10)])


@pytest.mark.gpu
@pytest.mark.parametrize("argv,L,stride,m,thres,anchors", [
    (["-pl", "200", "-ps", "100"], 200, 100, 0, 200, "table"),
    (["-pl", "300", "-ps", "150", "-m", "3", "-l", "240"], 300, 150, 3, 240, "entries")],
    ids=["pl200", "pl300"])
def test_design_at_long_probes_equals_oracle_through_both_front_ends(ctx, oracle, tmp_path, monkeypatch, capsys,
                                                                     argv, L, stride, m, thres, anchors):
    """design at -pl 200 and at -pl 300 -m 3 -l 240 (random anchors of 20 over 281 positions: more than the device
    draws hold, so the front end hands over host-made entries): both front ends write the same file, and its probes
    are the oracle's selection from the same candidates."""
    from catch_amd.utils import seq_io
    out, printed, kinds = _design_both_front_ends(argv, tmp_path, monkeypatch, capsys)
    assert kinds and set(kinds) == {anchors}
    genomes = _ebola_genomes()
    cands = candidates(genomes, L, stride)
    np.random.seed(5)
    sel = oracle.set_cover_filter([cands], [genomes], m, thres, coverage=1.0, cover_extension=0)
    want = set(cands[j] for j in sel[0])
    got = set(seq_io.read_fasta(out).values())
    assert got == want and printed == len(want) > 20


@pytest.mark.gpu
def test_design_with_minhash_at_265_bases_equals_oracle_through_both_front_ends(ctx, oracle, tmp_path, monkeypatch, capsys):
    """--filter-with-lsh-minhash 0.6 at -pl 265: 256 k-mers of 10 per candidate, the most the filter takes and the
    last length at which the device front end runs it."""
    from catch_amd import engine
    from catch_amd.utils import seq_io
    calls = []
    for name in ("ndf_minhash", "ndf_minhash_many"):
        def counted(self, *a, _real=getattr(engine.Candidates, name), **k):
            calls.append(self.L)
            return _real(self, *a, **k)
        monkeypatch.setattr(engine.Candidates, name, counted)
    out, printed, _ = _design_both_front_ends(["-pl", "265", "-ps", "100", "--filter-with-lsh-minhash", "0.6"],
                                              tmp_path, monkeypatch, capsys)
    assert calls and set(calls) == {265}, "the device front end ran the filter"
    genomes = _ebola_genomes()
    strs = candidates(genomes, 265, 100, dedup=False)
    random.seed(5)
    params = oracle.minhash_draw_params(oracle.minhash_num_tables(0.6), 3)
    kept = oracle.ndf_minhash(strs, 0.6, params, 10)
    assert 0 < len(kept) < len(set(strs))
    sel = oracle.set_cover_filter([kept], [genomes], 0, 265, coverage=1.0, cover_extension=0)
    want = set(kept[j] for j in sel[0])
    got = set(seq_io.read_fasta(out).values())
    assert got == want and printed == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("front", ["default", "host"])
def test_design_with_minhash_at_266_bases_is_refused(ctx, tmp_path, monkeypatch, capsys, front):
    """One base more: 257 k-mers.  The device front end steps aside and the filter on the candidate strings refuses
    with the limit in its message -- never a probe set other than the reference's."""
    if front == "host":
        monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
    else:
        monkeypatch.delenv("CATCHHIP_HOST_FRONT_END", raising=False)
    fn = tmp_path / "out.fasta"
    with pytest.raises(ValueError, match="more than 256 k-mers per probe"):
        tdf._run_design([tdf.EBOLA, "--limit-target-genomes", "10", "-pl", "266", "-ps", "100",
                         "--filter-with-lsh-minhash", "0.6", "-o", str(fn)], 5, capsys)
    assert not fn.exists() or fn.read_bytes().count(b">") == 0
