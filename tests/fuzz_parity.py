"""Randomised differential test of the HIP path against the CPU oracle (GPU box).
    python tests/fuzz_parity.py [seconds] [seed]
Random groups of genomes (several chromosomes, N runs, repeats, short
sequences), random -pl/-ps/-m/-l/-e/-c/island/identify settings, with and
without duplicate candidates; compares the cover rows and the selected probe
sets, and the near-duplicate filters (MinHash k-mers of 6, 8, 10, 13 or 16).  Not part of the pytest suite: run by
hand after kernel changes; every failure prints the seed that reproduces it."""
import os
os.environ.setdefault("CATCHHIP_TEST_HOOKS", "1")
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import engine, genome, probe  # noqa: E402
from catch_amd.filter import candidate_probes, near_duplicate_filter  # noqa: E402
from catch_amd.filter.set_cover_filter import SetCoverFilter  # noqa: E402
from oracle import oracle  # noqa: E402


def rand_group(rnd):
    n_genomes = rnd.randrange(1, 9)
    root = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(300, 5000)))
    if rnd.random() < 0.3:   # a tandem repeat
        unit = root[:rnd.randrange(40, 200)]
        root += unit * rnd.randrange(2, 30)
    genomes = []
    for _ in range(n_genomes):
        s = list(root)
        for i in range(len(s)):
            if rnd.random() < rnd.choice([0.0, 0.01, 0.03]):
                s[i] = rnd.choice("ACGT")
        if rnd.random() < 0.4:
            i = rnd.randrange(len(s))
            s[i:i + rnd.randrange(1, 30)] = "N" * rnd.randrange(1, 30)
        s = "".join(s)
        if rnd.random() < 0.3:   # chromosomes
            c = sorted(rnd.sample(range(1, len(s)), min(3, len(s) - 1)))
            seqs = [s[a:b] for a, b in zip([0] + c, c + [len(s)])]
        else:
            seqs = [s]
        genomes.append(seqs)
    return genomes


SOLVER_ENV = ("CATCHHIP_FLAT_MIN_ROWS", "CATCHHIP_FLAT_STRIPED", "CATCHHIP_GF_LONG", "CATCHHIP_SEED_LIST",
              "CATCHHIP_FLAT_COUNT_ROUND0")


MINHASH_KMER_SIZES = (6, 8, 10, 13, 16)      # below and on a SipHash block, the compiled-in size, two id words, no 2-bit codes


def minhash_kmer_size(seed):
    """The k-mer size of a seed's MinHash filter: from a generator of its own, so that the sizes can change without
    moving any other draw of the seed."""
    return random.Random(seed * 7919 + 29).choice(MINHASH_KMER_SIZES)


def one_case(seed, ctx, kmer_size=None):
    """kmer_size: the MinHash filter's k-mer size instead of the seed's own (a pinned case keeps the size it was found
    with)."""
    rnd = random.Random(seed)
    # which of the equivalent kernel families run (all must give the oracle's result)
    for name in SOLVER_ENV:
        os.environ.pop(name, None)
    variant = random.Random(seed * 7919 + 13).choice(["default", "flat", "flat_striped", "flat_count0", "long", "seed_list"])
    if variant.startswith("flat"):
        os.environ["CATCHHIP_FLAT_MIN_ROWS"] = "0"
        if variant == "flat_striped":
            os.environ["CATCHHIP_FLAT_STRIPED"] = "1"
        if variant == "flat_count0":      # round 0's gains counted by a launch instead of taken from the row build
            os.environ["CATCHHIP_FLAT_COUNT_ROUND0"] = "1"
    elif variant == "long":
        os.environ["CATCHHIP_GF_LONG"] = "1"
    elif variant == "seed_list":
        os.environ["CATCHHIP_SEED_LIST"] = "1"      # the seed-list scan of rounds 1-3 instead of the key-grouped join
    L = rnd.choice([40, 60, 75, 100, 120])
    stride = rnd.choice([L // 4, L // 2, L])
    m = rnd.choice([0, 1, 2, 3, 5])
    thres = L if rnd.random() < 0.7 else rnd.randrange(L // 2, L)
    island = 0 if rnd.random() < 0.8 else rnd.randrange(5, 30)
    ext = rnd.choice([0, 0, 10, 50, 50, 120])
    coverage = rnd.choice([1.0, 1.0, 1.0, 0.9, 0.5])
    groups = [rand_group(rnd) for _ in range(rnd.randrange(1, 4))]
    cands = []
    for g in groups:
        seqs = [s for gen in g for s in gen if len(s) >= L]
        if not seqs:
            seqs = ["".join(rnd.choice("ACGT") for _ in range(L + 10))]
            g.append(seqs)
        c = candidate_probes.candidate_strings_from_sequences(seqs, L, stride)
        if rnd.random() < 0.7:
            c = list(dict.fromkeys(c))
        cands.append(c)
    np_seed = rnd.randrange(1 << 30)
    desc = dict(seed=seed, variant=variant, L=L, stride=stride, m=m, thres=thres, island=island, ext=ext,
                coverage=coverage, groups=[(len(g), sum(len(s) for gen in g for s in gen)) for g in groups])
    np.random.seed(np_seed)
    want = oracle.set_cover_filter(cands, groups, m, thres, island=island, coverage=coverage,
                                   cover_extension=ext)
    np.random.seed(np_seed)
    f = SetCoverFilter(mismatches=m, lcf_thres=thres, island_of_exact_match=island,
                       coverage=coverage, cover_extension=ext)
    def mk(gen):
        if len(gen) == 1:
            return genome.Genome.from_one_seq(gen[0])
        return genome.Genome.from_chrs(dict(("c%d" % i, x) for i, x in enumerate(gen)))
    got = f._filter_strs(cands, [[mk(gen) for gen in g] for g in groups])
    assert [sorted(a) for a in got] == [sorted(b) for b in want], desc
    if not cands[0]:
        # (seed 1200792: the first group's only sequence of probe length or more is cut by a run of N's into pieces shorter
        # than a probe -- catch/filter/candidate_probes.py makes no candidate then; the filters above agreed on the empty
        # selection, and the checks below need a first group with candidates)
        return
    # rows of the first group through every scan mode that applies
    np.random.seed(np_seed)
    k, entries = oracle.anchor_table(cands[0], m, thres)
    uniq, owner = oracle._unique_last(cands[0])
    pr, un, st, en = oracle.make_sets(uniq, entries, k, groups[0], m, thres, island, ext)
    own = np.array(owner, dtype=np.int32)
    exp = sorted(zip((own[pr] if pr.size else pr).tolist(), un.tolist(), st.tolist(), en.tolist()))
    for mode in (engine.SCAN_AUTO, engine.SCAN_GENERAL):
        np.random.seed(np_seed)
        kk, uq, ow, ep, eo = probe.anchor_table(cands[0], m, thres)
        t = engine.Targets(ctx, groups[0])
        p = engine.Probes(ctx, uq, ow, ep, eo, kk)
        rows = engine.Rows.scan(ctx, p, t, m, thres, island, ext, mode)
        a = rows.fetch()
        got_rows = sorted(zip(a[0].tolist(), a[1].tolist(), a[2].tolist(), a[3].tolist()))
        rows.close(); p.close(); t.close()
        assert got_rows == exp, (desc, mode)
    # the first group with its universes sharded 2 and 3 ways (full coverage, short rows)
    from catch_amd import parallel
    np.random.seed(np_seed)
    kk, uq, ow, ep, eo = probe.anchor_table(cands[0], m, thres)
    if thres == L and island == 0 and L + 2 * ext <= 250 and len(groups[0]) >= 2:
        p = engine.Probes(ctx, uq, ow, ep, eo, kk)
        t = engine.Targets(ctx, groups[0])
        rows = engine.Rows.scan(ctx, p, t, m, thres, island, ext)
        a = rows.fetch()
        ok_len = a[0].size == 0 or int((a[3] - a[2]).max()) <= 257
        whole = rows.greedy(len(cands[0]))
        # ... and under partial coverage, fractions per universe
        up = None
        if ok_len:
            up = [rnd.choice([1.0, 0.9, 0.5, 0.25]) for _ in groups[0]]
            if all(x >= 1.0 for x in up):
                up[0] = 0.8
            whole_p = rows.greedy(len(cands[0]), None, up)
        rows.close(); t.close()
        if ok_len:
            lens = [sum(len(x) for x in gen) for gen in groups[0]]
            for world in (2, 3):
                b = parallel.split_universes(lens, world)
                for fractions, expect in ((None, whole), (up, whole_p if up else None)):
                    if fractions is None and expect is None:
                        continue
                    if fractions is None and expect is not whole:
                        continue
                    held, shards = [], []
                    for v in range(world):
                        tv = engine.Targets(ctx, groups[0][b[v]:b[v + 1]])
                        rv = engine.Rows.scan(ctx, p, tv, m, thres, island, ext)
                        held += [tv, rv]
                        # (instance_partial: the same on every shard -- one with fractions of 1.0 only builds the
                        # partial kind too, as SetCoverFilter does; catchhip_shard_solve insists on it)
                        shards.append(engine.Shard(rv, len(cands[0]), None,
                                                   None if fractions is None else fractions[b[v]:b[v + 1]],
                                                   instance_partial=fractions is not None))
                    # the interpreter's round loop, or the loop under the C ABI with 1-5 rounds per read-back (round 6)
                    rps = rnd.choice([0, 1, 2, 3, 5])
                    if rps == 0:
                        got_s = parallel.sharded_solve(shards, lambda w: engine.shards_allreduce_local(shards, w))
                    else:
                        got_s = engine.shards_solve(shards, "local", rps)
                    for h in shards + held[::-1]:
                        h.close()
                    assert got_s == expect, (desc, "sharded", world, fractions, "rounds per sync", rps)
        p.close()
    # near-duplicate filters on the first group's candidates (equal lengths)
    strs = [s for s in cands[0] if len(s) == L][:1500]
    if len(strs) > 3:
        d = rnd.choice([1, 2, 3])
        random.seed(seed)
        fh = near_duplicate_filter.NearDuplicateFilterWithHammingDistance(d, L)
        pos = fh._draw_positions()
        fh._draw_positions = lambda: pos
        gh = sorted(p.seq_str for p in fh.filter([probe.Probe.from_str(s) for s in strs]))
        assert gh == sorted(oracle.ndf_hamming(strs, d, pos)), (desc, "ndf hamming")
        dj = rnd.choice([0.3, 0.5, 0.6])
        drawn = rnd.choice([8, 10])      # (the sizes of rounds 1-6; still drawn: the later draws of a seed stay what they were)
        ks = kmer_size or minhash_kmer_size(seed)
        desc.update(minhash_kmer_size=ks, minhash_kmer_size_of_rounds_1_to_6=drawn)
        fm = near_duplicate_filter.NearDuplicateFilterWithMinHash(dj, ks)
        par = fm._draw_params()
        fm._draw_params = lambda: par
        gm = sorted(p.seq_str for p in fm.filter([probe.Probe.from_str(s) for s in strs]))
        assert gm == sorted(oracle.ndf_minhash(strs, dj, par, fm.kmer_size)), (desc, "ndf minhash")
    # adapter filter on a subsample of the first group's candidates, votes from
    # all sequences of all groups (this interpreter's string hash on both sides)
    from catch_amd.filter.adapter_filter import AdapterFilter
    sub = cands[0][::max(1, len(cands[0]) // 400)]
    if len(set(map(len, sub))) >= 1 and sub:
        kmap = rnd.choice([10, 15, 20])
        if min(map(len, sub)) >= kmap:
            all_seqs = [s for g in groups for gen in g for s in gen]
            np.random.seed(np_seed)
            want_a = oracle.adapter_filter(sub, all_seqs, ("AA", "CC"), ("GG", "TT"), m, thres, island, kmap,
                                           hash_fn=hash)
            np.random.seed(np_seed)
            fa = AdapterFilter(("AA", "CC"), ("GG", "TT"), m, thres, island_of_exact_match=island,
                               kmer_probe_map_k=kmap)
            got_a = fa.filter([probe.Probe.from_str(s) for s in sub],
                              [[mk(gen) for gen in g] for g in groups])
            assert [p.seq_str for p in got_a] == want_a, (desc, "adapter filter", kmap)
    # whole designs: front end on the device (per group or as one grouped
    # instance) against the host front end, same random streams
    from catch_amd.filter import duplicate_filter, probe_designer
    kind = rnd.choice(["dup", "hamming", "minhash"])
    hd = rnd.choice([1, 2])
    gens = [[mk(gen) for gen in g] for g in groups]
    if rnd.random() < 0.5:          # many small groups
        gens = [[x] for grp in gens for x in grp] * 2
        gens = gens[:max(8, len(gens))]
    outs = []
    for host in (False, True):
        if host:
            os.environ["CATCHHIP_HOST_FRONT_END"] = "1"
        else:
            os.environ.pop("CATCHHIP_HOST_FRONT_END", None)
        first = (duplicate_filter.DuplicateFilter() if kind == "dup" else
                 near_duplicate_filter.NearDuplicateFilterWithHammingDistance(hd, L)
                 if kind == "hamming" else near_duplicate_filter.NearDuplicateFilterWithMinHash(0.5))
        fs = SetCoverFilter(mismatches=m, lcf_thres=thres, island_of_exact_match=island,
                            coverage=coverage, cover_extension=ext)
        pd = probe_designer.ProbeDesigner(gens, [first, fs], probe_length=L, probe_stride=stride,
                                          seq_length_to_skip=L - 1)
        random.seed(seed)
        np.random.seed(np_seed)
        outs.append([[p.seq_str for p in g] for g in pd._design_on_strings(gens, [first, fs])])
    os.environ.pop("CATCHHIP_HOST_FRONT_END", None)
    rnd.random()   # keep the stream position independent of the branch above
    assert outs[0] == outs[1], (desc, "front end", kind, len(gens))
    # clustering of all sequences (whole and fragmented), both methods
    from catch_amd.utils import cluster
    all_seqs = [s for g in groups for gen in g for s in gen if len(s) >= 12]
    if rnd.random() < 0.5:
        fl = rnd.choice([200, 500, 1000])
        all_seqs = [f for s in all_seqs for f in oracle.fragments_of(s, fl) if len(f) >= 12]
    if all_seqs:
        thr = rnd.choice([0.05, 0.1, 0.15, 0.3])
        for method in ("simple", "hierarchical"):
            if method == "hierarchical" and len(all_seqs) > 300:
                continue
            random.seed(seed)
            want_c = oracle.cluster_with_minhash_signatures(all_seqs, threshold=thr, cluster_method=method)
            random.seed(seed)
            got_c = cluster.cluster_with_minhash_signatures(dict(enumerate(all_seqs)), threshold=thr,
                                                            cluster_method=method)
            assert got_c == want_c, (desc, "cluster", method, thr)
    return desc


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ctx = engine.default_context()
    t0 = time.time()
    n = 0
    while time.time() - t0 < budget:
        try:
            one_case(seed0 + n, ctx)
        except BaseException:
            print("fuzz: FAILED at seed %d (python tests/fuzz_parity.py 1 %d reproduces it)" % (seed0 + n, seed0 + n), flush=True)
            raise
        n += 1
    print("fuzz: %d cases ok (seeds %d..%d) in %.0f s" % (n, seed0, seed0 + n - 1, time.time() - t0))


if __name__ == "__main__":
    main()
