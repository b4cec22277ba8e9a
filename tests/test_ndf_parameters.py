"""The near-duplicate filters of csrc/ndf.hip over their whole parameter domain, against the CPU oracle.

The rest of the suite compares the filters' resolution forms with each other on large inputs and visits a few
parameter points against the oracle (k-mers of 10 and 12, three functions per table, 1-25 tables, up to four Hamming
tables).  Here every k-mer size 1-16, 1-16 functions per table, 1-65 tables, pairs exactly on and just beyond the
Jaccard threshold, Hamming lengths round every multiple of 8, thresholds 0-L, 1-L sampled positions and 1-8 tables
go against the oracle, all bit-exact, on inputs of at most 700 probes.  Section 0 pins the oracle's own string hash
to SipHash-2-4 written out in plain Python, so that oracle and kernel cannot share a mistake at some length.  The
tests without the gpu mark check, with the oracle alone, that the inputs sit on the branch points they are there for.
"""
import random
import subprocess
import sys

import numpy as np
import pytest

import test_probe_lengths as tpl

_CACHE = {}
P31 = 2 ** 31 - 1
NDF_OWN_STEPS = 8                    # of csrc/ndf.hip: steps a lane walks alone before the wavefront shares its walk
WAVE = 64
MAX_PROBES = 700


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------ 0. the oracle's hash
_M64 = (1 << 64) - 1


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & _M64


def _siphash24(data, k0=0, k1=0):
    """SipHash-2-4 (Aumasson & Bernstein 2012) of `data` under the key (k0, k1), as an unsigned 64-bit int:
    little-endian blocks of 8 bytes, the last one holding the rest and the length (mod 256) in its top byte."""
    v0, v1 = k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d
    v2, v3 = k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573

    def rounds(n, v0, v1, v2, v3):
        for _ in range(n):
            v0 = (v0 + v1) & _M64; v1 = _rotl(v1, 13); v1 ^= v0; v0 = _rotl(v0, 32)
            v2 = (v2 + v3) & _M64; v3 = _rotl(v3, 16); v3 ^= v2
            v0 = (v0 + v3) & _M64; v3 = _rotl(v3, 21); v3 ^= v0
            v2 = (v2 + v1) & _M64; v1 = _rotl(v1, 17); v1 ^= v2; v2 = _rotl(v2, 32)
        return v0, v1, v2, v3
    whole = len(data) - len(data) % 8
    blocks = [int.from_bytes(data[i:i + 8], "little") for i in range(0, whole, 8)]
    blocks.append(int.from_bytes(data[whole:], "little") | (len(data) & 0xff) << 56)
    for m in blocks:
        v3 ^= m
        v0, v1, v2, v3 = rounds(2, v0, v1, v2, v3)
        v0 ^= m
    v2 ^= 0xff
    v0, v1, v2, v3 = rounds(4, v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def _pyhash_seed0(s):
    """hash(s) of CPython 3.4-3.10 under PYTHONHASHSEED=0 for an ASCII str: the empty string hashes to 0 before any
    algorithm runs (Python/pyhash.c), anything else is SipHash-2-4 of its bytes under the key (0, 0), read as a
    signed 64-bit number, -1 -> -2."""
    if not s:
        return 0
    x = _siphash24(s.encode("ascii"))
    x = x - (1 << 64) if x >> 63 else x
    return -2 if x == -1 else x


HASH_LENGTHS = tuple(range(25)) + (63,)


def _hash_strings():
    rng = random.Random(11)
    out = []
    for n in HASH_LENGTHS:
        out.append("".join(rng.choice("ACGT") for _ in range(n)))
        out.append("".join(rng.choice("ACGTNacgtn") for _ in range(n)))
        out.append(("N" * n, "acgtn" * 13)[n % 2][:n])
    return out


def test_siphash_restatement_matches_the_published_vectors():
    """The paper's worked example (key 00 .. 0f, input 00 .. 0e) and entries of the reference implementation's vector
    table, whose inputs are 00, 01, ... of 0, 1, 7 and 8 bytes: no block, a tail only, a full tail, one block."""
    k0, k1 = 0x0706050403020100, 0x0f0e0d0c0b0a0908
    vectors = {0: 0x726fdb47dd0e0e31, 1: 0x74f839c593dc67fd, 7: 0xab0200f58b01d137, 8: 0x93f5f5799a932462,
               15: 0xa129ca6149be45e5}
    for n, want in vectors.items():
        assert _siphash24(bytes(range(n)), k0, k1) == want, n


def test_oracle_pyhash_is_siphash24_at_every_block_count(oracle):
    """oracle.pyhash_seed0 against the plain-Python SipHash-2-4 at every length 0-24 (no block, one, two, three, with
    every tail length) and at 63, on A/C/G/T strings and on strings with N and lower case.  Whatever the interpreter:
    nothing here calls hash().  The k-mers the MinHash oracle hashes are 1-16 characters long."""
    strs = _hash_strings()
    assert sorted(set(map(len, strs))) == list(HASH_LENGTHS) and len(strs) == 3 * len(HASH_LENGTHS)
    assert {len(s) // 8 for s in strs} >= {0, 1, 2, 3, 7} and {len(s) % 8 for s in strs} == set(range(8))
    for s in strs:
        assert oracle.pyhash_seed0(s) == _pyhash_seed0(s), (len(s), s)
    assert len({_pyhash_seed0(s) for s in set(strs)}) == len(set(strs))


def test_oracle_pyhash_is_this_interpreters_hash(oracle):
    """Where the interpreter itself still hashes str with SipHash-2-4 (CPython <= 3.10), hash() of a child process
    under PYTHONHASHSEED=0 says the same as both restatements, at the same lengths."""
    if sys.version_info >= (3, 11) or sys.hash_info.algorithm != "siphash24":
        pytest.skip("this interpreter hashes str with " + sys.hash_info.algorithm)
    strs = _hash_strings()
    out = subprocess.run([sys.executable, "-c", "print([hash(x) for x in %r])" % (strs,)],
                         env={"PYTHONHASHSEED": "0", "PATH": "/usr/bin:/bin"},
                         capture_output=True, text=True, check=True).stdout
    got = eval(out)
    assert got == [_pyhash_seed0(s) for s in strs]
    assert got == [oracle.pyhash_seed0(s) for s in strs]


# ------------------------------------------------------------------ inputs
def _rand_str(rng, L, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(L))


def _family_strs(L, seed, max_subs=4, sub_alphabet="ACGT"):
    """6 random roots with 80 variants each of 0..max_subs substitutions, 100 unrelated strings and three strings of
    low complexity, all of L characters, unique, in this order (= the filters' priority order)."""
    def make():
        rng = random.Random(seed)
        out = []
        for _ in range(6):
            root = _rand_str(rng, L)
            for _ in range(80):
                s = list(root)
                for _ in range(rng.randint(0, max_subs)):
                    s[rng.randrange(L)] = rng.choice(sub_alphabet)
                out.append("".join(s))
        out += [_rand_str(rng, L) for _ in range(100)]
        out += ["A" * L, ("AC" * L)[:L], ("ACG" * L)[:L]]
        out = list(dict.fromkeys(out))
        assert len(out) <= MAX_PROBES
        return out
    return _cached(("family", L, seed, max_subs, sub_alphabet), make)


def _plant_n(strs):
    """An N in every third string."""
    out = [s if i % 3 else s[:(7 * i) % len(s)] + "N" + s[(7 * i) % len(s) + 1:] for i, s in enumerate(strs)]
    return list(dict.fromkeys(out))


def _draw_params(oracle, ntables, k, seed):
    state = random.getstate()
    random.seed(seed)
    try:
        return oracle.minhash_draw_params(ntables, k)
    finally:
        random.setstate(state)


def _draw_positions(oracle, ntables, k, L, seed):
    state = random.getstate()
    random.seed(seed)
    try:
        return oracle.lsh_draw_positions(ntables, k, L)
    finally:
        random.setstate(state)


def _kmers(s, ks):
    return {s[i:i + ks] for i in range(len(s) - ks + 1)}


def _minhash_keys(oracle, strs, params, ks):
    """keys[table][probe]: the oracle's table keys (tuples of the k minima)."""
    lib = oracle.lib()
    keys = [[None] * len(strs) for _ in params]
    for i, s in enumerate(strs):
        buf = oracle._bytes_arr(s)
        ptr = oracle._p(buf, oracle._u8p)
        for t, fns in enumerate(params):
            keys[t][i] = tuple(int(lib.orc_minhash(ptr, len(s), ks, a, b)) for a, b in fns)
    return keys


def _hamming_keys(strs, positions):
    return [[tuple(s[j] for j in pos) for s in strs] for pos in positions]


def _largest_bucket(keys):
    best = 0
    for row in keys:
        count = {}
        for key in row:
            count[key] = count.get(key, 0) + 1
        best = max(best, max(count.values()))
    return best


def _buckets(row):
    out = {}
    for i, key in enumerate(row):
        out.setdefault(key, []).append(i)
    return [b for b in out.values() if len(b) > 1]


def _need(S, thres):
    """The smallest intersection m of two k-mer sets of S = |A| + |B| members with 1 - m / (S - m) <= thres."""
    for m in range(S // 2 + 1):
        if 1.0 - float(m) / (S - m) <= thres:
            return m
    return S // 2 + 1


# ------------------------------------------------------------------ MinHash cases
KMER_SIZES = tuple(range(1, 17))
KMER_SIZES_MORE = (7, 8, 9, 15, 16)          # round the id words' split at 8 / 9 and the packable limit at 15 / 16
MIXED_LENGTH_KMER_SIZES = (8, 16)
FUNCTION_COUNTS = (1, 2, 3, 4, 5, 6, 7, 16)
TABLE_COUNTS = (1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65)
SECTION2_KMER_SIZES = (10, 12)
MH_FORMS = (None, "CATCHHIP_MH_ALL_PAIRS", "CATCHHIP_MH_NO_WAVE64")


def _mh_case(oracle, key, strs, ks, params, dist):
    def make():
        assert len(strs) == len(set(strs)) <= MAX_PROBES
        keys = _minhash_keys(oracle, strs, params, ks)
        return dict(strs=strs, ks=ks, params=params, dist=dist, keys=keys, largest=_largest_bucket(keys),
                    kept=oracle.ndf_minhash(strs, dist, params, ks, inclusion_order=True))
    return _cached(key, make)


def _kmer_length(ks):
    """100 characters hold every 1-, 2- and 3-mer: all probes alike.  Short probes for the short k-mers."""
    return 100 if ks >= 4 else 4 * ks + 4


def _kmer_case(oracle, ks, planted_n=False):
    strs = _family_strs(_kmer_length(ks), 100 + ks)
    if planted_n:
        strs = _cached(("planted", ks), lambda: _plant_n(strs))
    return _mh_case(oracle, ("kmer", ks, planted_n), strs, ks, _draw_params(oracle, 13, 3, 7), 0.5)


def _kmer_groups_case(oracle, ks):
    def make():
        strs = _family_strs(_kmer_length(ks), 100 + ks)
        groups = [strs[g::3] for g in range(3)]
        params = [_draw_params(oracle, 13, 3, 20 + g) for g in range(3)]
        kept = [oracle.ndf_minhash(g, 0.5, p, ks, inclusion_order=True) for g, p in zip(groups, params)]
        return dict(groups=groups, params=params, kept=kept)
    return _cached(("kmer groups", ks), make)


def _mixed_length_case(oracle, ks):
    """Every length from one k-mer to 256 k-mers, cut from two roots (prefixes of both, suffixes of one) so that short
    and long probes share minima, next to unrelated strings; shuffled."""
    def make():
        rng = random.Random(300 + ks)
        roots = [_rand_str(rng, ks + 255) for _ in range(2)]
        strs = [r[:n] for n in range(ks, ks + 256) for r in roots]
        strs += [roots[0][-n:] for n in range(ks, ks + 256, 4)]
        strs += [_rand_str(rng, rng.randrange(ks, ks + 256)) for _ in range(60)]
        strs = list(dict.fromkeys(strs))
        rng.shuffle(strs)
        return strs
    strs = _cached(("mixed strs", ks), make)
    return _mh_case(oracle, ("mixed", ks), strs, ks, _draw_params(oracle, 13, 3, 8), 0.5)


def _functions_case(oracle, ks, k):
    """k = 16: two probes share a bucket only when 16 minima agree -- near-identical variants (0..1 substitutions)."""
    strs = _family_strs(100, 100 + ks, max_subs=1 if k == 16 else 4)
    return _mh_case(oracle, ("functions", ks, k), strs, ks, _draw_params(oracle, 4, k, 40 + k), 0.5)


def _tables_case(oracle, ks, ntables):
    return _mh_case(oracle, ("tables", ks, ntables), _family_strs(100, 100 + ks), ks,
                    _draw_params(oracle, ntables, 3, 60 + ntables), 0.5)


def _extreme_params(oracle):
    """Four tables; in the second every a is 2^31 - 1 (= 0 mod p: every k-mer hashes to b, all probes in one bucket),
    in the third every b is 2^31 - 1: both ends of the reference's randint."""
    params = [list(t) for t in _draw_params(oracle, 4, 3, 77)]
    params[1] = [(P31, b) for _, b in params[1]]
    params[2] = [(a, P31) for a, _ in params[2]]
    return params


def _extreme_case(oracle, ks, dist):
    return _mh_case(oracle, ("extreme", ks, dist), _family_strs(100, 100 + ks), ks, _extreme_params(oracle), dist)


# pairs on the threshold: (dist_thres, tables, shared k-mers m, near?) at 99 characters, k-mers of 10: 90 k-mers each
PAIR_L, PAIR_KS = 99, 10
THRESHOLD_CLASSES = [
    (0.5, 13, 60, True),             # 1 - 60 / 120 = 0.5
    (0.5, 13, 59, False),            # 1 - 59 / 121 = 0.5124
    (0.6, 25, 52, True),             # 1 - 52 / 128 = 0.59375
    (0.6, 25, 51, False),            # 1 - 51 / 129 = 0.6047
]
PAIR_FORMS = ("pairs", "family", "with_n")
NPAIRS, NFAMILIES, NVARIANTS = 150, 3, 200


def _threshold_pair(rng, m, n_in=0):
    """(P + X, P + Y): a common prefix of m + 9 characters, random tails, both with 90 distinct k-mers and exactly m in
    common.  n_in: an N in X (1) or in both tails (2)."""
    full = PAIR_L - PAIR_KS + 1
    while True:
        prefix = _rand_str(rng, m + PAIR_KS - 1)
        x, y = (list(_rand_str(rng, PAIR_L - len(prefix))) for _ in range(2))
        if n_in >= 1:
            x[rng.randrange(1, len(x))] = "N"
        if n_in >= 2:
            y[rng.randrange(1, len(y))] = "N"
        a, b = prefix + "".join(x), prefix + "".join(y)
        ka, kb = _kmers(a, PAIR_KS), _kmers(b, PAIR_KS)
        if len(ka) == len(kb) == full and len(ka & kb) == m:
            return a, b


def _pair_strs(m, form):
    """pairs / with_n: 150 pairs, mates adjacent.  family: three times P + Y, P + X and 200 variants of P + X with 1-3
    substitutions in X only -- each variant shares the prefix's m k-mers with P + Y and no other, and walks a run of
    up to 201 higher-priority mates."""
    def make():
        rng = random.Random(500 + m + 1000 * PAIR_FORMS.index(form))
        strs = []
        if form == "family":
            for _ in range(NFAMILIES):
                a, b = _threshold_pair(rng, m)
                strs += [b, a]
                for _ in range(NVARIANTS):
                    s = list(a)
                    for _ in range(rng.randint(1, 3)):
                        s[rng.randrange(m + PAIR_KS - 1, PAIR_L)] = rng.choice("ACGT")
                    strs.append("".join(s))
        else:
            for i in range(NPAIRS):
                strs += _threshold_pair(rng, m, (1 + i % 2) if form == "with_n" else 0)
        return list(dict.fromkeys(strs))
    return _cached(("pair strs", m, form), make)


def _pair_case(oracle, dist, ntables, m, form):
    return _mh_case(oracle, ("pair", dist, ntables, m, form), _pair_strs(m, form), PAIR_KS,
                    _draw_params(oracle, ntables, 3, 90 + ntables), dist)


def _pairs_on_threshold(c, m):
    """(i, j), i < j, of a case: both with 90 distinct k-mers, exactly m in common and a bucket in common."""
    strs, keys = c["strs"], c["keys"]
    sets = [_kmers(s, PAIR_KS) for s in strs]
    full = PAIR_L - PAIR_KS + 1
    out = set()
    for row in keys:
        for b in _buckets(row):
            for x, i in enumerate(b):
                for j in b[x + 1:]:
                    if (i, j) not in out and len(sets[i]) == len(sets[j]) == full and len(sets[i] & sets[j]) == m:
                        out.add((i, j))
    return out


def _equal_set_strs():
    """Different strings with equal k-mer sets (distance 0.0): the two phases of a dinucleotide repeat at k-mers of 2,
    the twelve rotations of a repeat with a unit of 12 at k-mers of 8 (windows of 60 hold all twelve k-mers); next to
    each a string with one more k-mer, and unrelated ones."""
    rng = random.Random(71)
    two = ["AC" * 10, "CA" * 10, "AC" * 9 + "AA", "ACCA" * 5, "GT" * 10, "TG" * 10] + [_rand_str(rng, 20) for _ in range(20)]
    unit = "ACGGTCATTGCA"
    eight = [(unit * 7)[r:r + 60] for r in range(12)] + [(unit * 7)[:59] + "T"] + [_rand_str(rng, 60) for _ in range(20)]
    assert len(_kmers(unit * 3, 8)) == 12
    return {2: list(dict.fromkeys(two)), 8: eight}


def _equal_set_case(oracle, ks):
    return _mh_case(oracle, ("equal sets", ks), _equal_set_strs()[ks], ks, _draw_params(oracle, 1, 3, 72), 0.0)


def _all_minhash_cases(oracle):
    """(name, case, facts claimed of it): "own" -- a bucket longer than a lane's own steps, "wave" -- longer than a
    wavefront, "both" -- the oracle keeps some probes and drops some."""
    for ks in KMER_SIZES:
        yield ("kmer", ks), _kmer_case(oracle, ks), {"own", "both"}
    for ks in KMER_SIZES_MORE:
        yield ("kmer with N", ks), _kmer_case(oracle, ks, planted_n=True), {"own", "both"}
    for ks in MIXED_LENGTH_KMER_SIZES:
        yield ("mixed lengths", ks), _mixed_length_case(oracle, ks), {"own", "both"}
    for ks in SECTION2_KMER_SIZES:
        for k in FUNCTION_COUNTS:
            # (sixteen minima agree for a handful of near-identical probes only: the pairs are counted instead)
            yield ("functions", ks, k), _functions_case(oracle, ks, k), {"both"} | ({"own"} if k <= 7 else set())
        for nt in TABLE_COUNTS:
            yield ("tables", ks, nt), _tables_case(oracle, ks, nt), {"own", "both"}
        yield ("extreme", ks, 0.5), _extreme_case(oracle, ks, 0.5), {"own", "wave", "both"}
    for dist, nt, m, near in THRESHOLD_CLASSES:
        # (separate pairs make buckets of two; a class that is not near drops nothing among separate pairs)
        yield ("pairs", dist, m), _pair_case(oracle, dist, nt, m, "pairs"), {"both"} if near else set()
        yield ("family", dist, m), _pair_case(oracle, dist, nt, m, "family"), {"own", "wave", "both"}
        yield ("with_n", dist, m), _pair_case(oracle, dist, nt, m, "with_n"), {"both"} if near else set()


# ------------------------------------------------------------------ Hamming cases
HAMMING_LENGTHS = (5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 101)
HAMMING_DEVICE_LENGTHS = (9, 64, 101)
HAMMING_THRESHOLDS = (0, 1, 99, 100)
HAMMING_SAMPLED = (1, 2, 50, 100)
HAMMING_TABLES = (1, 2, 3, 4, 5, 8)
HAMMING_DEDUPE_FROM = 4                      # HammingFamily::dedupe of csrc/ndf.hip
REPEATED_POSITIONS = [[5, 5, 17], [0, 99, 0], [42, 42, 42]]


def _hamming_case(oracle, key, strs, positions, dist):
    def make():
        assert len(strs) == len(set(strs)) <= MAX_PROBES and len(set(map(len, strs))) == 1
        kept = oracle.ndf_hamming(strs, dist, positions, inclusion_order=True)
        keys = _hamming_keys(strs, positions)
        return dict(strs=strs, L=len(strs[0]), positions=positions, dist=dist, kept=kept, keys=keys,
                    largest=_largest_bucket(keys), as_set=oracle.as_list_of_set(kept))
    return _cached(key, make)


def _hamming_length_case(oracle, L):
    return _hamming_case(oracle, ("hamming length", L), _family_strs(L, 200 + L),
                         _draw_positions(oracle, 3, min(3, L), L, 30 + L), 2)


def _hamming_threshold_case(oracle, dist):
    return _hamming_case(oracle, ("hamming threshold", dist), _family_strs(100, 300),
                         _draw_positions(oracle, 3, 3, 100, 31), dist)


def _hamming_sampled_case(oracle, k):
    positions = REPEATED_POSITIONS if k == "repeated" else _draw_positions(oracle, 3, k, 100, 32 + k)
    return _hamming_case(oracle, ("hamming sampled", k), _family_strs(100, 300), positions, 2)


def _hamming_tables_case(oracle, ntables):
    return _hamming_case(oracle, ("hamming tables", ntables), _family_strs(100, 300),
                         _draw_positions(oracle, ntables, 20, 100, 33), 6)


def _hamming_bytes_case(oracle):
    return _hamming_case(oracle, "hamming bytes", _family_strs(100, 301, sub_alphabet="ACGTNNacgt"),
                         _draw_positions(oracle, 3, 3, 100, 34), 2)


def _hamming_groups_case(oracle):
    def make():
        groups = [_family_strs(100, 310 + g) for g in range(3)]
        positions = [_draw_positions(oracle, 4, 20, 100, 35 + g) for g in range(3)]
        kept = [oracle.ndf_hamming(g, 3, p, inclusion_order=True) for g, p in zip(groups, positions)]
        return dict(groups=groups, positions=positions, kept=kept)
    return _cached("hamming groups", make)


def _all_hamming_cases(oracle):
    for L in HAMMING_LENGTHS:
        yield ("length", L), _hamming_length_case(oracle, L), {"own", "both"}
    for d in HAMMING_THRESHOLDS:
        yield ("threshold", d), _hamming_threshold_case(oracle, d), {"own", "both"} if d else {"own"}
    for k in HAMMING_SAMPLED + ("repeated",):
        # (50 and 100 sampled positions: only near-identical probes share a key)
        yield ("sampled", k), _hamming_sampled_case(oracle, k), {"both"} | (set() if k in (50, 100) else {"own"})
    for nt in HAMMING_TABLES:
        yield ("tables", nt), _hamming_tables_case(oracle, nt), {"own", "both"}
    yield ("bytes",), _hamming_bytes_case(oracle), {"own", "both"}


def _bucket_pairs(keys):
    """Per table, the pairs (i, j), i < j, that share a bucket."""
    return [{(i, j) for b in _buckets(row) for x, i in enumerate(b) for j in b[x + 1:]} for row in keys]


def _comparisons_expected(c):
    """Pairs compared when no walk ends early: from four tables on a pair belongs to the first table it meets in, with
    fewer it is compared in every table it meets in (HammingFamily::dedupe and the edge kernel's n_earlier)."""
    per_table = _bucket_pairs(c["keys"])
    once, every = len(set().union(*per_table)), sum(map(len, per_table))
    return once if len(c["keys"]) >= HAMMING_DEDUPE_FROM else every


def _pairs_meeting_again(c):
    """Pairs within the threshold that share a bucket in some table and in an earlier one as well."""
    strs, seen, again = c["strs"], set(), set()
    arr = [np.frombuffer(s.encode("latin-1"), dtype=np.uint8) for s in strs]
    for row in c["keys"]:
        here = set()
        for b in _buckets(row):
            for x, i in enumerate(b):
                for j in b[x + 1:]:
                    if int(np.count_nonzero(arr[i] != arr[j])) <= c["dist"]:
                        here.add((i, j))
        again |= here & seen
        seen |= here
    return again


# ------------------------------------------------------------------ 5. no GPU: the inputs sit where they are claimed to
def test_parameter_tables_include_both_sides_of_every_switch():
    assert {7, 8, 9} <= set(KMER_SIZES) and {9, 10, 11} <= set(KMER_SIZES) and {15, 16} <= set(KMER_SIZES)
    assert min(KMER_SIZES) == 1 and max(KMER_SIZES) == 16 and {7, 8, 9, 15, 16} == set(KMER_SIZES_MORE)
    for multiple in (3, 6):                                      # MH_KF = 3 functions per pass over the k-mers
        assert {multiple - 1, multiple, multiple + 1} <= set(FUNCTION_COUNTS)
    assert min(FUNCTION_COUNTS) == 1 and max(FUNCTION_COUNTS) == 16
    for below, from_ in ((3, 4), (16, 17), (32, 33), (64, 65)):  # ndf_table_stride at 16 | 17 and 32 | 33, probe_pass up to 64
        assert {below, from_} <= set(TABLE_COUNTS)
    assert {HAMMING_DEDUPE_FROM - 1, HAMMING_DEDUPE_FROM, HAMMING_DEDUPE_FROM + 1} <= set(HAMMING_TABLES)
    assert {L % 8 for L in HAMMING_LENGTHS} >= {0, 1, 7} and min(HAMMING_LENGTHS) < 8
    for multiple in (8, 16, 64):
        assert {multiple - 1, multiple, multiple + 1} <= set(HAMMING_LENGTHS)
    assert set(HAMMING_DEVICE_LENGTHS) <= set(HAMMING_LENGTHS) and {L % 8 for L in HAMMING_DEVICE_LENGTHS} == {1, 0, 5}
    assert {0, 100} <= set(HAMMING_THRESHOLDS) and {1, 100} <= set(HAMMING_SAMPLED)
    assert all(len(set(p)) < len(p) for p in REPEATED_POSITIONS)
    for dist, _, m, near in THRESHOLD_CLASSES:                   # the reference's expression, on and beyond the threshold
        full = PAIR_L - PAIR_KS + 1
        assert (1.0 - float(m) / (2 * full - m) <= dist) == near and _need(2 * full, dist) == m + (0 if near else 1)
    assert 1.0 - 60.0 / 120.0 == 0.5 and not 1.0 - 60.0 / 120.0 <= float(np.nextafter(0.5, 0))


def test_minhash_cases_sit_on_their_branch_points(oracle):
    for name, c, claims in _all_minhash_cases(oracle):
        n, kept = len(c["strs"]), len(c["kept"])
        assert n <= MAX_PROBES, name
        assert ("own" not in claims) or c["largest"] > NDF_OWN_STEPS, (name, c["largest"])
        assert ("wave" not in claims) or c["largest"] > WAVE, (name, c["largest"])
        assert ("both" not in claims) or 0 < kept < n, (name, kept, n)
    for ks in KMER_SIZES:
        assert {len(s) for s in _kmer_case(oracle, ks)["strs"]} == {_kmer_length(ks)}
    for ks in KMER_SIZES_MORE:
        strs = _kmer_case(oracle, ks, planted_n=True)["strs"]
        assert len(strs) // 4 <= sum("N" in s for s in strs) <= len(strs) // 2
        g = _kmer_groups_case(oracle, ks)
        assert all(0 < len(k) < len(s) for k, s in zip(g["kept"], g["groups"])) and g["params"][0] != g["params"][1]
    for ks in MIXED_LENGTH_KMER_SIZES:
        c = _mixed_length_case(oracle, ks)
        assert set(range(ks, ks + 256)) == set(map(len, c["strs"]))             # one k-mer to 256 k-mers
        # mates of one bucket that differ so much in size that no intersection reaches the threshold (need > most)
        sizes = [len(_kmers(s, ks)) for s in c["strs"]]
        hopeless = sum(1 for row in c["keys"] for b in _buckets(row)
                       if _need(min(sizes[i] for i in b) + max(sizes[i] for i in b), 0.5) > min(sizes[i] for i in b))
        assert hopeless >= 10, (ks, hopeless)
    for ks in SECTION2_KMER_SIZES:
        c = _functions_case(oracle, ks, 16)
        assert sum(len(b) * (len(b) - 1) // 2 for row in c["keys"] for b in _buckets(row)) >= 10
        assert all(len(key) == 16 for key in c["keys"][0])
        c = _extreme_case(oracle, ks, 0.5)
        assert len(set(c["keys"][1])) == 1 and c["largest"] == len(c["strs"])     # a = 2^31 - 1: one bucket
        assert c["params"][1][0][0] == P31 and c["params"][2][0][1] == P31
        assert _extreme_case(oracle, ks, 1.0)["kept"] == c["strs"][:1] != c["kept"]


def test_threshold_pairs_share_buckets(oracle):
    """Liveness of section 3: in every class and form at least 50 pairs that sit exactly on (or one k-mer beyond) the
    threshold share a bucket, so their verdict is the comparison's -- and the oracle drops exactly the near ones."""
    for dist, nt, m, near in THRESHOLD_CLASSES:
        for form in ("pairs", "with_n"):
            c = _pair_case(oracle, dist, nt, m, form)
            strs = c["strs"]
            assert len(strs) == 2 * NPAIRS
            meet = _pairs_on_threshold(c, m)
            assert meet <= {(i, i + 1) for i in range(0, len(strs), 2)} and len(meet) >= 50, (dist, m, form, len(meet))
            dropped = {strs[j] for _, j in meet} if near else set()
            assert c["kept"] == [s for s in strs if s not in dropped]
            if form == "with_n":
                assert all("N" in strs[i] for i in range(0, len(strs), 2))
                assert sum("N" in strs[i] for i in range(1, len(strs), 2)) == NPAIRS // 2
        c = _pair_case(oracle, dist, nt, m, "family")
        strs = c["strs"]
        meet = _pairs_on_threshold(c, m)
        assert len(meet) >= 50, (dist, m, len(meet))
        # the walking probes' runs: the last probe of the largest bucket has all the others before it
        assert c["largest"] - 1 > WAVE and 0 < len(c["kept"]) < len(strs), (dist, m, c["largest"])
    # just below a boundary value the class on the threshold is not near any more
    c = _pair_case(oracle, float(np.nextafter(0.5, 0)), 13, 60, "pairs")
    assert c["kept"] == c["strs"] and len(_pairs_on_threshold(c, 60)) >= 50
    for ks in (2, 8):
        c = _equal_set_case(oracle, ks)
        sets = {frozenset(_kmers(s, ks)) for s in c["strs"]}
        assert len(c["kept"]) == len(sets) < len(c["strs"]) and len(c["params"]) == oracle.minhash_num_tables(0.0) == 1


def test_hamming_cases_sit_on_their_branch_points(oracle):
    for name, c, claims in _all_hamming_cases(oracle):
        n, kept = len(c["strs"]), len(c["kept"])
        assert ("own" not in claims) or c["largest"] > NDF_OWN_STEPS, (name, c["largest"])
        assert ("both" not in claims) or 0 < kept < n, (name, kept, n)
    assert _hamming_threshold_case(oracle, 0)["kept"] == _family_strs(100, 300)          # unique strings: none within 0
    assert _hamming_sampled_case(oracle, 1)["largest"] > WAVE
    for nt in HAMMING_TABLES:
        c = _hamming_tables_case(oracle, nt)
        assert len(c["positions"]) == nt and (len(_pairs_meeting_again(c)) >= 20) == (nt >= 2), nt
        per_table = _bucket_pairs(c["keys"])
        assert (sum(map(len, per_table)) - len(set().union(*per_table)) >= 100) == (nt >= 2), nt
    strs = _hamming_bytes_case(oracle)["strs"]
    assert sum("N" in s for s in strs) >= 50 and sum(s != s.upper() for s in strs) >= 50
    # (N equals N, a differs from A: a pair that differs in case only at up to two places is within 2)
    g = _hamming_groups_case(oracle)
    assert all(0 < len(k) < len(s) for k, s in zip(g["kept"], g["groups"]))


# ------------------------------------------------------------------ device side
def _assert_minhash(ctx, monkeypatch, c, forms=MH_FORMS):
    """The lazy resolution, the edge list over 16-byte ids and the lazy resolution without the staged codes keep what
    the oracle keeps, in its order."""
    strs = c["strs"]
    for hook in forms:
        with monkeypatch.context() as m:
            if hook:
                m.setenv(hook, "1")
            keep = ctx.ndf_minhash(strs, c["ks"], c["params"], c["dist"])
        got = [s for s, kp in zip(strs, keep) if kp]
        assert got == c["kept"], (hook or "lazy", c["ks"], c["dist"], len(got), len(c["kept"]))


def _minhash_filter(dist, ks, k, params):
    from catch_amd.filter import near_duplicate_filter as ndf
    f = ndf.NearDuplicateFilterWithMinHash(dist, ks)
    f.k = k
    f._draw_params = lambda: params
    return f


# ------------------------------------------------------------------ 1. MinHash: every k-mer size
@pytest.mark.gpu
@pytest.mark.parametrize("ks", KMER_SIZES)
def test_ndf_minhash_matches_oracle_at_every_kmer_size(ctx, oracle, monkeypatch, ks):
    c = _kmer_case(oracle, ks)
    assert 0 < len(c["kept"]) < len(c["strs"])
    _assert_minhash(ctx, monkeypatch, c)
    f = _minhash_filter(0.5, ks, 3, c["params"])
    assert f._filter_strs(c["strs"]) == oracle.as_list_of_set(c["kept"])


@pytest.mark.gpu
@pytest.mark.parametrize("ks", KMER_SIZES_MORE)
def test_ndf_minhash_with_n_round_the_id_word_and_code_limits(ctx, oracle, monkeypatch, ks):
    """An N in every third probe: pairs of a probe with 2-bit codes and one without, compared by their 16-byte ids."""
    _assert_minhash(ctx, monkeypatch, _kmer_case(oracle, ks, planted_n=True))


@pytest.mark.gpu
@pytest.mark.parametrize("ks", KMER_SIZES_MORE)
def test_ndf_minhash_many_round_the_id_word_and_code_limits(ctx, oracle, monkeypatch, ks):
    """Three groups in one call, hash functions of their own each: the oracle's selection group by group."""
    g = _kmer_groups_case(oracle, ks)
    for hook in MH_FORMS:
        with monkeypatch.context() as m:
            if hook:
                m.setenv(hook, "1")
            keeps = ctx.ndf_minhash_many(g["groups"], ks, g["params"], 0.5)
        got = [[s for s, kp in zip(strs, keep) if kp] for strs, keep in zip(g["groups"], keeps)]
        assert got == g["kept"], (hook or "lazy", ks)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", KMER_SIZES_MORE)
def test_ndf_minhash_on_device_candidates_round_the_id_word_and_code_limits(ctx, oracle, ks):
    """The same strings as sequences of one genome, one candidate each: the candidates the device keeps."""
    c = _kmer_case(oracle, ks)
    L = _kmer_length(ks)
    got = tpl._kept_on_device(ctx, [c["strs"]], L, L, lambda cands: cands.ndf_minhash(ks, c["params"], 0.5))
    assert got == oracle.as_list_of_set(c["kept"])


@pytest.mark.gpu
@pytest.mark.parametrize("ks", MIXED_LENGTH_KMER_SIZES)
def test_ndf_minhash_matches_oracle_from_1_to_256_kmers_per_probe(ctx, oracle, monkeypatch, ks):
    _assert_minhash(ctx, monkeypatch, _mixed_length_case(oracle, ks))


# ------------------------------------------------------------------ 2. MinHash: functions per table, tables, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("k", FUNCTION_COUNTS)
@pytest.mark.parametrize("ks", SECTION2_KMER_SIZES)
def test_ndf_minhash_matches_oracle_at_1_to_16_functions_per_table(ctx, oracle, monkeypatch, ks, k):
    """The key kernel takes three functions per pass over the k-mers: a clamped pass (1, 2), full ones (3, 6), a
    second and third pass with a clamped tail (4, 5, 7) and the most the entry takes (16)."""
    c = _functions_case(oracle, ks, k)
    _assert_minhash(ctx, monkeypatch, c)
    assert _minhash_filter(0.5, ks, k, c["params"])._filter_strs(c["strs"]) == oracle.as_list_of_set(c["kept"])


@pytest.mark.gpu
@pytest.mark.parametrize("ntables", TABLE_COUNTS)
@pytest.mark.parametrize("ks", SECTION2_KMER_SIZES)
def test_ndf_minhash_matches_oracle_at_1_to_65_tables(ctx, oracle, monkeypatch, ks, ntables):
    _assert_minhash(ctx, monkeypatch, _tables_case(oracle, ks, ntables))


@pytest.mark.gpu
@pytest.mark.parametrize("ks", SECTION2_KMER_SIZES)
def test_ndf_minhash_matches_oracle_at_the_ends_of_the_draw(ctx, oracle, monkeypatch, ks):
    """a = 2^31 - 1 (every probe in one bucket) and b = 2^31 - 1: the oracle's selection at 0.5; at 1.0 everything
    collapses into the first probe."""
    half, one = _extreme_case(oracle, ks, 0.5), _extreme_case(oracle, ks, 1.0)
    _assert_minhash(ctx, monkeypatch, half)
    _assert_minhash(ctx, monkeypatch, one)
    assert one["kept"] == one["strs"][:1] and len(half["kept"]) > 1


@pytest.mark.gpu
def test_ndf_minhash_refuses_what_lies_beyond_its_domain(ctx, oracle):
    strs = _family_strs(100, 110)[:50]
    params = _draw_params(oracle, 4, 3, 7)

    def with_first(ab):
        return [[ab] + list(params[0][1:])] + [list(t) for t in params[1:]]
    assert len(ctx.ndf_minhash(strs, 1, params, 0.5)) == len(ctx.ndf_minhash(strs, 16, params, 0.5)) == len(strs)
    for ks in (0, 17):
        with pytest.raises(ValueError):
            ctx.ndf_minhash(strs, ks, params, 0.5)
    with pytest.raises(ValueError):
        ctx.ndf_minhash(strs, 10, np.ones((0, 3, 2), dtype=np.int64), 0.5)
    for k in (0, 17):
        with pytest.raises(ValueError):
            ctx.ndf_minhash(strs, 10, np.ones((4, k, 2), dtype=np.int64), 0.5)
    for ab in ((0, 5), (2 ** 31, 5), (5, -1), (5, 2 ** 31)):
        with pytest.raises(ValueError):
            ctx.ndf_minhash(strs, 10, with_first(ab), 0.5)
    for ab in ((1, 0), (P31, P31)):
        assert len(ctx.ndf_minhash(strs, 10, with_first(ab), 0.5)) == len(strs)
    with pytest.raises(ValueError, match="shorter than the k-mer size"):
        ctx.ndf_minhash(strs + ["ACGTACGTA"], 10, params, 0.5)
    with pytest.raises(ValueError):
        ctx.ndf_minhash_many([strs[:25], strs[25:] + ["ACGTACGTA"]], 10, [params, params], 0.5)


# ------------------------------------------------------------------ 3. MinHash: pairs on the threshold
@pytest.mark.gpu
@pytest.mark.parametrize("form", PAIR_FORMS)
@pytest.mark.parametrize("dist,ntables,m,near", THRESHOLD_CLASSES)
def test_ndf_minhash_decides_pairs_on_the_threshold_as_the_oracle(ctx, oracle, monkeypatch, dist, ntables, m, near, form):
    """Pairs whose k-mer sets share exactly the number the threshold needs (near) or one fewer (not near): as separate
    pairs (a lane's own steps), inside families of 200 variants (the wave-shared walk) and with an N (16-byte ids)."""
    _assert_minhash(ctx, monkeypatch, _pair_case(oracle, dist, ntables, m, form))


@pytest.mark.gpu
def test_ndf_minhash_just_below_a_boundary_value_and_at_zero(ctx, oracle, monkeypatch):
    """dist_thres = nextafter(0.5, 0): the pairs at exactly 0.5 are kept, every one.  dist_thres = 0.0: different
    strings with equal k-mer sets collapse, a string with one k-mer more does not."""
    c = _pair_case(oracle, float(np.nextafter(0.5, 0)), 13, 60, "pairs")
    assert c["kept"] == c["strs"]
    _assert_minhash(ctx, monkeypatch, c)
    for ks in (2, 8):
        _assert_minhash(ctx, monkeypatch, _equal_set_case(oracle, ks))


# ------------------------------------------------------------------ 4. Hamming
def _assert_hamming(ctx, monkeypatch, c, k):
    from catch_amd.filter import near_duplicate_filter as ndf
    strs, L, pos, dist = c["strs"], c["L"], c["positions"], c["dist"]
    for hook in (None, "CATCHHIP_NDF_ALL_PAIRS"):
        with monkeypatch.context() as m:
            if hook:
                m.setenv(hook, "1")
            keep = ctx.ndf_hamming(strs, L, pos, dist)
        got = [s for s, kp in zip(strs, keep) if kp]
        assert got == c["kept"], (hook or "lazy", L, dist, len(got), len(c["kept"]))
    f = ndf.NearDuplicateFilterWithHammingDistance(dist, L)
    f.k = k
    f._draw_positions = lambda: pos
    assert f._filter_strs(strs) == c["as_set"]


@pytest.mark.gpu
@pytest.mark.parametrize("L", HAMMING_LENGTHS)
def test_ndf_hamming_matches_oracle_round_every_multiple_of_8(ctx, oracle, monkeypatch, L):
    """Rows are padded to words of 8 characters: lengths below one word, one short of, on and one past a multiple."""
    c = _hamming_length_case(oracle, L)
    _assert_hamming(ctx, monkeypatch, c, min(3, L))
    if L in HAMMING_DEVICE_LENGTHS:
        got = tpl._kept_on_device(ctx, [c["strs"]], L, L, lambda cands: cands.ndf_hamming(c["positions"], 2))
        assert got == c["as_set"]


@pytest.mark.gpu
@pytest.mark.parametrize("dist", HAMMING_THRESHOLDS)
def test_ndf_hamming_matches_oracle_from_threshold_0_to_the_length(ctx, oracle, monkeypatch, dist):
    _assert_hamming(ctx, monkeypatch, _hamming_threshold_case(oracle, dist), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", HAMMING_SAMPLED + ("repeated",))
def test_ndf_hamming_matches_oracle_from_1_to_100_sampled_positions(ctx, oracle, monkeypatch, k):
    """... and with tables that sample a position twice: the entry checks the range only, a key is the tuple."""
    _assert_hamming(ctx, monkeypatch, _hamming_sampled_case(oracle, k), 3 if k == "repeated" else k)


@pytest.mark.gpu
@pytest.mark.parametrize("ntables", HAMMING_TABLES)
def test_ndf_hamming_matches_oracle_from_1_to_8_tables(ctx, oracle, monkeypatch, ntables):
    """Across the table count from which a pair that met in an earlier table is skipped (four).  The edge list looks
    at every pair of a bucket, and so does the lazy resolution at dist_thres = 0, where no probe of a set of unique
    strings is near another and every walk runs to its end: the comparisons counted are the host's."""
    c = _hamming_tables_case(oracle, ntables)
    _assert_hamming(ctx, monkeypatch, c, 20)
    want = _comparisons_expected(c)
    with monkeypatch.context() as m:
        m.setenv("CATCHHIP_NDF_ALL_PAIRS", "1")
        ctx.ndf_hamming(c["strs"], 100, c["positions"], 6)
        assert ctx.ndf_counters()["pairs_compared"] == want
    assert ctx.ndf_hamming(c["strs"], 100, c["positions"], 0).all()
    assert ctx.ndf_counters()["pairs_compared"] == want


@pytest.mark.gpu
def test_ndf_hamming_refuses_what_lies_beyond_its_domain(ctx, oracle):
    strs = _family_strs(16, 216)[:50]
    assert len(ctx.ndf_hamming(strs, 16, [[0, 7, 15]], 2)) == len(strs)
    for positions in ([[0, 7, 16]], [[-1, 7, 15]], [[0, 1, 2], [3, 4, 99]], np.zeros((0, 3), dtype=np.int32),
                      np.zeros((2, 0), dtype=np.int32)):
        with pytest.raises(ValueError):
            ctx.ndf_hamming(strs, 16, positions, 2)
    with pytest.raises(ValueError):
        ctx.ndf_hamming(strs, 0, [[0, 0, 0]], 2)


@pytest.mark.gpu
def test_ndf_hamming_compares_bytes(ctx, oracle, monkeypatch):
    """Lower case and N among the substitutions: N equals N, a differs from A."""
    _assert_hamming(ctx, monkeypatch, _hamming_bytes_case(oracle), 3)


@pytest.mark.gpu
def test_ndf_hamming_many_matches_oracle_group_by_group(ctx, oracle):
    """Candidates of three groups with sampled positions of their own, four tables each."""
    engine = tpl.gp._engine()
    g = _hamming_groups_case(oracle)
    flat = "".join(s for strs in g["groups"] for s in strs)
    t = engine.Targets(ctx, g["groups"])
    t.set_groups(np.arange(3))
    c = engine.Candidates(ctx, t, 100, 100)
    try:
        c.ndf_hamming_many(g["positions"], 3)
        got = list(zip(c.groups().tolist(), (flat[p:p + 100] for p in c.positions().tolist())))
    finally:
        c.close(); t.close()
    for gi, want in enumerate(g["kept"]):
        assert sorted(s for grp, s in got if grp == gi) == sorted(want)
