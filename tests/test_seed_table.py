"""The seed table -- the hash table of anchor k-mers that both seed scans look target k-mers up in -- as its build
launches leave it (csrc/scan.hip: seed_init / seed_count / seed_alloc / seed_fill).

catchhip_selftest_seed_table (engine.Context.selftest_seed_table) builds the table of a probes object the way the
key-grouped join does or the way the seed-list scan does and copies it out: the 16-byte slots {key, first, count},
the entry ids grouped by key, the presence words, and what seed_alloc counted.  Every dump is compared with a
dictionary built here from the probe STRINGS, with the two hashes restated in Python:
  - every key sits in exactly one slot, reachable from its home slot without crossing an empty one;
  - count = the key's multiplicity, ents[first .. first + count) = exactly its entries;
  - the ranges are disjoint and tile [0, entries in the table);
  - a slot without entries has count 0, an empty slot is {EMPTY, 0, 0};
  - the presence words hold exactly the bits of the keys' masks (so every key's bits are set, and the set bits
    number at most bits-per-key x keys).
The shapes are the smallest at which each piece of the build can go wrong (see the cases).  The larger ones are also
scanned through engine.Rows.scan and compared with a brute-force Hamming scan in NumPy.
"""
import contextlib
import functools
import os
import random

import numpy as np
import pytest

from util import rows_as_tuples, small_species, candidates

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
EMPTY = M64
SLOT_N, SLOT_BITS = 0x80000000, 0x7fffffff


# ---- csrc/scan.hip restated ------------------------------------------------------------------------------------
def seed_hash(k):
    k ^= k >> 29
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 32
    return k & 0xffffffff


def seed_mix2(k):
    k ^= k >> 31
    k = (k * 0x94d049bb133111eb) & M64
    k ^= k >> 29
    return k


def seed_hash2(k):
    return seed_mix2(k) & 0xffffffff


def seed_presence(key, pmask, bits):
    """-> (word, mask) of a key in the presence words (seed_presence)."""
    h = seed_mix2(key)
    b = (h & 0xffffffff) & pmask
    m = 1 << (b & 31)
    if bits > 1:
        m |= 1 << ((h >> 32) & 31)
    if bits > 2:
        m |= 1 << ((h >> 37) & 31)
    return b >> 5, m


_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def kmer_key(s, k):
    """Planes 0 / 1 of the first min(k, 32) bases (an N reads as A)."""
    lo = hi = 0
    for i, c in enumerate(s[:min(k, 32)]):
        code = _CODE.get(c, 0)
        lo |= (code & 1) << i
        hi |= (code >> 1) << i
    return (hi << 32) | lo


def table_capacity(keys):
    cap = 1024
    while cap < 2 * keys:
        cap *= 2
    return cap


# ---- the check ---------------------------------------------------------------------------------------------------
def check_table(d, in_table, slot_only=(), bits=None):
    """d: a dump; in_table: {entry id: key} of the entries the table holds; slot_only: keys that have a slot and no
    entries (the seed-list scan's anchors beyond pos_limit); bits: bits per key expected (None: no presence words)."""
    cap, slots, ents = d["capacity"], d["slots"], d["ents"]
    assert cap >= 1024 and cap & (cap - 1) == 0 and slots.shape == (cap, 4)
    mask = cap - 1
    keys = (slots[:, 1].astype(np.uint64) << np.uint64(32)) | slots[:, 0].astype(np.uint64)
    first, count = slots[:, 2].astype(np.int64), slots[:, 3].astype(np.int64)
    used = keys != np.uint64(EMPTY)
    want = {}
    for e, key in in_table.items():
        want.setdefault(key, []).append(e)
    all_keys = set(want) | set(slot_only)
    assert 2 * len(all_keys) <= cap                      # (what ends every probe chain)
    # an empty slot is {EMPTY, 0, 0}
    assert not first[~used].any() and not count[~used].any()
    # every key in exactly one slot
    slot_of = {}
    for s in np.nonzero(used)[0]:
        key = int(keys[s])
        assert key not in slot_of, "key %x in two slots" % key
        slot_of[key] = int(s)
    assert set(slot_of) == all_keys
    # ... reachable from its home slot without crossing an empty one
    for key, s in slot_of.items():
        at, steps = seed_hash(key) & mask, 0
        while at != s:
            assert used[at], "key %x: an empty slot before its own" % key
            at = (at + 1) & mask
            steps += 1
            assert steps < cap
    # count = multiplicity, the range holds exactly the key's entries; a slot without entries has count 0
    for key, s in slot_of.items():
        mine = want.get(key, [])
        assert count[s] == len(mine), "key %x: count %d, %d entries" % (key, count[s], len(mine))
        if mine:
            assert sorted(int(x) for x in ents[first[s]:first[s] + count[s]]) == sorted(mine)
    # the ranges are disjoint and tile [0, entries in the table)
    has = np.nonzero(count > 0)[0]
    order = has[np.argsort(first[has], kind="stable")]
    ends = first[order] + count[order]
    n_table = len(in_table)
    if n_table:
        assert first[order[0]] == 0 and ends[-1] == n_table and (first[order[1:]] == ends[:-1]).all()
    assert d["entries"] == n_table and d["keys"] == len(want) == has.size
    # presence words
    if bits is None:
        assert d["present"].size == 0 and d["set_bits"] == 0
        return slot_of
    present = d["present"]
    assert d["bits_per_key"] == bits and present.size > 0 and present.size & (present.size - 1) == 0
    pmask = 32 * present.size - 1
    exp = np.zeros(present.size, dtype=np.uint32)
    for key in all_keys:
        w, m = seed_presence(key, pmask, bits)
        assert int(present[w]) & m == m, "key %x: a mask bit is not set" % key
        exp[w] |= np.uint32(m)
    assert (present == exp).all()
    nset = int(np.unpackbits(present.view(np.uint8)).sum())
    assert d["set_bits"] == nset and nset <= bits * len(all_keys)
    return slot_of


def pigeonhole_entries(probes, L, m):
    """-> (k, nanch, ntab, {entry: key} below pos_limit, {entry: key} of the rest)"""
    from catch_amd import probe
    k = probe.pigeonhole_kmer_length(L, m)
    nanch, ntab = L // k, min(L // k, m + 1)
    low, high = {}, {}
    for p, s in enumerate(probes):
        for a in range(nanch):
            (low if a < ntab else high)[p * nanch + a] = kmer_key(s[a * k:a * k + k], k)
    return k, nanch, ntab, low, high


def make_probes(ctx, probes, L, k, ent=None):
    from catch_amd import engine
    n = len(probes)
    if ent is None:
        nanch = L // k
        ep = np.repeat(np.arange(n, dtype=np.int32), nanch)
        eo = np.tile(np.arange(nanch, dtype=np.int32) * k, n)
    else:
        ep, eo = ent
    return engine.Probes(ctx, probes, np.arange(n, dtype=np.int32), ep, eo, k), int(len(ep))


@contextlib.contextmanager
def _env(**hooks):
    old = {k: os.environ.get(k) for k in hooks}
    try:
        for k, v in hooks.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rs(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def dump_join(ctx, probes, L, m, bits=None):
    """Dump of the join's table of `probes`, checked; -> (dump, slot of every key)."""
    k, nanch, ntab, low, _ = pigeonhole_entries(probes, L, m)
    P, nent = make_probes(ctx, probes, L, k)
    try:
        d = ctx.selftest_seed_table(P, nent, m)
    finally:
        P.close()
    assert d["capacity"] == table_capacity(len(probes) * nanch) and not d["filtered"]
    has_words = d["capacity"] >= 1 << 16
    return d, check_table(d, low, bits=(bits or d["bits_per_key"]) if has_words else None)


# ---- 1. every key has one entry; one seed_alloc workgroup and more ---------------------------------------------
@pytest.mark.parametrize("n", [100, 200, 400, 700])
def test_random_probes(ctx, n):
    """Random probes (L = 100, m = 2: three of four anchors enter, the table is sized by all four): every key has one
    entry.  100 and 200 probes: 1,024 and 2,048 slots, a part of the 4,096 of a seed_alloc workgroup; 400: 4,096, the
    whole of one; 700: 8,192, two workgroups."""
    rng = random.Random(1000 + n)
    probes = [_rs(rng, 100) for _ in range(n)]
    d, _ = dump_join(ctx, probes, 100, 2)
    assert d["capacity"] == {100: 1024, 200: 2048, 400: 4096, 700: 8192}[n]
    assert d["keys"] == d["entries"] == 3 * n and (d["slots"][:, 3] <= 1).all()


# ---- 2. hundreds of wavefronts count up and then down on one slot ------------------------------------------------
def test_one_key_many_entries(ctx):
    """One k-mer is anchor 0 of 700 distinct probes, and 300 of them share anchor 1 as well."""
    rng = random.Random(2)
    k0, k1 = _rs(rng, 25), _rs(rng, 25)
    probes = [k0 + (k1 if i < 300 else _rs(rng, 25)) + _rs(rng, 50) for i in range(700)]
    assert len(set(probes)) == 700
    d, slot_of = dump_join(ctx, probes, 100, 2)
    assert d["slots"][slot_of[kmer_key(k0, 25)], 3] == 700 and d["slots"][slot_of[kmer_key(k1, 25)], 3] == 300


# ---- 3. chains that wrap past slot 0 -----------------------------------------------------------------------------
def test_chain_wraps(ctx):
    """Ten distinct keys whose home slot is the table's last or second-to-last (found with the Python hash), two of
    them with 65 entries each: the chain runs on from slot 0."""
    rng = random.Random(3)
    cap = table_capacity(138 * 4)                        # of the 138 probes below
    found = []
    while len(found) < 10:
        s = _rs(rng, 25)
        if seed_hash(kmer_key(s, 25)) & (cap - 1) >= cap - 2 and s not in found:
            found.append(s)
    probes = [found[0] + _rs(rng, 75) for _ in range(65)] + [_rs(rng, 25) + found[1] + _rs(rng, 50) for _ in range(65)]
    probes += [f + _rs(rng, 75) for f in found[2:]]
    d, slot_of = dump_join(ctx, probes, 100, 2)
    assert len(probes) == 138 and d["capacity"] == cap == 2048   # (the homes are where they were looked for)
    homes = [slot_of[kmer_key(f, 25)] for f in found]
    assert sum(1 for s in homes if s < cap - 2) >= 8     # at least eight of the ten were pushed past slot 0
    assert d["slots"][homes[0], 3] == 65 and d["slots"][homes[1], 3] == 65


# ---- brute force -------------------------------------------------------------------------------------------------
def brute_rows(probes, genomes, L, m, ext, anchors=None, k=0):
    """(set, genome, start, end) of every probe against every window of every sequence (one sequence per genome):
    <= m mismatches (a target N matches nothing), with `anchors` (per probe, offsets) one of the probe's anchor
    k-mers exact; extended by ext, clipped, touching ranges merged."""
    seqs = [g[0] for g in genomes]
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    flat = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    oh = np.stack([(flat == ord(c)) for c in "ACGT"], axis=1).astype(np.float32)
    win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(oh, L, axis=0).transpose(0, 2, 1).reshape(-1, 4 * L))
    start = np.arange(win.shape[0], dtype=np.int64)
    sq = np.searchsorted(off, start, side="right") - 1
    inside = start + L <= off[sq + 1]
    pb = np.frombuffer("".join(probes).encode(), dtype=np.uint8).reshape(len(probes), L)
    poh = np.stack([(pb == ord(c)) for c in "ACGT"], axis=2).astype(np.float32).reshape(len(probes), 4 * L)
    per = {}
    for p0 in range(0, len(probes), 512):
        match = win @ poh[p0:p0 + 512].T                 # (windows, probes): matching bases
        hit = (match >= L - m) & inside[:, None]
        for i, j in zip(*np.nonzero(hit)):
            p = p0 + int(j)
            if anchors is not None:
                w = flat[i:i + L]
                if not any((w[a:a + k] == pb[p, a:a + k]).all() for a in anchors[p]):
                    continue
            g, at = int(sq[i]), int(start[i] - off[sq[i]])
            per.setdefault((p, g), []).append((max(0, at - ext), min(int(lens[g]), at + L + ext)))
    rows = []
    for (s, g), iv in per.items():
        iv.sort()
        cs, ce = iv[0]
        for a, b in iv[1:]:
            if a <= ce:
                ce = max(ce, b)
            else:
                rows.append((s, g, cs, ce))
                cs, ce = a, b
        rows.append((s, g, cs, ce))
    return sorted(rows)


def scan_rows(ctx, P, genomes, m, L, ext):
    from catch_amd import engine
    t = engine.Targets(ctx, genomes)
    try:
        rows = engine.Rows.scan(ctx, P, t, m, L, 0, ext, engine.SCAN_SEED)
        cn = ctx.counters()
        out = rows_as_tuples(*rows.fetch())
        rows.close()
    finally:
        t.close()
    return out, cn


# ---- 4. presence words in use: 1, 2 and 3 bits per key -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strains():
    """About 9,500 distinct probes (L = 100, stride 10) of 16 strains of one 8,000-base species: the join's table
    has 2^17 slots and presence words.  Targets: two of the strains.  -> (probes,
    genomes, brute-force rows, target positions whose k-mer is a key with entries)"""
    sp = small_species(seed=91, n=16, length=8000, with_n=False)
    probes = candidates(sp, 100, 10)
    assert 8200 <= len(probes) <= 16000
    genomes = [sp[0], sp[7]]
    k, nanch, ntab, low, _ = pigeonhole_entries(probes, 100, 2)
    keys = set(low.values())
    hitpos = sum(1 for g in genomes for s in g for i in range(len(s) - k + 1) if kmer_key(s[i:i + k], k) in keys)
    return probes, genomes, brute_rows(probes, genomes, 100, 2, 10), hitpos


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_presence_bits(ctx, bits):
    """Dump and scan with 1, 2 and 3 presence bits per key.  The rows equal the brute-force scan's and the seed-list
    scan's; join_hit_positions equals the target positions whose k-mer is a key with entries -- a false negative
    of the filter fails there even where it loses no row."""
    probes, genomes, exp, hitpos = strains()
    with _env(CATCHHIP_PRESENCE_BITS=bits):
        d, _ = dump_join(ctx, probes, 100, 2, bits=bits)
        assert d["capacity"] == 1 << 17 and d["present"].size == (1 << 17) // 32
        P, _ = make_probes(ctx, probes, 100, 25)
        try:
            rows, cn = scan_rows(ctx, P, genomes, 2, 100, 10)
            with _env(CATCHHIP_SEED_LIST=1):
                rows1, cn1 = scan_rows(ctx, P, genomes, 2, 100, 10)
        finally:
            P.close()
    print("bits", bits, "rows", len(rows), "hit positions", cn["join_hit_positions"], "set bits", d["set_bits"], "keys", d["keys"])
    assert len(exp) > 0 and rows == exp
    assert cn1["join_hit_positions"] == 0 and rows1 == exp
    assert cn["join_hit_positions"] == hitpos


# ---- 5. the seed-list scan's builder -------------------------------------------------------------------------------
def check_aslot(d, slot_of, all_entries):
    """The filtered look-up's slot of EVERY anchor's k-mer (no probe here holds an N)."""
    assert d["filtered"]
    for e, key in all_entries.items():
        assert int(d["aslot"][e]) == slot_of[key]


@pytest.mark.parametrize("which", ["small", "presence"])
def test_seed_list_pigeonhole(ctx, which):
    """A pigeonhole table as the seed-list scan builds it, the anchor-pair filter on: the anchor at pos_limit (the
    fourth of four) has a slot and no entries.  small: 1,024-odd slots and a scan against brute force; presence: the
    probes of case 4, whose table of 2^17 slots has presence words (four bits per slot, one per key)."""
    if which == "small":
        sp = small_species(seed=92, n=4, length=1500, with_n=False)
        probes, genomes, exp = candidates(sp, 100, 25), [sp[1], sp[2]], None
    else:
        probes, genomes, exp, _ = strains()
    k, nanch, ntab, low, high = pigeonhole_entries(probes, 100, 2)
    assert (nanch, ntab) == (4, 3) and set(high.values()) - set(low.values())
    P, nent = make_probes(ctx, probes, 100, k)
    try:
        d = ctx.selftest_seed_table(P, nent, 2, as_list=True)
        assert d["capacity"] == table_capacity(nent) and d["anchors_per_probe"] == 4
        slot_of = check_table(d, low, slot_only=set(high.values()) - set(low.values()),
                              bits=1 if which == "presence" else None)
        check_aslot(d, slot_of, {**low, **high})
        if which == "presence":
            assert d["present"].size == d["capacity"] // 8
        else:
            with _env(CATCHHIP_SEED_LIST=1):
                rows, cn = scan_rows(ctx, P, genomes, 2, 100, 10)
            assert cn["join_hit_positions"] == 0
            exp = brute_rows(probes, genomes, 100, 2, 10)
            assert len(exp) > 0 and rows == exp
    finally:
        P.close()


def test_seed_list_random_anchors(ctx):
    """A random-anchor table (m = 5, k = 20, 20 anchors per probe at random offsets) of 300 probes, every anchor in
    the table; targets holding N.  Dump, and a scan against brute force (<= 5 mismatches and one of the probe's own
    anchors exact)."""
    L, m, k = 100, 5, 20
    sp = small_species(seed=93, n=6, length=2000, with_n=False)
    probes = candidates(sp, L, 25)[:300]
    assert len(probes) == 300
    rng = random.Random(5)
    anchors = [sorted(rng.sample(range(L - k + 1), 20)) for _ in probes]
    ep = np.repeat(np.arange(300, dtype=np.int32), 20)
    eo = np.array([a for an in anchors for a in an], dtype=np.int32)
    genomes = []
    for g in sp[:3]:
        s = list(g[0])
        for i in rng.sample(range(len(s)), 12):
            s[i] = "N"
        genomes.append(["".join(s)])
    entries = {e: kmer_key(probes[e // 20][eo[e]:eo[e] + k], k) for e in range(6000)}
    P, nent = make_probes(ctx, probes, L, k, ent=(ep, eo))
    try:
        d = ctx.selftest_seed_table(P, nent, m, as_list=True)
        assert d["capacity"] == table_capacity(6000) and d["anchors_per_probe"] == 0
        slot_of = check_table(d, entries)
        check_aslot(d, slot_of, entries)
        rows, cn = scan_rows(ctx, P, genomes, m, L, 10)
    finally:
        P.close()
    exp = brute_rows(probes, genomes, L, m, 10, anchors=anchors, k=k)
    assert cn["join_hit_positions"] == 0 and len(exp) > 0 and rows == exp
