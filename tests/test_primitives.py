"""The two device-wide primitives of csrc/primitives.hip on their own: chip_exclusive_scan_u32 and
chip_radix_sort_pairs / chip_radix_sort_pairs_segments, through the test entry points catchhip_selftest_scan_u32 and
catchhip_selftest_sort_pairs (Context.selftest_scan_u32 / selftest_sort_pairs), which only copy in, call and copy out.

Every kernel family calls them, at the sizes its inputs happen to have; here they meet their own structural edges:
the 64-lane wavefront, the 2048-element scan tile and the second and third level of the scan's recursion (more than
2048 and more than 2048^2 elements), the 1024 keys a wavefront ranks and the 4096-key sort tile, the filler key ~0 of
the lanes past n, a histogram longer than one scan tile (more than 8 sort tiles), odd and even numbers of passes (the
result changes buffers every pass), bits outside the sorted range carried along, stability, and the segment offset of
the segmented scatter.  All results are integers and every comparison is for equality: the scan against
np.cumsum in 64 bits masked to 32, the sort against np.argsort(kind="stable") of the sorted bits.

Not covered here: the third scan level inside ONE sort (a histogram of more than 2048^2 counters: about 67 M keys; the
65,535 two-key segments of the refusal test do scan 16.8 M counters, but one tile per segment) and the n * nseg
arithmetic of the segmented sort near 2^32.  The full-size digests of bench.py remain the check for both.

The wavefront-level helpers of csrc/wave.h (reductions, scans, DPP sums, find_segment) are below the two, through
catchhip_selftest_wave and catchhip_selftest_find_segment: one kernel that calls every helper on one value per thread
and hands back what every thread got.

The base-interval helpers of csrc/spans.h (the words and end masks of [a, b) on a bitmap, paint, all-set test,
popcount, difference mark) are at the end, through catchhip_selftest_spans: one interval per thread, over every pair
of the points at which a mask can be off by one, against a model of one boolean per base.
"""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1
SCAN_TILE = 2048
SORT_TILE = 4096


# ------------------------------------------------------------------ references
def expected_scan(x):
    """Exclusive prefix sum mod 2^32: np.cumsum in 64 bits, shifted by one, masked."""
    inc = np.cumsum(np.asarray(x, dtype=np.uint32), dtype=np.uint64)
    out = np.zeros(inc.size, dtype=np.uint64)
    out[1:] = inc[:-1]
    return (out & np.uint64(0xffffffff)).astype(np.uint32)


def sort_passes(key_bits):
    return max(1, -(-key_bits // 8))


def sorted_bits(keys, key_bits, first_bit):
    """The bits a call orders by: [first_bit, first_bit + 8 * passes), as a number."""
    width = min(8 * sort_passes(key_bits), 64 - first_bit)
    return (keys >> np.uint64(first_bit)) & np.uint64(MASK64 >> (64 - width))


def expected_perm(keys, key_bits, first_bit):
    return np.argsort(sorted_bits(keys, key_bits, first_bit), kind="stable")


PATTERNS = ("random", "all_equal", "all_ones", "two_values", "ascending", "descending", "tile_of_one_digit")


def make_keys(rng, n, key_bits, first_bit, pattern):
    """n 64-bit keys.  The field [first_bit, first_bit + key_bits) follows `pattern`; the bits from its end to the
    next byte boundary of the sorted range are zero, as every caller keeps them; all bits below first_bit and above
    the sorted range are random and must come back untouched."""
    field_mask = (1 << key_bits) - 1
    if pattern == "random":
        field = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    elif pattern == "all_equal":
        field = np.full(n, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    elif pattern == "all_ones":           # the digit of the filler key in every pass that lies inside the field
        field = np.full(n, MASK64, dtype=np.uint64)
    elif pattern == "two_values":
        field = np.where(rng.integers(0, 2, size=n).astype(bool), np.uint64(0x0123456789abcdef), np.uint64(0xfedcba9876543210))
    elif pattern == "ascending":
        field = np.arange(n, dtype=np.uint64)
    elif pattern == "descending":
        field = np.arange(n, dtype=np.uint64)[::-1].copy()
    elif pattern == "tile_of_one_digit":  # the second sort tile (when there is one) holds one value of the lowest digit
        field = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        field[SORT_TILE:2 * SORT_TILE] = (field[SORT_TILE:2 * SORT_TILE] & np.uint64(MASK64 ^ 0xff)) | np.uint64(0x07)
    else:
        raise AssertionError(pattern)
    field = field & np.uint64(field_mask)
    other = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    top = first_bit + 8 * sort_passes(key_bits)
    keep = (MASK64 >> (64 - first_bit) if first_bit else 0) | ((MASK64 << top) & MASK64 if top < 64 else 0)
    return (other & np.uint64(keep)) | ((field << np.uint64(first_bit)) & np.uint64(MASK64))


# ------------------------------------------------------------------ without a GPU
def test_selftest_symbols_declared_bound_and_wrapped():
    from catch_amd import _lib, engine
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    src = open(os.path.join(REPO, "catch_amd", "csrc", "primitives.hip")).read()
    for name in ("catchhip_selftest_scan_u32", "catchhip_selftest_sort_pairs", "catchhip_selftest_wave",
                 "catchhip_selftest_find_segment", "catchhip_selftest_spans"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r'extern "C" int %s\s*\(' % name, src), name
        assert name in _lib.PROTOTYPES, name
    assert callable(engine.Context.selftest_scan_u32) and callable(engine.Context.selftest_sort_pairs)
    assert callable(engine.Context.selftest_wave) and callable(engine.Context.selftest_find_segment)
    assert callable(engine.Context.selftest_spans)
    # the structural sizes this file is written around
    assert re.search(r"#define SCAN_THREADS 256\b", src) and re.search(r"#define SCAN_ITEMS 8\b", src)
    assert re.search(r"#define RS_THREADS 256\b", src) and re.search(r"#define RS_ROUNDS 16\b", src)
    assert "nseg > 65535" in src


def test_references_and_key_maker_are_what_they_claim():
    """The expected values on inputs small enough to write down, and the key maker's promises: the gap up to the
    byte boundary is zero, the field follows the pattern, bits outside the sorted range are not all alike."""
    assert expected_scan([]).tolist() == []
    assert expected_scan([5]).tolist() == [0]
    assert expected_scan([1, 2, 3, 0xffffffff, 7]).tolist() == [0, 1, 3, 6, 5]       # 6 + 0xffffffff wraps to 5
    assert [sort_passes(b) for b in (0, 1, 8, 9, 13, 32, 33, 40, 64)] == [1, 1, 1, 2, 2, 4, 5, 5, 8]
    k = np.array([0x0300, 0x0101, 0x0200, 0x0100, 0xff0000000100], dtype=np.uint64)
    assert expected_perm(k, 16, 0).tolist() == [3, 4, 1, 2, 0]          # bits 16 and above do not order
    assert expected_perm(k, 8, 8).tolist() == [1, 3, 4, 2, 0]           # stable inside digit 1; bits 0-7 do not order
    assert expected_perm(k, 0, 32).tolist() == [0, 1, 2, 3, 4]          # one pass over bits 32-39: 0, 0, 0, 0, 0
    rng = np.random.default_rng(1)
    for key_bits, first_bit in SORT_SHAPES:
        top = first_bit + 8 * sort_passes(key_bits)
        for pattern in PATTERNS:
            keys = make_keys(rng, 9000, key_bits, first_bit, pattern)
            gap = (keys >> np.uint64(first_bit + key_bits)) & np.uint64((1 << (top - first_bit - key_bits)) - 1) \
                if top > first_bit + key_bits else np.zeros(1, np.uint64)
            assert not gap.any(), (key_bits, first_bit, pattern)
            if first_bit:
                assert np.unique(keys & np.uint64((1 << first_bit) - 1)).size > 8000
            if top < 64:
                assert np.unique(keys >> np.uint64(top)).size > min(8000, (1 << (64 - top)) // 2)
            field = sorted_bits(keys, key_bits, first_bit)
            if pattern in ("all_equal", "all_ones"):
                assert np.unique(field).size == 1
                if pattern == "all_ones":
                    assert int(field[0]) == (1 << key_bits) - 1
            if pattern == "two_values" and key_bits:
                assert np.unique(field).size == 2
            if pattern == "tile_of_one_digit" and key_bits >= 8:
                assert set((field[SORT_TILE:2 * SORT_TILE] & np.uint64(0xff)).tolist()) == {7}


# ------------------------------------------------------------------ scan
# both sides of: the wavefront (64), a thread's 8 items, the tile (2048), the second level (> 2048 elements: two and
# more tiles), a second-level tile boundary, the third level (> 2048^2 elements)
SCAN_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5, 100003,
              2048 * 2047 + 1, 2048 * 2048 - 1, 2048 * 2048, 2048 * 2048 + 1, 2048 * 2048 + 2048 + 77)


def _scan_input(kind, n):
    rng = np.random.default_rng(n + 17)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "runs":          # 0 / 1 flags in runs of up to 5,000: longer than a tile, shorter than a wavefront
        lens = rng.integers(1, 5001, size=n // 1000 + 2)
        lens[::7] = rng.integers(1, 40, size=lens[::7].size)
        flags = np.repeat(np.arange(lens.size) & 1, lens)[:n]
        assert flags.size == n
        return flags.astype(np.uint32)
    assert kind == "random"     # full range: the sums wrap many times (analysis.hip relies on wrapping sums)
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeros", "ones", "runs", "random"])
def test_exclusive_scan_equals_cumsum(ctx, kind):
    levels = {1: 0, 2: 0, 3: 0}
    for n in SCAN_SIZES:
        x = _scan_input(kind, n)
        want = expected_scan(x)
        for in_place in (False, True):
            got = ctx.selftest_scan_u32(x, in_place=in_place)
            assert got.dtype == np.uint32 and got.shape == want.shape
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (kind, n, in_place, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        tiles = -(-n // SCAN_TILE)
        levels[1 if tiles <= 1 else 2 if tiles <= SCAN_TILE else 3] += 1
        if kind == "random" and n >= 64:
            assert int(x.astype(np.uint64).sum()) >= 1 << 32        # (the sums did wrap)
    assert levels[1] >= 10 and levels[2] >= 8 and levels[3] >= 2
    print("scan %s: %d sizes in and out of place, up to %d elements; recursion levels 1/2/3 reached by %d/%d/%d sizes; "
          "above 2048^2: %s" % (kind, len(SCAN_SIZES), max(SCAN_SIZES), levels[1], levels[2], levels[3],
                                [n for n in SCAN_SIZES if n > SCAN_TILE * SCAN_TILE]))


# ------------------------------------------------------------------ sort
# (key_bits, first_bit) as the callers use them: whole keys, 32 bits, computed widths that end inside a byte, the
# upper half of a key; (0, 32) is one pass over bits 32-39.  Passes: 8, 4, 5, 5, 1, 2, 2, 2, 1.
SORT_SHAPES = ((64, 0), (32, 0), (33, 0), (40, 0), (1, 0), (13, 0), (13, 32), (9, 32), (0, 32))
# both sides of the wavefront's 1024 keys and of the 4096-key tile, two tiles and a bit, more than 8 tiles (the
# histogram of 256 counters per tile passes one scan tile), about 10^5
SORT_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1234, 8 * 4096, 8 * 4096 + 1, 9 * 4096 + 1, 100003)


def _check_sort(ctx, keys, key_bits, first_bit, what):
    n = keys.size
    vals = np.arange(n, dtype=np.uint32)
    got_k, got_v = ctx.selftest_sort_pairs(keys, vals, key_bits, first_bit)
    perm = expected_perm(keys, key_bits, first_bit)
    bad = np.nonzero(got_v != perm)[0]
    assert bad.size == 0, what + (bad[:5].tolist(), got_v[bad[:5]].tolist(), perm[bad[:5]].tolist())
    assert np.array_equal(got_k, keys[perm]), what          # all 64 bits of every key


@pytest.mark.gpu
@pytest.mark.parametrize("key_bits,first_bit", SORT_SHAPES)
def test_radix_sort_equals_stable_argsort(ctx, key_bits, first_bit):
    rng = np.random.default_rng(1000 * key_bits + first_bit)
    calls = 0
    for n in SORT_SIZES:
        for pattern in PATTERNS:
            if pattern == "tile_of_one_digit" and n <= SORT_TILE:
                continue
            keys = make_keys(rng, n, key_bits, first_bit, pattern)
            _check_sort(ctx, keys, key_bits, first_bit, (key_bits, first_bit, n, pattern))
            calls += 1
    passes = sort_passes(key_bits)
    assert any(n % SORT_TILE for n in SORT_SIZES if n > SORT_TILE)      # (the filler key's digit meets real all-ones keys)
    print("sort key_bits %d first_bit %d: %d passes (%s: the result comes back from the %s buffer), %d calls, sizes %s; "
          "histogram of %d counters at the largest"
          % (key_bits, first_bit, passes, "odd" if passes & 1 else "even", "swapped" if passes & 1 else "original",
             calls, list(SORT_SIZES), 256 * -(-max(SORT_SIZES) // SORT_TILE)))


def test_sort_shapes_hold_odd_and_even_pass_counts():
    passes = [sort_passes(b) for b, _ in SORT_SHAPES]
    assert any(p & 1 for p in passes) and any(not p & 1 for p in passes) and 1 in passes and 8 in passes
    assert {f for _, f in SORT_SHAPES} == {0, 32}


# ------------------------------------------------------------------ segmented sort
SEG_COUNTS = (1, 2, 25, 300)
SEG_SIZES = (2, 37, 4095, 4096, 4097, 2 * 4096 + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("key_bits", [32, 64])
def test_segmented_sort_sorts_every_segment_on_its_own(ctx, key_bits):
    """Segments side by side with values numbered through ALL segments: every segment must come back as its own
    stable sort, so a key that crossed a boundary, or a segment written at another's place, shows in the values.
    The same small set of keys occurs in every segment (ties within and across segments)."""
    rng = np.random.default_rng(key_bits)
    most = 0
    for nseg in SEG_COUNTS:
        for n in SEG_SIZES:
            for pattern in ("random", "two_values", "few"):
                if pattern == "few":
                    keys = make_keys(rng, 11, key_bits, 0, "random")[rng.integers(0, 11, size=n * nseg)]
                else:
                    keys = make_keys(rng, n * nseg, key_bits, 0, pattern)
                vals = np.arange(n * nseg, dtype=np.uint32)
                got_k, got_v = ctx.selftest_sort_pairs(keys, vals, key_bits, 0, nseg=nseg)
                seg_keys = keys.reshape(nseg, n)
                perm = np.argsort(sorted_bits(seg_keys, key_bits, 0), axis=1, kind="stable")
                want_v = (perm + np.arange(nseg)[:, None] * n).reshape(-1)
                bad = np.nonzero(got_v != want_v)[0]
                assert bad.size == 0, (key_bits, nseg, n, pattern, bad[:5].tolist(), got_v[bad[:5]].tolist(),
                                       want_v[bad[:5]].tolist())
                assert np.array_equal(got_k, np.take_along_axis(seg_keys, perm, axis=1).reshape(-1))
                assert np.array_equal(got_v // n if n else got_v, np.repeat(np.arange(nseg), n))    # nothing crossed
                most = max(most, n * nseg)
    print("segmented sort key_bits %d: segments %s x sizes %s, up to %d keys in one call"
          % (key_bits, list(SEG_COUNTS), list(SEG_SIZES), most))


@pytest.mark.gpu
def test_segmented_sort_refuses_65536_segments(ctx):
    keys = np.arange(2 * 65536, dtype=np.uint64)
    with pytest.raises(ValueError, match="radix sort: too many keys in all segments"):
        ctx.selftest_sort_pairs(keys, np.arange(keys.size, dtype=np.uint32), 32, 0, nseg=65536)
    # 65,535 segments are taken
    keys = np.arange(2 * 65535, dtype=np.uint64)[::-1].copy()
    got_k, got_v = ctx.selftest_sort_pairs(keys, np.arange(keys.size, dtype=np.uint32), 32, 0, nseg=65535)
    assert np.array_equal(got_k, keys.reshape(-1, 2)[:, ::-1].reshape(-1))
    assert np.array_equal(got_v, np.arange(keys.size).reshape(-1, 2)[:, ::-1].reshape(-1))


# ------------------------------------------------------------------ wave.h
WAVE_PATTERNS = ("zeros", "all_ones", "ramp", "lane0", "lane63", "lane15", "lane16", "lanes15_16", "lane31", "lane32",
                 "lanes31_32", "random")
WAVE_SIZES = (256, 512)     # one workgroup of four wavefronts, and two


def _wave_input(pattern, n):
    """One value per thread.  The single-lane patterns put a value that differs from wavefront to wavefront (and has
    its top bit set: two of them wrap) into the named lanes of every wavefront: lane 0 and lane 63 are the ends of the
    shuffles, 15|16 and 31|32 the borders of the DPP rows and of the row broadcasts."""
    x = np.zeros(n, dtype=np.uint32)
    lanes = {"lane0": (0,), "lane63": (63,), "lane15": (15,), "lane16": (16,), "lanes15_16": (15, 16), "lane31": (31,),
             "lane32": (32,), "lanes31_32": (31, 32)}
    if pattern == "zeros":
        pass
    elif pattern == "all_ones":
        x[:] = 0xffffffff
    elif pattern == "ramp":
        x[:] = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
    elif pattern == "random":
        x[:] = np.random.default_rng(n).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    else:
        for lane in lanes[pattern]:
            x[lane::64] = np.uint32(0x80000001) + np.arange(n // 64, dtype=np.uint32) * np.uint32(0x01010101) + np.uint32(lane)
    return x


def _wave_expected(x):
    """NumPy's answers, per thread; None where a helper promises nothing (every lane but 0 of a lane-0 form)."""
    m32 = np.uint64(0xffffffff)
    w = x.reshape(-1, 64).astype(np.uint64)
    inc = np.cumsum(w, axis=1) & m32
    tot = (w.sum(axis=1) & m32)[:, None]
    ones = np.ones_like(w)
    w64 = ((w & np.uint64(0xffff)) << np.uint64(32)) | w
    exp = {
        "wave_sum": tot[:, 0], "wave_max": w.max(axis=1),                    # lane 0 of every wavefront only
        "wave_sum_all": tot * ones, "wave_max_all": w.max(axis=1)[:, None] * ones,
        "wave_incl_scan": inc, "wave_excl_scan": (inc - w) & m32, "wave_excl_scan_total": tot * ones,
        "wave_incl_scan_dpp": inc,
        "quad_sum": np.repeat(x.reshape(-1, 4).astype(np.uint64).sum(axis=1) & m32, 4),
        "row8_sum": np.repeat(x.reshape(-1, 8).astype(np.uint64).sum(axis=1) & m32, 8),
        "wave_max_u64": w64.max(axis=1),                                       # lane 0 only
        "wave_incl_scan_u64": np.cumsum(w64, axis=1),
    }
    return {k: v.reshape(-1) for k, v in exp.items()}


LANE0_FORMS = ("wave_sum", "wave_max", "wave_max_u64")


def test_wave_references_on_a_case_written_down():
    x = np.zeros(256, dtype=np.uint32)
    x[0], x[1], x[63], x[64] = 0xffffffff, 2, 5, 7
    e = _wave_expected(x)
    assert e["wave_sum"].tolist() == [6, 7, 0, 0] and e["wave_max"].tolist() == [0xffffffff, 7, 0, 0]
    assert e["wave_incl_scan"][:3].tolist() == [0xffffffff, 1, 1] and int(e["wave_incl_scan"][63]) == 6
    assert e["wave_excl_scan"][:3].tolist() == [0, 0xffffffff, 1] and set(e["wave_excl_scan_total"][:64].tolist()) == {6}
    assert e["quad_sum"][:5].tolist() == [1, 1, 1, 1, 0] and e["row8_sum"][56:65].tolist() == [5] * 8 + [7]
    assert int(e["wave_max_u64"][0]) == (0xffff << 32) | 0xffffffff and int(e["wave_incl_scan_u64"][1]) == (0xffff << 32) + 0xffffffff + (2 << 32) + 2
    for pattern in WAVE_PATTERNS:
        for n in WAVE_SIZES:
            v = _wave_input(pattern, n)
            assert v.size == n and (pattern == "zeros") == (not v.any())
    assert np.count_nonzero(_wave_input("lanes15_16", 256)) == 8 and np.count_nonzero(_wave_input("lane63", 512)) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", WAVE_PATTERNS)
def test_wave_helpers_equal_numpy(ctx, pattern):
    """Lane-0 forms are asserted in lane 0 of each wavefront, everything else in every lane."""
    for n in WAVE_SIZES:
        x = _wave_input(pattern, n)
        got, want = ctx.selftest_wave(x), _wave_expected(x)
        assert set(got) == set(want)
        for name in got:
            g = got[name][::64] if name in LANE0_FORMS else got[name]
            assert g.shape == want[name].shape, (pattern, n, name)
            bad = np.nonzero(g.astype(np.uint64) != want[name])[0]
            assert bad.size == 0, (pattern, n, name, bad[:5].tolist(), g[bad[:5]].tolist(), want[name][bad[:5]].tolist())


def _segment_tables():
    rng = np.random.default_rng(300)
    lens300 = rng.integers(0, 40, size=300)
    lens300[rng.integers(0, 300, size=60)] = 0
    tables = {
        "n1": [5], "n2": [3, 4], "n300": lens300,
        "empty_front": [0, 0, 0, 4, 5], "empty_middle": [3, 0, 2, 0, 0, 0, 0, 6, 0, 0, 1, 9], "empty_end": [4, 5, 0, 0, 0],
    }
    return {k: np.concatenate(([0], np.cumsum(v))).astype(np.uint32) for k, v in tables.items()}


def test_segment_tables_are_what_they_claim():
    t = _segment_tables()
    assert t["n1"].tolist() == [0, 5] and t["n2"].tolist() == [0, 3, 7] and t["n300"].size == 301
    assert t["empty_front"][:4].tolist() == [0, 0, 0, 0] and t["empty_end"][-4:].tolist() == [9, 9, 9, 9]
    d = np.diff(t["empty_middle"].astype(np.int64))
    assert d[0] > 0 and d[-1] > 0 and (d[3:7] == 0).all()
    d = np.diff(t["n300"].astype(np.int64))
    assert (d == 0).sum() >= 40 and ((d[1:] == 0) & (d[:-1] == 0)).any() and all(int(v[-1]) > 0 for v in t.values())
    # the reference on a table small enough to write down: off = [0, 0, 0, 0, 4, 9]
    assert np.searchsorted(t["empty_front"][1:], np.arange(9), side="right").tolist() == [3] * 4 + [4] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["n1", "n2", "n300", "empty_front", "empty_middle", "empty_end"])
def test_find_segment_equals_searchsorted(ctx, table):
    off = _segment_tables()[table]
    n = off.size - 1
    x = np.arange(int(off[n]), dtype=np.uint32)           # every x of the contract: [0, off[n])
    got = ctx.selftest_find_segment(off, x)
    want = np.searchsorted(off[1:n + 1], x, side="right")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (table, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert (off[got] <= x).all() and (x < off[got + 1]).all()


# ------------------------------------------------------------------ spans.h
SPAN_T = 449                # bases of the space: no multiple of 64, and more than SUB_MAXW + 1 = 6 words
SPAN_WORDS = 8
SPAN_POINTS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 319, 320, 321, 384, 385, SPAN_T - 1, SPAN_T)
SPAN_INTERVALS = [(a, b) for a in SPAN_POINTS for b in SPAN_POINTS if a < b]


def _words(bits):
    """uint64 words of a boolean per base (rows of 64 * k booleans -> rows of k words), bit i of a word = base i."""
    bits = np.asarray(bits, dtype=bool)
    return np.packbits(bits.reshape(bits.shape[:-1] + (-1, 64)), axis=-1, bitorder="little").view("<u8")[..., 0]


def _span_bitmap(kind):
    if kind == "random":
        return np.random.default_rng(449).integers(0, 2, size=64 * SPAN_WORDS).astype(bool)
    return np.full(64 * SPAN_WORDS, kind == "ones")


def _span_expected(bm_bits, view):
    """The model: one boolean per base.  Nothing here shifts or masks a word."""
    a = np.array([i[0] for i in SPAN_INTERVALS])[:, None]
    b = np.array([i[1] for i in SPAN_INTERVALS])[:, None]
    pos = np.arange(64 * SPAN_WORDS)[None, :]
    inside = (pos >= a) & (pos < b)                                  # [interval][base]
    in_word = np.arange(64)[None, :]
    masks = _words(inside)                                           # [interval][word]
    diff = np.zeros(64 * SPAN_WORDS + 1, dtype=np.uint64)
    np.add.at(diff, a[:, 0], 1)
    np.add.at(diff, b[:, 0], 0xffffffff)
    return {
        "first_word": a[:, 0] // 64, "words": (b[:, 0] - 1) // 64 - a[:, 0] // 64 + 1,
        "first_mask": _words(in_word >= a % 64)[:, 0], "last_mask": _words(in_word <= (b - 1) % 64)[:, 0],
        "word_view": masks[:, view],
        "popcount": (inside & bm_bits[None, :]).sum(axis=1), "all_set": (~inside | bm_bits[None, :]).all(axis=1),
        "painted": np.bitwise_or.reduce(masks, axis=0), "diff": diff & np.uint64(0xffffffff),
    }


def test_span_model_on_cases_written_down():
    assert len(SPAN_INTERVALS) == 120 and SPAN_T > 6 * 64 and SPAN_T % 64 and SPAN_T <= 64 * SPAN_WORDS
    lens = {(b - 1) // 64 - a // 64 + 1 for a, b in SPAN_INTERVALS}
    assert {1, 2, 5, 6, 8} <= lens and (0, 64) in SPAN_INTERVALS and (63, 64) in SPAN_INTERVALS
    assert (SPAN_T - 1, SPAN_T) in SPAN_INTERVALS and (64, 384) in SPAN_INTERVALS      # one base; five whole words
    assert _words(np.arange(128) == 65).tolist() == [0, 2] and int(_words(np.ones(64, bool))[0]) == MASK64
    e = _span_expected(_span_bitmap("random"), 1)
    i = SPAN_INTERVALS.index((63, 129))
    assert (int(e["first_word"][i]), int(e["words"][i])) == (0, 3)
    assert (int(e["first_mask"][i]), int(e["last_mask"][i]), int(e["word_view"][i])) == (1 << 63, 1, MASK64)
    i = SPAN_INTERVALS.index((1, 62))                                # one word: the two masks overlap
    assert (int(e["first_mask"][i]), int(e["last_mask"][i])) == (MASK64 - 1, MASK64 >> 2) and int(e["word_view"][i]) == 0
    assert int(e["diff"][0]) == 15 and int(e["diff"][SPAN_T]) == (-15) & 0xffffffff and int(e["diff"].sum()) % (1 << 32) == 0
    assert e["painted"].tolist() == [MASK64] * 7 + [(1 << (SPAN_T - 448)) - 1]
    ones = _span_expected(_span_bitmap("ones"), 0)
    assert ones["all_set"].all() and ones["popcount"].tolist() == [b - a for a, b in SPAN_INTERVALS]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
def test_span_helpers_equal_bit_model(ctx, kind):
    bm_bits = _span_bitmap(kind)
    a, b = np.array(SPAN_INTERVALS, dtype=np.uint32).T
    for view in range(SPAN_WORDS):
        got, want = ctx.selftest_spans(_words(bm_bits), a, b, view), _span_expected(bm_bits, view)
        assert set(got) == set(want)
        for name in got:
            g, w = got[name].astype(np.uint64), np.asarray(want[name]).astype(np.uint64)
            assert g.shape == w.shape, (kind, view, name)
            bad = np.nonzero(g != w)[0]
            where = [SPAN_INTERVALS[k] for k in bad[:5]] if g.size == len(SPAN_INTERVALS) else bad[:5].tolist()
            assert bad.size == 0, (kind, view, name, where, g[bad[:5]].tolist(), w[bad[:5]].tolist())
