"""One list of records against another (catch_amd/filter/cross_dimer.py: cross_against, conflicts_with;
csrc/cross.hip: catchhip_cross_against / _flags): both C entries and the NumPy form against the definition, at the
tile edges of either list, the word edges of the bit planes and every form of the run search.  Every comparison is of
exact integers.  The model of the large lists is a run matrix computed once here, block by block, and held to the
quantifiers of the definition on a sample and on the planted pairs."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RC = str.maketrans("ACGT", "TGCA")

LENGTHS = (0, 1, 2, 63, 64, 65, 100, 127, 128, 129, 255, 256)
SIZES = (0, 1, 63, 64, 65, 130)
STRETCHES = (1, 20, 21, 63, 64, 65, 100, 128, 200, 256)
THRESHOLDS = (1, 20, 62, 63, 64, 65, 100, 255, 256)
N = 130
_shared = {}


def _rc(s):
    return s[::-1].translate(_RC)


def _cd():
    from catch_amd.filter import cross_dimer
    return cross_dimer


def _random(rng, length, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=length)) if length else ""


def _block(bs, as_):
    """int32 (len(bs), len(as_)): run(b, a), by the recurrence of cross_dimer.run_rows over the cells of this block
    alone (as wide as ITS longest record of `as_`, as many steps as its longest of `bs`)."""
    cd = _cd()
    out = np.zeros((len(bs), len(as_)), dtype=np.int32)
    if not bs or not as_:
        return out
    d = cd._digits(as_)
    L = d.shape[1]
    wants = np.where(d >= 0, 3 - d, -2).astype(np.int8)
    mine = cd._digits(bs)
    cells = np.zeros((len(bs), len(as_), L + 1), dtype=np.int16)
    for x in range(mine.shape[1]):
        m = wants[None, :, :] == mine[:, x][:, None, None]
        cells[:, :, :L] = (cells[:, :, 1:] + 1) * m
        np.maximum(out, cells[:, :, :L].max(axis=2), out=out)
    return out


def _matrix(bs, as_):
    """_block over the four blocks of short (at most 65 characters) and long records: the long ones are few."""
    out = np.zeros((len(bs), len(as_)), dtype=np.int32)
    for b_long in (False, True):
        bi = [i for i, s in enumerate(bs) if (len(s) > 65) == b_long]
        for a_long in (False, True):
            ai = [j for j, s in enumerate(as_) if (len(s) > 65) == a_long]
            if bi and ai:
                out[np.ix_(bi, ai)] = _block([bs[i] for i in bi], [as_[j] for j in ai])
    return out


def _place(k, where):
    """(record length, offset) for a stretch of k characters at the record's start, at its end, or across the border of
    the first and second (x64) or second and third (x128) 64-character word; None where it does not fit."""
    if where == "start":
        return min(x for x in LENGTHS if x >= k), 0
    if where == "end":
        fits = [x for x in LENGTHS if x >= k + 7]
        return (fits[0], fits[0] - k) if fits else None
    at = 60 if where == "x64" else 120
    fits = [x for x in LENGTHS if x >= at + k]
    return (fits[0], at) if fits and k >= 9 else None


def _plants():
    """(b index, a index, k, b length, b offset, a length, a offset, breaker): every stretch length three times --
    whole, broken by an N in its middle, broken by a lower-case letter --, the places cycling so that every length
    meets starts, ends and word borders on one side or the other; indices spread over the three tiles of each list."""
    places = ("start", "end", "x64", "x128")
    out = []
    t = 0
    for k in STRETCHES:
        for breaker in (None, "N", "g"):
            pb = _place(k, places[t % 4]) or _place(k, "end") or _place(k, "start")
            pa = _place(k, places[(t // 4 + t + 1) % 4]) or _place(k, "start")
            out.append(((7 * t + 3) % N, (11 * t + 5) % N, k, pb[0], pb[1], pa[0], pa[1], breaker))
            t += 1
    # and one that fills two words exactly on both sides (64 and 256 do so in the cycle above)
    out.append(((7 * t + 3) % N, (11 * t + 5) % N, 128, 128, 0, 128, 0, None))
    return out


def _master():
    """Two lists of 130 records, B and A, and run(b_i, a_j) for all of them (the model, computed once): lengths mixed
    from LENGTHS, 5 % N and some lower case, and the stretches of _plants between B and A."""
    if "m" not in _shared:
        cd = _cd()
        rng = np.random.default_rng(20261022)
        plants = _plants()
        short = [x for x in LENGTHS if x <= 65]
        alphabet = list("ACGT") * 23 + ["N"] * 5 + ["a", "c", "g"]
        lens_b = [int(rng.choice(short)) for _ in range(N)]
        lens_a = [int(rng.choice(short)) for _ in range(N)]
        for i, n in ((0, 129), (1, 255), (2, 127), (4, 100)):
            lens_b[i] = n
        for i, n in ((0, 128), (2, 256), (3, 100), (4, 127), (6, 129)):
            lens_a[i] = n
        for bi, aj, _k, lb, _ob, la, _oa, _br in plants:
            lens_b[bi], lens_a[aj] = lb, la
        assert set(lens_b) | set(lens_a) == set(LENGTHS)
        assert len({p[0] for p in plants}) == len({p[1] for p in plants}) == len(plants) == 31
        bs = [_random(rng, n, alphabet) for n in lens_b]
        as_ = [_random(rng, n, alphabet) for n in lens_a]
        for bi, aj, k, _lb, ob, _la, oa, breaker in plants:
            piece = _random(rng, k)
            mine = piece if breaker is None else piece[:k // 2] + breaker + piece[k // 2 + 1:]
            bs[bi] = bs[bi][:ob] + mine + bs[bi][ob + k:]
            as_[aj] = as_[aj][:oa] + _rc(piece) + as_[aj][oa + k:]
        assert [len(s) for s in bs] == lens_b and [len(s) for s in as_] == lens_a
        m = _matrix(bs, as_)
        # the model against the quantifiers: a sample of pairs of short records, and what the plants say
        for _ in range(60):
            i, j = int(rng.integers(N)), int(rng.integers(N))
            if len(bs[i]) <= 65 and len(as_[j]) <= 65:
                assert m[i, j] == cd.run(bs[i], as_[j]), (i, j)
        for bi, aj, k, _lb, _ob, _la, _oa, breaker in plants:
            if breaker is None:
                assert m[bi, aj] >= k
            elif k > 40:
                # a broken stretch: the longer half, which the flanks may lengthen by chance, and never the whole
                assert max(k // 2, k - k // 2 - 1) <= m[bi, aj] < k - 10, (k, breaker)
        _shared["m"] = (bs, as_, m)
    return _shared["m"]


def _of_matrix(m):
    """(values, partners) of a block of the run matrix."""
    if m.shape[1] == 0:
        return np.zeros(m.shape[0], np.int32), np.full(m.shape[0], -1, np.int32)
    values = m.max(axis=1)
    return values, np.where(values > 0, m.argmax(axis=1), -1)


# ------------------------------------------------------------------ without a GPU
def test_third_header_third_table_and_the_two_headers_before_it():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib
    new = {"catchhip_cross_against", "catchhip_cross_against_flags", "catchhip_rows_drop_sets"}
    hdr = open(os.path.join(REPO, "include", "catchhip_redesign.h")).read()
    declared = set(re.findall(r"\b(catchhip_[a-z0-9_]+)\s*\(", hdr))
    assert declared == new == set(_lib.REDESIGN_PROTOTYPES)
    assert '#include "catchhip.h"' in hdr
    assert not new & set(_lib.PROTOTYPES) and not new & set(_lib.CROSS_PROTOTYPES)
    for other in ("catchhip.h", "catchhip_cross.h"):
        text = open(os.path.join(REPO, "include", other)).read()
        assert not any(name in text for name in new), other
        assert "cross_against" not in text and "drop_sets" not in text, other
    L = _lib.lib()
    for name, (res, args) in _lib.REDESIGN_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.catchhip_abi_version() == 2


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
def test_definition_numpy_form_and_device_on_small_lists(ctx):
    """cross_against from the quantifiers is the oracle: the NumPy form and both entries give what it gives."""
    from catch_amd import engine
    cd = _cd()
    rng = np.random.default_rng(17)
    assert cd.cross_against("ACGT", []) == (0, -1)
    assert cd.cross_against("ACGT", ["ACGT", "ACGT"]) == (4, 0)
    assert cd.cross_against("AAAA", ["AAAA", "CCTT", "TTTT", "TTTT"]) == (4, 2)
    assert cd.cross_against("NNNN", ["ACGT"]) == (0, -1)
    assert cd.conflicts_with("AAAA", ["TTTT"], 3) and not cd.conflicts_with("AAAA", ["TTTT"], 4)
    for _ in range(3):
        bs = [_random(rng, int(rng.integers(0, 41)), "ACGTNa-") for _ in range(14)]
        as_ = [_random(rng, int(rng.integers(0, 41)), "ACGTNa-") for _ in range(9)]
        piece = _random(rng, 13)
        bs[4] = (bs[4] + piece)[-40:]
        as_[6] = (_rc(piece) + as_[6])[:40]
        as_[8] = as_[6]                                        # the same record again: the smaller index is the partner
        bs[9] = as_[2]                                         # a record of B that is a record of A
        want = [cd.cross_against(b, as_) for b in bs]
        assert want[4] == (max(13, want[4][0]), 6) and want[9][0] >= cd.run(as_[2], as_[2])
        got_v, got_p = cd.cross_against_numpy(bs, as_)
        assert got_v.dtype == got_p.dtype == np.int32
        assert list(zip(got_v.tolist(), got_p.tolist())) == want
        dev_v, dev_p = engine.cross_against(ctx, bs, as_)
        assert dev_v.dtype == dev_p.dtype == np.int32
        assert list(zip(dev_v.tolist(), dev_p.tolist())) == want
        for above in (1, 5, 12, 13):
            flags = engine.cross_against_flags(ctx, bs, as_, above)
            assert flags.dtype == bool and flags.tolist() == [cd.conflicts_with(b, as_, above) for b in bs]
        assert cd.measure_against(bs, as_)[0].tolist() == [v for v, _p in want]
        assert cd.flags_against(bs, as_, 12).tolist() == [v > 12 for v, _p in want]


@pytest.mark.gpu
@pytest.mark.parametrize("nb", SIZES)
def test_device_equals_the_model_at_the_tile_edges_of_both_lists(ctx, nb):
    from catch_amd import engine
    bs, as_, m = _master()
    for na in SIZES:
        want_v, want_p = _of_matrix(m[:nb, :na])
        values, partners = engine.cross_against(ctx, bs[:nb], as_[:na])
        assert values.shape == partners.shape == (nb,)
        wrong = [(i, int(values[i]), int(partners[i]), int(want_v[i]), int(want_p[i])) for i in range(nb)
                 if values[i] != want_v[i] or partners[i] != want_p[i]]
        assert not wrong, (na, wrong[:10])
        flags = engine.cross_against_flags(ctx, bs[:nb], as_[:na], 20)
        assert flags.tolist() == (want_v > 20).tolist(), na
        # the same calls again: the same bytes
        again = engine.cross_against(ctx, bs[:nb], as_[:na])
        assert again[0].tobytes() == values.tobytes() and again[1].tobytes() == partners.tobytes()
        assert engine.cross_against_flags(ctx, bs[:nb], as_[:na], 20).tobytes() == flags.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("longest", [64, 128, 256])
def test_every_word_count_of_the_planes_and_the_numpy_form(ctx, longest):
    """Lists of records of at most 64, 128 and 256 characters: W = 1, 2 and 4."""
    from catch_amd import engine
    cd = _cd()
    bs, as_, m = _master()
    bi = [i for i, s in enumerate(bs) if len(s) <= longest]
    ai = [j for j, s in enumerate(as_) if len(s) <= longest]
    assert max(len(bs[i]) for i in bi) == longest == max(len(as_[j]) for j in ai)
    want_v, want_p = _of_matrix(m[np.ix_(bi, ai)])
    assert int(want_v.max()) == longest          # the stretch of 64, 128 or 256 characters, start to end
    values, partners = engine.cross_against(ctx, [bs[i] for i in bi], [as_[j] for j in ai])
    assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist()
    got_v, got_p = cd.cross_against_numpy([bs[i] for i in bi], [as_[j] for j in ai])
    assert got_v.tolist() == want_v.tolist() and got_p.tolist() == want_p.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("above", THRESHOLDS)
def test_flags_are_the_values_above_the_threshold(ctx, above):
    from catch_amd import engine
    bs, as_, m = _master()
    for nb, na in ((N, N), (65, 63), (64, 130)):
        want = _of_matrix(m[:nb, :na])[0] > above
        flags = engine.cross_against_flags(ctx, bs[:nb], as_[:na], above)
        assert flags.tolist() == want.tolist(), (nb, na)
    if above == 256:
        assert not want.any()
    if above == 255:
        assert int(want.sum()) == 1               # the one whole stretch of 256


@pytest.mark.gpu
def test_partner_rules(ctx):
    from catch_amd import engine
    cd = _cd()
    rng = np.random.default_rng(8)
    s = _random(rng, 100)
    others = [_random(rng, 100) for _ in range(140)]
    # the reverse complement of s at two indices of A, in different tiles: the smaller one is the partner
    as_ = others[:70] + [_rc(s)] + others[70:128] + [_rc(s)] + others[128:]
    assert [j for j, a in enumerate(as_) if a == _rc(s)] == [70, 129]
    values, partners = engine.cross_against(ctx, [others[3], s, s], as_)
    assert values.tolist()[1:] == [100, 100] and partners.tolist()[1:] == [70, 70]
    # others[3] is a record of A: its value is at least run with itself, nothing is exempted
    want_v, want_p = cd.cross_against_numpy([others[3]], as_)
    assert (int(values[0]), int(partners[0])) == (int(want_v[0]), int(want_p[0]))
    assert int(values[0]) >= cd.run(others[3], others[3]) > 0
    # (ACGT) x 25 is its own reverse complement: against a list that holds it, the value is run(b, b) = 100
    own = "ACGT" * 25
    assert cd.run(own, own) == 100
    values, partners = engine.cross_against(ctx, [own], others[:9] + [own])
    assert values.tolist() == [100] and partners.tolist() == [9]
    assert engine.cross_against_flags(ctx, [own], others[:9] + [own], 99).tolist() == [True]
    assert engine.cross_against_flags(ctx, [own], others[:9] + [own], 100).tolist() == [False]


@pytest.mark.gpu
def test_refusals_and_empty_lists(ctx):
    from catch_amd import engine
    rng = np.random.default_rng(2)
    long = _random(rng, 257)
    ok = [_random(rng, 40), _random(rng, 64)]
    for bs, as_ in (([ok[0], long], ok), (ok, [long, ok[1]])):
        with pytest.raises(ValueError, match="257 characters.*at most 256"):
            engine.cross_against(ctx, bs, as_)
        with pytest.raises(ValueError, match="257 characters.*at most 256"):
            engine.cross_against_flags(ctx, bs, as_, 20)
    for above in (0, -1):
        with pytest.raises(ValueError, match="at least 1"):
            engine.cross_against_flags(ctx, ok, ok, above)
    # 256 is taken
    values, partners = engine.cross_against(ctx, [long[:256]], [ok[0], _rc(long[:256])])
    assert values.tolist() == [256] and partners.tolist() == [1]
    # an empty list on either side
    v, p = engine.cross_against(ctx, ok, [])
    assert v.tolist() == [0, 0] and p.tolist() == [-1, -1]
    assert engine.cross_against_flags(ctx, ok, [], 5).tolist() == [False, False]
    v, p = engine.cross_against(ctx, [], ok)
    assert v.size == p.size == 0 and engine.cross_against_flags(ctx, [], ok, 5).size == 0
    # more records than a call takes: refused from the sizes alone (the offsets say 2^30 + 1 empty records)
    n = (1 << 30) + 1
    buf = np.zeros(1, dtype=np.uint8)
    off = np.zeros(2, dtype=np.int64)
    out = np.zeros(1, dtype=np.int32)
    u8p, i64p, i32p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int64, ctypes.c_int32))
    rc = ctx._L.catchhip_cross_against(ctx._h, buf.ctypes.data_as(u8p), off.ctypes.data_as(i64p), 1,
                                       buf.ctypes.data_as(u8p), off.ctypes.data_as(i64p), n,
                                       out.ctypes.data_as(i32p), out.ctypes.data_as(i32p))
    assert rc == -1 and b"1073741824" in ctx._L.catchhip_last_error()


@pytest.mark.gpu
def test_the_three_entries_on_poisoned_memory(ctx, monkeypatch):
    from catch_amd import engine
    bs, as_, m = _master()
    want_v, want_p = _of_matrix(m)
    drop = np.arange(6) % 2 == 1
    outs = {}
    for poison in (None, 255, 85):
        # (set before the context is created: its first blocks are poisoned too)
        if poison is None:
            monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
        else:
            monkeypatch.setenv("CATCHHIP_POOL_POISON", str(poison))
        c = engine.Context(ctx.device)
        try:
            values, partners = engine.cross_against(c, bs, as_)
            flags = engine.cross_against_flags(c, bs, as_, 20)
            rows = engine.Rows.from_host(c, [0, 1, 1, 3, 4, 5], [0, 0, 1, 0, 1, 1], [0, 5, 2, 40, 0, 30],
                                         [10, 25, 9, 90, 20, 31], [100, 50])
            try:
                left = rows.drop_sets(6, drop)
                try:
                    fetched = left.fetch()
                    gain0, longest, picks = left.fetch_gain0(6), left.longest(), left.greedy(6)
                finally:
                    left.close()
            finally:
                rows.close()
        finally:
            c.close()
        assert values.tolist() == want_v.tolist() and partners.tolist() == want_p.tolist(), poison
        assert flags.tolist() == (want_v > 20).tolist(), poison
        assert [x.tolist() for x in fetched] == [[0, 4], [0, 1], [0, 0], [10, 20]], poison
        assert gain0.tolist() == [10, 0, 0, 0, 20, 0] and longest == 20 and picks == [4, 0], poison
        outs[poison] = (values.tobytes(), partners.tobytes(), flags.tobytes()) + tuple(x.tobytes() for x in fetched)
    monkeypatch.delenv("CATCHHIP_POOL_POISON", raising=False)
    assert outs[None] == outs[255] == outs[85]


@pytest.mark.gpu
def test_probe_report_against_a_panel(ctx, tmp_path, monkeypatch, capsys):
    """--cross-dimer-against: two columns behind cross_partner or where it would stand, the rule cross-against under
    --max-cross-dimer, the same bytes on the device and on the host path, and no change without the option."""
    from catch_amd import probe_report
    cd = _cd()
    new = ["GATTACAGATTACCAGGTCA", "AAAAAAAA", "NNNN", "ACGTTGCA" * 5]
    panel = ["CCCC", "TTTTTGGTAATCTGTTTTTT", "TTTTTGGTAATCTGTTTTTT", "ACGTTGCA" * 5]
    want = [cd.cross_against(b, panel) for b in new]
    assert [v for v, _p in want] == [11, 6, 0, 36] and [p for _v, p in want] == [1, 1, -1, 3]
    fa, pa = str(tmp_path / "new.fasta"), str(tmp_path / "panel.fasta")
    for path, seqs in ((fa, new), (pa, panel)):
        with open(path, "w") as f:
            f.write("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    texts = {}
    for host in (False, True):
        if host:
            monkeypatch.setenv("CATCHHIP_HOST_FRONT_END", "1")
        for name, more in (("plain", []), ("against", ["--cross-dimer-against", pa]),
                           ("both", ["--cross-dimer", "--cross-dimer-against", pa]),
                           ("judged", ["--cross-dimer-against", pa, "--max-cross-dimer", "10"]),
                           ("alone", ["--max-cross-dimer", "10"])):
            out = str(tmp_path / ("%s_%d.tsv" % (name, host)))
            failed = probe_report.main(probe_report.parse_args(["-f", fa, "-o", out] + more))
            texts[name, host] = open(out).read()
            if name == "judged":
                assert failed == [["cross-against"], [], [], ["cross-against"]]
    capsys.readouterr()
    assert all(texts[name, False] == texts[name, True] for name, _h in texts)
    rows = {name: [line.split("\t") for line in texts[name, False].splitlines()] for name, _h in texts}
    cols = [[str(v), "NA" if p < 0 else str(p + 1)] for v, p in want]
    assert rows["against"][0][-3:] == ["background_hits", "cross_against", "cross_against_partner"]
    assert [r[:-2] for r in rows["against"]] == rows["plain"] and [r[-2:] for r in rows["against"][1:]] == cols
    assert rows["both"][0][-4:] == ["cross_dimer", "cross_partner", "cross_against", "cross_against_partner"]
    assert [r[-2:] for r in rows["both"][1:]] == cols
    assert rows["judged"][0][-5:] == ["cross_dimer", "cross_partner", "cross_against", "cross_against_partner", "verdict"]
    assert [r[-3:-1] for r in rows["judged"][1:]] == cols
    assert [r[-1] for r in rows["judged"][1:]] == ["cross-against", "ok", "ok", "cross-against"]
    # without the option the report is what it was
    assert rows["alone"][0][-3:] == ["cross_dimer", "cross_partner", "verdict"]
    assert [r[:len(rows["alone"][0]) - 1] for r in rows["judged"]] == [r[:-1] for r in rows["alone"]]
