"""Design aid (not product code): the frontier rounds of the row-parallel set-cover solver with GAIN BANDS, on the
CPU, over the oracle's rows of a scaled S4 group and of a union of small S4 groups.

    python tools/sim_banded_rounds.py [scale] [group | "union"]

The model follows setcover_flat.inc launch by launch: the count launch of a round streams the records of the awake
bands that were alive at the count before (a band that wakes: all its records), the claim launch those that are alive
now; a set claims when its gain reaches the level's boundary, a claimant is accepted when it holds the largest key on
every 64-base word in which it has uncovered bases, a round without a claimant raises the level.  Reported per
configuration: rounds, levels, record visits of the count and of the claim launches per row, the rounds that stream
less than 2 % of the rows ("thin"), and whether the picks -- ordered by accept-time key -- are the sequential
greedy's.  bands = 1 is the solver without bands."""
import sys

import numpy as np

sys.path.insert(0, ".")
from oracle import oracle  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402
from tests.util import candidates  # noqa: E402


def rows_of(genomes):
    cand = candidates(genomes, 100, 50)
    k, entries = oracle.anchor_table(cand, 2, 100)
    uniq, owner = oracle._unique_last(cand)
    pr, un, st, en = oracle.make_sets(uniq, entries, k, genomes, 2, 100, 0, 50)
    sid = np.array(owner, dtype=np.int64)[pr]
    glen = np.array([sum(len(s) for s in g) for g in genomes])
    base = np.concatenate([[0], np.cumsum(glen)])
    return sid, np.asarray(un), base[un] + st, base[un] + en, len(cand), int(base[-1]), len(genomes)


def union(parts):
    """Independent instances side by side: sets and coordinates of each moved behind the one before."""
    sid, gs, ge, grp, ns, tot = [], [], [], [], 0, 0
    for g, (s, _, a, b, n, t, _) in enumerate(parts):
        sid.append(s + ns); gs.append(a + tot); ge.append(b + tot); grp.append(np.full(n, g))
        ns += n; tot += t
    return np.concatenate(sid), np.concatenate(gs), np.concatenate(ge), ns, tot, np.concatenate(grp)


def simulate(sid, gs, ge, nsets, total, nbands, ratio, group=None):
    """-> dict(rounds, levels, count_visits, claim_visits, thin, picks); group: per set, for boundaries relative to
    each group's own largest gain instead of the instance's."""
    nrows = len(sid)
    g0 = np.bincount(sid, weights=ge - gs, minlength=nsets).astype(np.int64)
    norm = np.full(nsets, g0.max(), dtype=np.float64)
    if group is not None:
        gmax = np.zeros(group.max() + 1)
        np.maximum.at(gmax, group, g0)
        norm = gmax[group]
    rel = g0 / np.maximum(norm, 1)
    thr_rel = [ratio ** (b + 1) for b in range(nbands - 1)] + [0.0]
    band = np.full(nsets, nbands - 1)
    for b in range(nbands - 2, -1, -1):
        band[rel >= thr_rel[b]] = b
    # (row, word) pairs
    w0, w1 = gs >> 6, (ge - 1) >> 6
    nw = w1 - w0 + 1
    prow = np.repeat(np.arange(nrows), nw)
    pw = np.concatenate([np.arange(a, b + 1) for a, b in zip(w0, w1)]) if nrows else np.zeros(0, np.int64)
    plo = np.maximum(gs[prow], pw << 6)
    phi = np.minimum(ge[prow], (pw + 1) << 6)
    unc = np.ones(total, dtype=bool)
    picked = np.zeros(nsets, dtype=bool)
    in_buf = np.zeros(nrows, dtype=bool)          # records the next count launch streams
    woke = np.zeros(nbands, dtype=bool)
    level, rounds, cvis, kvis, thin = 0, 0, 0, 0, 0
    picks = []
    ids = np.arange(nsets)
    while True:
        if not woke[level]:
            in_buf |= band[sid] == level
            woke[level] = True
        streamed = int(in_buf.sum())
        cs = np.concatenate([[0], np.cumsum(unc)])
        rc = cs[ge] - cs[gs]
        alive = in_buf & (rc > 0)
        in_buf = alive
        if rounds:
            cvis += streamed                     # (round 0 has no count launch: the gains came with the rows)
        kvis += int(alive.sum())
        if streamed < 0.02 * nrows:
            thin += 1
        rounds += 1
        gain = np.bincount(sid[alive], weights=rc[alive], minlength=nsets).astype(np.int64)
        t_l = np.maximum(1, np.floor(thr_rel[level] * norm)) if level + 1 < nbands else np.ones(nsets)
        claim = (gain >= t_l) & (gain > 0)
        if not claim.any():
            if level + 1 < nbands:
                level += 1
                continue
            break
        key = (gain << 32) | (0xFFFFFFFF - ids)
        pu = (cs[phi] - cs[plo]) > 0
        m = pu & alive[prow] & claim[sid[prow]]
        owner = np.zeros((total >> 6) + 2, dtype=np.int64)
        np.maximum.at(owner, pw[m], key[sid[prow[m]]])
        lost = np.zeros(nsets, dtype=bool)
        lm = m & (owner[pw] != key[sid[prow]])
        lost[sid[prow[lm]]] = True
        acc = claim & ~lost
        for i in np.nonzero(acc[sid] & alive)[0]:
            unc[gs[i]:ge[i]] = False
        picked |= acc
        picks += [(int(key[s]), int(s)) for s in np.nonzero(acc)[0]]
    picks.sort(reverse=True)
    return dict(rounds=rounds, levels=level + 1, count_visits=cvis / max(nrows, 1), claim_visits=kvis / max(nrows, 1),
                thin=thin, picks=[s for _, s in picks])


def report(name, sid, un, gs, ge, nsets, total, nuniv, group=None):
    exp = list(oracle.approx_multiuniverse(sid, un, gs, ge, nsets, 1, None, None, None))
    print("%s: rows %d sets %d bases %d picks %d" % (name, len(sid), nsets, total, len(exp)))
    print("  %-28s %6s %6s %12s %12s %5s %s" % ("bands x ratio (norm)", "rounds", "levels", "count visits", "claim visits", "thin", "order"))
    for norm in (["instance"] if group is None else ["instance", "group"]):
        for nbands, ratio in [(1, 0.75), (2, 0.75), (4, 0.75), (8, 0.75), (16, 0.75), (4, 0.5), (8, 0.5), (8, 0.85), (16, 0.85), (32, 0.85)]:
            if nbands == 1 and norm == "group":
                continue
            r = simulate(sid, gs, ge, nsets, total, nbands, ratio, group if norm == "group" else None)
            print("  %-28s %6d %6d %12.2f %12.2f %5d %s" % ("%d x %.2f (%s)" % (nbands, ratio, norm), r["rounds"], r["levels"],
                                                           r["count_visits"], r["claim_visits"], r["thin"],
                                                           "sequential" if r["picks"] == exp else "DIFFERS"))


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.05
    which = sys.argv[2] if len(sys.argv) > 2 else "0"
    groups = synthetic.dataset("S4", scale=scale)
    if which == "union":
        parts = [rows_of(g) for g in groups[1:6]]
        sid, gs, ge, ns, tot, grp = union(parts)
        report("union of S4 groups 1-5 x %g" % scale, sid, np.zeros(len(sid), dtype=np.int64), gs, ge, ns, tot, 1, grp)
    else:
        sid, un, gs, ge, ns, tot, nu = rows_of(groups[int(which)])
        report("S4 group %s x %g" % (which, scale), sid, np.zeros(len(sid), dtype=np.int64), gs, ge, ns, tot, 1)


if __name__ == "__main__":
    main()
