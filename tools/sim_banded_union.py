"""Design aid (not product code): gain bands on a UNION of S4's small groups, on the CPU (DESIGN.md section 4 K2,
"Gain bands"; the model of the rounds is tools/sim_banded_rounds.py's).

    python tools/sim_banded_union.py [scale] [ratio]

The groups that bench.py solves as one instance (those below 16 Mbases x scale) are laid side by side and solved with
one band, with 2 bands cut by the INSTANCE's largest round-0 gain, and with 2 bands cut group by group -- every group
by its own largest gain -- under one level for the whole instance: a round of level L streams the bands <= L, a set
claims when its gain reaches its own group's boundary of L, a round without a claimant raises L.  Printed per
configuration: rounds, record visits per row (count + claim launches), and whether every group's picks, in pick
order, are the sequential greedy's of that group alone."""
import sys

import numpy as np

sys.path.insert(0, ".")
from oracle import oracle  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402
from tools.sim_banded_rounds import rows_of, simulate, union  # noqa: E402


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.03
    ratio = float(sys.argv[2]) if len(sys.argv) > 2 else 0.65
    groups = synthetic.dataset("S4", scale=scale)
    bases = [sum(len(s) for g in grp for s in g) for grp in groups]
    small = [i for i in range(len(groups)) if bases[i] < 16e6 * scale]
    parts = [rows_of(groups[i]) for i in small]
    sid, gs, ge, ns, tot, grp = union(parts)
    # the sequential greedy of every group alone, ids moved to the union's numbering
    want, first = [], 0
    for s, un, a, b, n, t, _ in parts:
        exp = oracle.approx_multiuniverse(s, np.zeros(len(s), dtype=np.int64), a, b, n, 1, None, None, None)
        want.append([int(x) + first for x in exp])
        first += n
    print("union of S4 x %g groups %s: rows %d sets %d bases %d, gains' maxima per group %s" % (
        scale, small, len(sid), ns, tot,
        [int(np.bincount(s, weights=b - a).max()) for s, _, a, b, _, _, _ in parts]))
    print("  %-34s %6s %6s %15s %s" % ("bands (boundaries by)", "rounds", "levels", "visits per row", "picks per group"))
    for name, nbands, by in (("1", 1, None), ("2 x %.2f (instance)" % ratio, 2, None), ("2 x %.2f (group)" % ratio, 2, grp)):
        r = simulate(sid, gs, ge, ns, tot, nbands, ratio, by)
        picks = np.asarray(r["picks"], dtype=np.int64)
        ok = all([int(x) for x in picks[grp[picks] == g]] == want[g] for g in range(len(parts)))
        print("  %-34s %6d %6d %15.2f %s" % (name, r["rounds"], r["levels"], r["count_visits"] + r["claim_visits"],
                                          "sequential" if ok else "DIFFER"))


if __name__ == "__main__":
    main()
