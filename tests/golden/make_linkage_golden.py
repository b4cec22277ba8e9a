#!/usr/bin/env python3
"""tests/golden/linkage.json.gz: average-linkage cases recorded from SciPy
(scipy.cluster.hierarchy.linkage(method="average") + fcluster(criterion=
"distance")), for tests/test_linkage.py.

    python tests/golden/make_linkage_golden.py

Needs SciPy and NumPy only.  Every case holds
  * the float32 condensed matrix: small integer codes + the lut they index
    (kind "codes", one byte each), or the float32 values themselves (kind
    "f32", little-endian), xz-compressed and base64-encoded;
  * `unsorted`: the n - 1 merges (x, y, height, size) in the order the
    nearest-neighbour chain makes them -- from the model below, which restates
    SciPy's nn_chain for `average`; the generator refuses to write a case whose
    sorted and relabelled merges are not bit for bit SciPy's linkage matrix;
  * `Z`: SciPy's linkage matrix, heights as float.hex();
  * thresholds (float.hex()) and, per threshold, the clusters in the order
    cluster.cluster_hierarchically_from_dist_matrix returns them.
"""
import base64
import gzip
import json
import lzma
import os
import sys
from collections import defaultdict
from fractions import Fraction

import numpy as np
import scipy
from scipy.cluster import hierarchy

HERE = os.path.dirname(os.path.abspath(__file__))
WORKGROUP = 1024        # threads of linkage_nn_chain_kernel (catch_amd/csrc/linkage.hip: LK_THREADS)


def square_from_condensed(cond, n):
    D = np.full((n, n), np.inf, dtype=np.float64)
    iu = np.triu_indices(n, 1)
    D[iu] = cond.astype(np.float64)
    D[(iu[1], iu[0])] = D[iu]
    return D


def nn_chain_average(D, average=None):
    """SciPy's nn_chain for method="average" (_hierarchy.pyx) over a full square float64 matrix with +inf on the
    diagonal; dead clusters' rows and columns are set to +inf, so np.argmin (first occurrence = lowest index) is
    the scan.  Returns the merges in production order.  average(nx, a, ny, b): the update of one entry (default:
    NumPy's separately rounded (nx * a + ny * b) / (nx + ny))."""
    n = D.shape[0]
    D = D.copy()
    size = np.ones(n, dtype=np.int64)
    chain = []
    out = []
    for _ in range(n - 1):
        if not chain:
            chain.append(int(np.nonzero(size > 0)[0][0]))
        while True:
            x = chain[-1]
            i = int(np.argmin(D[x]))
            cur, y = D[x, i], i
            if len(chain) > 1 and D[x, chain[-2]] <= cur:       # only a strictly smaller distance replaces it
                y, cur = chain[-2], D[x, chain[-2]]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        chain.pop()
        chain.pop()
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        out.append((x, y, float(cur), nx + ny))
        size[x], size[y] = 0, nx + ny
        live = size > 0
        live[y] = False
        if average is None:
            new = (nx * D[x, live] + ny * D[y, live]) / (nx + ny)
        else:
            new = np.array([average(nx, a, ny, b) for a, b in zip(D[x, live].tolist(), D[y, live].tolist())])
        D[y, live] = new
        D[live, y] = new
        D[x, :] = np.inf
        D[:, x] = np.inf
    return out


def sort_and_relabel(merges, n):
    """linkage()'s tail: stable sort by height, union-find relabelling."""
    order = sorted(range(len(merges)), key=lambda k: merges[k][2])      # (sorted() is stable)
    parent = list(range(2 * n - 1))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    count = [1] * (2 * n - 1)
    Z = []
    for k, m in enumerate(order):
        a, b = sorted((find(merges[m][0]), find(merges[m][1])))
        parent[a] = parent[b] = n + k
        count[n + k] = count[a] + count[b]
        Z.append((a, b, merges[m][2], count[n + k]))
    return Z


def clusters_at(Z, threshold):
    """cluster.cluster_hierarchically_from_dist_matrix, after its linkage call."""
    labels = hierarchy.fcluster(Z, threshold, criterion="distance")
    members = defaultdict(list)
    for i, c in enumerate(labels):
        members[int(c)].append(i)
    numbers = list(range(min(members), max(members) + 1))
    numbers.sort(key=lambda c: len(members[c]), reverse=True)
    return [members[c] for c in numbers]


def pack_bytes(raw):
    """base64 of the xz-compressed bytes (the rows of a 2,500-point matrix repeat beyond gzip's 32-KB window)"""
    return base64.b64encode(lzma.compress(raw, preset=9)).decode()


def pack_merges(rows):
    return dict(a=[int(r[0]) for r in rows], b=[int(r[1]) for r in rows], h=[float(r[2]).hex() for r in rows],
                s=[int(r[3]) for r in rows])


def record(name, n, cond, thresholds=None, codes=None, lut=None, average=None):
    cond = np.ascontiguousarray(cond, dtype=np.float32)
    assert cond.size == n * (n - 1) // 2 and np.isfinite(cond).all()
    case = dict(name=name, n=n)
    if codes is not None:
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert (lut[codes] == cond).all()
        case.update(kind="codes", lut=[float(v).hex() for v in lut], data=pack_bytes(codes.tobytes()))
    else:
        case.update(kind="f32", data=pack_bytes(cond.astype("<f4").tobytes()))
    if n == 1:
        case.update(unsorted=pack_merges([]), Z=pack_merges([]), thresholds=[(0.5).hex()], clusters=[[[0]]])
        return case
    Zs = hierarchy.linkage(cond, method="average")
    merges = nn_chain_average(square_from_condensed(cond, n))
    mine = sort_and_relabel(merges, n)
    same = all(a == int(z[0]) and b == int(z[1]) and h.hex() == float(z[2]).hex() and s == int(z[3])
               for (a, b, h, s), z in zip(mine, Zs))
    if not same:
        raise SystemExit("%s: the model's merges are not SciPy's linkage matrix" % name)
    if average is not None:
        # what a contracted update would give: must differ, or the case proves nothing
        for form, fn in average.items():
            other = sort_and_relabel(nn_chain_average(square_from_condensed(cond, n), fn), n)
            if [m[2].hex() for m in other] == [m[2].hex() for m in mine]:
                raise SystemExit("%s: %s gives the same heights" % (name, form))
    heights = sorted(set(float(z[2]) for z in Zs))
    if thresholds is None:
        lo, hi = heights[0], heights[-1]
        thresholds = [np.nextafter(lo, -np.inf) if lo > 0 else -1.0, lo, heights[len(heights) // 2],
                      float(np.nextafter(heights[len(heights) // 2], np.inf)), hi, hi + 1.0]
    thresholds = [float(t) for t in thresholds]
    case.update(unsorted=pack_merges(merges), Z=pack_merges(Zs), thresholds=[t.hex() for t in thresholds],
                clusters=[clusters_at(Zs, t) for t in thresholds])
    print("%-22s n=%5d heights %5d  clusters %s" % (name, n, len(heights), [len(c) for c in case["clusters"]]), flush=True)
    return case


def lut_of(N):
    """the product's lut: float32(1 - c / N), c = 0 .. N (catch_amd/utils/cluster.py)"""
    return (1.0 - np.arange(N + 1, dtype=np.float64) / float(N)).astype(np.float32)


def block_codes(rng, n, groups, noise, shuffled=True):
    """101-value codes with block structure: groups of related points (many common values, a few levels), unrelated
    groups share 0-3 values; `noise` of the entries move by one."""
    g = rng.integers(0, groups, size=n)
    if not shuffled:
        g.sort()
    base = rng.integers(0, 4, size=(groups, groups))
    base = np.minimum(base, base.T)
    base[np.arange(groups), np.arange(groups)] = rng.integers(60, 96, size=groups)
    iu = np.triu_indices(n, 1)
    codes = base[g[iu[0]], g[iu[1]]]
    flip = rng.random(codes.size) < noise
    codes = np.where(flip, codes + rng.integers(-1, 2, size=codes.size), codes)
    return np.clip(codes, 0, 100).astype(np.uint8)


def fused_a(nx, a, ny, b):
    """fma(nx, a, ny * b) / (nx + ny): the sum of the first product, exact, and the rounded second one"""
    if np.isinf(a) or np.isinf(b):
        return float("inf")
    return float(Fraction(nx) * Fraction(a) + Fraction(float(ny) * b)) / (nx + ny)


def fused_b(nx, a, ny, b):
    if np.isinf(a) or np.isinf(b):
        return float("inf")
    return float(Fraction(float(nx) * a) + Fraction(ny) * Fraction(b)) / (nx + ny)


def contraction_case():
    """A small random float32 matrix whose heights change in the last bit when either product of the update is
    fused into the sum."""
    rng = np.random.default_rng(2718)
    for attempt in range(10000):
        n = 9
        cond = rng.random(n * (n - 1) // 2, dtype=np.float32) + np.float32(0.25)
        sq = square_from_condensed(cond, n)
        ref = [m[2].hex() for m in sort_and_relabel(nn_chain_average(sq), n)]
        if all([m[2].hex() for m in sort_and_relabel(nn_chain_average(sq, fn), n)] != ref for fn in (fused_a, fused_b)):
            print("contraction case: attempt", attempt, flush=True)
            return record("contraction", n, cond, average={"fma(nx, a, ny * b)": fused_a, "fma(ny, b, nx * a)": fused_b})
    raise SystemExit("no contraction case found")


def main():
    rng = np.random.default_rng(20260)
    lut100, lut4 = lut_of(100), lut_of(4)
    cases = []
    # sizes where the reduction and the strides can go wrong
    for n in (1, 2, 3, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 2500):
        if n <= 65:
            codes = rng.integers(40, 60, size=n * (n - 1) // 2).astype(np.uint8)
        else:
            codes = block_codes(rng, n, groups=max(6, n // 90), noise=0.004)
        cases.append(record("size_%d" % n, n, lut100[codes], codes=codes, lut=lut100))
    # tie regimes
    n = 200
    m = n * (n - 1) // 2
    codes = np.full(m, 37, dtype=np.uint8)
    cases.append(record("all_equal", n, lut100[codes], codes=codes, lut=lut100))
    codes = rng.integers(0, 5, size=m).astype(np.uint8)
    cases.append(record("five_values", n, lut4[codes], codes=codes, lut=lut4))
    codes = block_codes(rng, 203, groups=7, noise=0.05)
    cases.append(record("blocks_101", 203, lut100[codes], codes=codes, lut=lut100))
    # points on a line with strictly shrinking gaps: the chain grows to n before the first merge
    gaps = np.arange(2 * n, n + 1, -1, dtype=np.int64)[:n - 1]
    pos = np.concatenate([[0], np.cumsum(gaps)])
    iu = np.triu_indices(n, 1)
    cases.append(record("long_chain", n, (pos[iu[1]] - pos[iu[0]]).astype(np.float32)))
    first = nn_chain_average(square_from_condensed((pos[iu[1]] - pos[iu[0]]).astype(np.float32), n))[0]
    assert (first[0], first[1]) == (n - 2, n - 1)
    vals = ((rng.permutation(1 << 22)[:197 * 196 // 2] + 1) / float(1 << 22)).astype(np.float32)      # distinct: no ties
    assert np.unique(vals).size == vals.size
    cases.append(record("random_f32", 197, vals))
    cases.append(contraction_case())
    out = dict(python=sys.version.split()[0], scipy=scipy.__version__, numpy=np.__version__, workgroup=WORKGROUP,
               cases=cases)
    path = os.path.join(HERE, "linkage.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
