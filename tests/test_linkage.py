"""Average linkage on the device (catch_amd/csrc/linkage.hip) against SciPy.

The fixture tests/golden/linkage.json.gz (generator: tests/golden/make_linkage_golden.py) was recorded with SciPy:
float32 condensed matrices, the merges of the nearest-neighbour chain in production order, SciPy's linkage matrix
(heights as float.hex()) and the clusters of cluster.cluster_hierarchically_from_dist_matrix at several thresholds.
Where SciPy imports, the GPU tests also compare with the live routine on the same matrix.
"""
import base64
import ctypes
import lzma
import os
import random
import re

import numpy as np
import pytest

from util import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from scipy.cluster import hierarchy as _scipy_hierarchy
except ImportError:             # (the product path does not need it)
    _scipy_hierarchy = None

_golden = None
_cluster_golden = None


def _cases():
    global _golden
    if _golden is None:
        _golden = load_golden("linkage")
    return {c["name"]: c for c in _golden["cases"]}


def _matrix(case):
    raw = lzma.decompress(base64.b64decode(case["data"]))
    if case["kind"] == "codes":
        lut = np.array([float.fromhex(v) for v in case["lut"]], dtype=np.float32)
        dm = lut[np.frombuffer(raw, dtype=np.uint8)]
    else:
        dm = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    assert dm.size == case["n"] * (case["n"] - 1) // 2
    return dm


def _merge_rows(packed):
    return list(zip(packed["a"], packed["b"], packed["h"], packed["s"]))


def _rows_of(merges):
    return [(int(r[0]), int(r[1]), float(r[2]).hex(), int(r[3])) for r in np.asarray(merges).reshape(-1, 4)]


SIZE_CASES = ["size_1", "size_2", "size_3", "size_63", "size_64", "size_65", "size_1023", "size_1024", "size_1025",
              "size_2500"]
TIE_CASES = ["all_equal", "five_values", "blocks_101", "long_chain", "random_f32"]


def _check_case_on_device(ctx, name):
    from catch_amd.utils import cluster
    case = _cases()[name]
    dm = _matrix(case)
    thresholds = [float.fromhex(t) for t in case["thresholds"]]
    for k, (t, want) in enumerate(zip(thresholds, case["clusters"])):
        got, merges = cluster.cluster_hierarchically_on_device(dm, t, ctx=ctx, return_merges=True)
        assert got == want, (name, t)
        # the linkage matrix bit for bit: children, heights, sizes
        assert _rows_of(merges) == _merge_rows(case["Z"]), (name, t)
        # the live routine on the same matrix (all thresholds of a small case, two of a large one)
        if _scipy_hierarchy is not None and (case["n"] <= 300 or k in (1, 2)):
            assert got == cluster.cluster_hierarchically_from_dist_matrix(dm, t), (name, t)
    if _scipy_hierarchy is not None and case["n"] > 1:
        assert _rows_of(_scipy_hierarchy.linkage(dm, method="average")) == _merge_rows(case["Z"])


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", SIZE_CASES)
def test_sizes_around_the_reduction_and_the_strides(ctx, name):
    """n = 1, 2, 3, around a wavefront, one below / at / one above the workgroup size of linkage_nn_chain_kernel, and
    2,500 (several strides per lane): the clusters in order and the merges bit-equal."""
    _check_case_on_device(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIE_CASES)
def test_tie_regimes(ctx, name):
    """All distances equal, a 5-value lut, the 101-value lut with block structure, a chain that grows to n before the
    first merge, and float32 values without ties; thresholds below every height, above every height and exactly
    equal to one."""
    case = _cases()[name]
    heights = sorted(set(float.fromhex(h) for h in case["Z"]["h"]))
    ts = [float.fromhex(t) for t in case["thresholds"]]
    assert min(ts) < heights[0] and max(ts) > heights[-1] and any(t in heights for t in ts)
    if name == "long_chain":
        u = case["unsorted"]
        assert (u["a"][0], u["b"][0]) == (case["n"] - 2, case["n"] - 1)     # the chain reached the last point first
    if name == "random_f32":
        assert len(heights) == case["n"] - 1
    _check_case_on_device(ctx, name)


@pytest.mark.gpu
def test_update_is_not_contracted(ctx):
    """(nx * a + ny * b) / (nx + ny) with the products and the sum rounded one by one: the fixture's case changes its
    heights in the last bit under either fused form (the generator checks that), so they must match bit for bit."""
    _check_case_on_device(ctx, "contraction")


def _hierarchical_records():
    global _cluster_golden
    if _cluster_golden is None:
        _cluster_golden = load_golden("cluster")
    g = _cluster_golden
    recs = [c for c in g["from_reference_tests"]["minhash"] + g["synthetic"] if c["method"] == "hierarchical"]
    return g, recs


@pytest.mark.gpu
def test_from_signatures_both_paths(ctx, monkeypatch):
    """The hierarchical records of tests/golden/cluster.json.gz through cluster_with_minhash_signatures: the recorded
    clusters on the device path, on the host path (CATCHHIP_CLUSTER_HOST_LINKAGE) and with the size limit lowered
    (CATCHHIP_LINKAGE_MAX_N); the reference's own test inputs through Signatures.linkage_clusters."""
    from catch_amd.utils import cluster, lsh
    g, recs = _hierarchical_records()
    seeded = [c for c in recs if "seed" in c]
    assert len(seeded) >= 3 and any(len(c["seqs"]) > 8 for c in seeded)

    def run(c):
        random.seed(c["seed"])
        return cluster.cluster_with_minhash_signatures(dict(zip(c["names"], c["seqs"])), k=c["k"], N=c["N"],
                                                       threshold=c["threshold"], cluster_method=c["method"])
    for c in seeded:
        monkeypatch.delenv("CATCHHIP_CLUSTER_HOST_LINKAGE", raising=False)
        monkeypatch.delenv("CATCHHIP_LINKAGE_MAX_N", raising=False)
        assert run(c) == c["out"]
        assert cluster.last_timings["linkage"] == "device" and cluster.last_timings["linkage_s"] >= 0.0
        monkeypatch.setenv("CATCHHIP_LINKAGE_MAX_N", "1000000")
        assert run(c) == c["out"] and cluster.last_timings["linkage"] == "device"
        if len(c["seqs"]) > 8:
            monkeypatch.setenv("CATCHHIP_LINKAGE_MAX_N", "8")
            assert run(c) == c["out"] and cluster.last_timings["linkage"] == "host"
        monkeypatch.delenv("CATCHHIP_LINKAGE_MAX_N")
        monkeypatch.setenv("CATCHHIP_CLUSTER_HOST_LINKAGE", "1")
        assert run(c) == c["out"] and cluster.last_timings["linkage"] == "host"
    monkeypatch.delenv("CATCHHIP_CLUSTER_HOST_LINKAGE", raising=False)
    # the reference's own test inputs (catch/utils/tests/test_cluster.py): recorded (a, b) replayed through the family
    replayed = 0
    for c in recs:
        fam = lsh.MinHashFamily(c["k"], N=c["N"])
        sigs = fam.signatures(c["seqs"], ab=(c["a"], c["b"]))
        thr = cluster._jaccard_dist_from_mash_dist(c["threshold"], c["k"])
        lut = (1.0 - np.arange(c["N"] + 1, dtype=np.float64) / float(c["N"])).astype(np.float32)
        cl, merges = sigs.linkage_clusters(lut, thr, return_merges=True)
        dm = sigs.condensed(lut)
        sigs.close()
        assert [[c["names"][i] for i in x] for x in cl] == c["out"]
        # the matrix filled from the signatures is the condensed matrix, entry for entry
        cl2, merges2 = cluster.cluster_hierarchically_on_device(dm, thr, ctx=ctx, return_merges=True)
        assert cl2 == cl and _rows_of(merges2) == _rows_of(merges)
        if _scipy_hierarchy is not None and len(c["seqs"]) > 1:
            assert _rows_of(merges) == _rows_of(_scipy_hierarchy.linkage(dm, method="average"))
        replayed += 1
    assert replayed >= 3


@pytest.mark.gpu
def test_probe_designer_hierarchical_on_both_paths(ctx, monkeypatch):
    """A ProbeDesigner design with cluster_method="hierarchical" from the same golden file: the recorded clustered
    genomes and final probes with the linkage on the device and on the host."""
    from collections import OrderedDict
    from catch_amd.filter import duplicate_filter, probe_designer, set_cover_filter
    from catch_amd.genome import Genome
    g, _ = _hierarchical_records()
    designs = [c for c in g["designs"] if c["method"] == "hierarchical"]
    assert designs
    for c in designs:
        groups = [[Genome.from_chrs(OrderedDict(("c%d" % i, s) for i, s in enumerate(gn)))
                   if len(gn) > 1 else Genome.from_one_seq(gn[0]) for gn in grp] for grp in c["genomes"]]
        finals = {}
        for path in ("device", "host"):
            if path == "host":
                monkeypatch.setenv("CATCHHIP_CLUSTER_HOST_LINKAGE", "1")
            else:
                monkeypatch.delenv("CATCHHIP_CLUSTER_HOST_LINKAGE", raising=False)
            f = set_cover_filter.SetCoverFilter(mismatches=2, lcf_thres=100, coverage=1.0, cover_extension=20)
            pd = probe_designer.ProbeDesigner(
                groups, [duplicate_filter.DuplicateFilter(), f], probe_length=100, probe_stride=50,
                seq_length_to_skip=c["seq_length_to_skip"], cluster_threshold=c["threshold"],
                cluster_merge_after=f, cluster_method=c["method"], cluster_fragment_length=c["fragment_length"])
            random.seed(c["seed"])
            clustered = pd._cluster_genomes()
            assert pd.cluster_timings["linkage"] == path
            assert [[x.seqs[0] for x in cl] for cl in clustered] == c["clustered"]
            random.seed(c["seed"])
            pd.design()
            finals[path] = "\n".join(p.seq_str for p in pd.final_probes).encode()
            assert sorted(p.seq_str for p in pd.final_probes) == c["final"]
        assert finals["device"] == finals["host"]


@pytest.mark.gpu
def test_refusals(ctx):
    """A NaN or an infinity in the condensed matrix, or a length that is not n (n - 1) / 2: ValueError, as SciPy."""
    from catch_amd.utils import cluster
    good = np.linspace(0.1, 0.9, 10 * 9 // 2).astype(np.float32)
    assert sorted(map(len, cluster.cluster_hierarchically_on_device(good, 10.0, ctx=ctx))) == [10]
    for bad_value in (np.nan, np.inf, -np.inf):
        for at in (0, 17, good.size - 1):
            dm = good.copy()
            dm[at] = bad_value
            with pytest.raises(ValueError):
                cluster.cluster_hierarchically_on_device(dm, 0.5, ctx=ctx)
    for length in (2, 4, 44, 46):
        with pytest.raises(ValueError):
            cluster.cluster_hierarchically_on_device(np.full(length, 0.5, dtype=np.float32), 0.5, ctx=ctx)
    # the context is as usable as before
    assert cluster.cluster_hierarchically_on_device(good, 0.0, ctx=ctx) == [[i] for i in range(10)]


# ------------------------------------------------------------------ CPU
def test_host_part_on_the_fixtures_unsorted_merges():
    """catchhip_linkage_labels (stable sort by height, union-find relabelling, maximum heights, fcluster's walk) needs
    no device: the fixture's merges in production order -> its linkage matrix and its clusters at every threshold."""
    from catch_amd import _lib
    from catch_amd.utils import cluster
    L = _lib.lib()
    cases = _cases()
    assert set(SIZE_CASES + TIE_CASES + ["contraction"]) <= set(cases)
    # the fixture's middle sizes sit around the workgroup size of the kernel as it is built
    src = open(os.path.join(REPO, "catch_amd", "csrc", "linkage.hip")).read()
    assert int(re.search(r"#define LK_THREADS (\d+)", src).group(1)) == cases["size_1024"]["n"] == _golden["workgroup"]
    for name, case in cases.items():
        n = case["n"]
        u = case["unsorted"]
        merges = np.array([[a, b, float.fromhex(h), s] for a, b, h, s in _merge_rows(u)], dtype=np.float64).reshape(-1, 4)
        assert merges.shape[0] == n - 1
        for t, want in zip(case["thresholds"], case["clusters"]):
            labels = np.zeros(n, dtype=np.int32)
            out = np.zeros((max(n - 1, 1), 4), dtype=np.float64)
            _lib.check(L.catchhip_linkage_labels(n, merges.ctypes.data_as(_lib.c_f64p) if n > 1 else None,
                                                 float.fromhex(t), labels.ctypes.data_as(_lib.c_i32p),
                                                 out.ctypes.data_as(_lib.c_f64p)))
            assert cluster._clusters_from_labels(labels) == want, (name, t)
            assert _rows_of(out[:n - 1]) == _merge_rows(case["Z"]), name
            if _scipy_hierarchy is not None and n > 1 and n <= 1100:
                assert labels.tolist() == _scipy_hierarchy.fcluster(out[:n - 1], float.fromhex(t), criterion="distance").tolist()
    # merges that are no tree are refused, not walked
    bad = np.array([[0, 1, 0.5, 2], [0, 1, 0.6, 3]], dtype=np.float64)
    labels = np.zeros(3, dtype=np.int32)
    with pytest.raises(ValueError):
        _lib.check(L.catchhip_linkage_labels(3, bad.ctypes.data_as(_lib.c_f64p), 0.5, labels.ctypes.data_as(_lib.c_i32p), None))


def test_wrong_length_is_refused_before_the_device_is_touched():
    from catch_amd.utils import cluster
    for length in (2, 4, 5, 7):
        with pytest.raises(ValueError):
            cluster.cluster_hierarchically_on_device(np.zeros(length, dtype=np.float32), 0.5, ctx=object())


def test_symbols_sources_and_documents():
    """The new entry points are declared in the header and bound in _lib.py, the kernel file is built, the hooks are
    documented, and the product path asks SciPy for nothing unless it takes the host path."""
    from catch_amd import _lib, engine
    from catch_amd.utils import cluster
    hdr = open(os.path.join(REPO, "include", "catchhip.h")).read()
    for name in ("catchhip_sigs_linkage_average", "catchhip_linkage_average", "catchhip_linkage_labels",
                 "catchhip_linkage_fits"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.lib(), name)
    assert "linkage.hip" in open(os.path.join(REPO, "catch_amd", "csrc", "Makefile")).read()
    assert hasattr(engine.Signatures, "linkage_clusters") and hasattr(cluster, "cluster_hierarchically_on_device")
    src = open(os.path.join(REPO, "catch_amd", "csrc", "linkage.hip")).read()
    assert "__dmul_rn" in src and "__dadd_rn" in src and "__ddiv_rn" in src
    readme = open(os.path.join(REPO, "README.md")).read()
    for hook in ("CATCHHIP_CLUSTER_HOST_LINKAGE", "CATCHHIP_LINKAGE_MAX_N"):
        assert hook in readme
    assert not re.search(r"^(import|from)\s+scipy\b", open(os.path.join(REPO, "catch_amd", "utils", "cluster.py")).read(), re.M)
    assert ctypes.sizeof(ctypes.c_double) == 8
