"""Drop-in boundary: the UNMODIFIED reference CLI (bin/design.py) picks up the
GPU SetCoverFilter, and the reference's ProbeDesigner the GPU clustering, when
they are registered at the reference's import paths.

What crossed the boundary when the reference ran that way -- the names it read
from each module, the constructor arguments, the call with its input, and the
reference's own answer to that call -- is recorded in
tests/golden/dropin_calls.json (tests/golden/make_dropin_golden.py).  These
tests replay those calls against catch_amd: without a GPU a call must reach
our code and stop at device creation; with one it must return the reference's
answer."""
import json
import os
import random

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropin_calls.json")


def _calls(name):
    with open(GOLDEN) as f:
        return json.load(f)[name]


def _seeded():
    # the reference's answers were recorded after these seeds
    random.seed(0)
    np.random.seed(0)


def test_reference_design_cli_reaches_gpu_filter(monkeypatch):
    from catch_amd import _lib, engine, genome, probe
    from catch_amd.filter import set_cover_filter as gpu_scf
    rec = _calls("design_cli")
    assert rec["design_args"] == ["-pl", "75", "-m", "2", "-e", "50"]
    assert rec["names_read"]
    for name in rec["names_read"]:
        assert hasattr(gpu_scf, name), name

    seen = {}
    orig = gpu_scf.SetCoverFilter._filter

    def spy(self, input, target_genomes_grouped):
        seen["groups"] = [len(x) for x in input]
        seen["genomes"] = [len(x) for x in target_genomes_grouped]
        seen["params"] = (self.mismatches, self.lcf_thres, self.cover_extension)
        return orig(self, input, target_genomes_grouped)

    monkeypatch.setattr(gpu_scf.SetCoverFilter, "_filter", spy)
    scf = gpu_scf.SetCoverFilter(*rec["init_args"], **rec["init_kwargs"])
    input = [[probe.Probe.from_str(s) for s in grp] for grp in rec["filter_input"]]
    targets = [[genome.Genome.from_one_seq(seqs[0]) for seqs in grp] for grp in rec["target_genomes"]]
    assert all(len(seqs) == 1 for grp in rec["target_genomes"] for seqs in grp)
    if engine.device_count() > 0:
        _seeded()
        out = scf.filter(input, targets, **rec["filter_kwargs"])
        assert [sorted(p.seq_str for p in grp) for grp in out] == rec["reference_selected"]
    else:
        with pytest.raises(_lib.CatchHipError):
            scf.filter(input, targets, **rec["filter_kwargs"])
    assert seen["genomes"] == [2] and seen["groups"][0] > 20
    assert seen["params"] == (2, 75, 50)


def test_reference_probe_designer_reaches_gpu_clustering():
    """--cluster-and-design-separately: the reference's ProbeDesigner calls
    catch.utils.cluster.cluster_with_minhash_signatures; with catch_amd's
    module registered there it receives the sequences and, with a GPU, returns
    the reference's clusters."""
    from catch_amd import _lib, engine
    from catch_amd.utils import cluster as gpu_cluster
    rec = _calls("probe_designer_clustering")
    assert rec["names_read"] == ["cluster_with_minhash_signatures"]
    for name in rec["names_read"]:
        assert hasattr(gpu_cluster, name), name
    seqs = {k: v for k, v in rec["seqs"]}
    assert len(seqs) == 8 and rec["kwargs"] == dict(threshold=0.1, cluster_method="simple")
    assert rec["reference_genome_clusters"] == 2
    if engine.device_count() > 0:
        _seeded()
        got = gpu_cluster.cluster_with_minhash_signatures(seqs, **rec["kwargs"])
        assert [list(c) for c in got] == rec["reference_clusters"]
    else:
        with pytest.raises(_lib.CatchHipError):
            gpu_cluster.cluster_with_minhash_signatures(seqs, **rec["kwargs"])
