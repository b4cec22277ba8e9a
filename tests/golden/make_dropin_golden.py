#!/usr/bin/env python3
"""Record what crosses the drop-in boundary -> tests/golden/dropin_calls.json.

Runs the UNMODIFIED reference CLI (bin/design.py) and the reference's
ProbeDesigner with catch_amd's modules registered at the reference's import
paths (catch.filter.set_cover_filter, catch.utils.cluster) behind recorders,
and keeps what crossed the boundary as data: the names the reference read from
each module, the constructor arguments, the call with its input, and the
reference's own answer to that same call.  tests/test_dropin_reference_cli.py
replays the calls against catch_amd.  Nothing from the reference is copied.

    PYTHONHASHSEED=0 python tests/golden/make_dropin_golden.py <checkout of broadinstitute/catch v1.5.2>
"""
import importlib
import importlib.util  # noqa: F401  (the reference's dynamic_load relies on it being imported)
import json
import os
import random
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(REF, "bin"), REF, REPO]

import numpy as np  # noqa: E402

import catch.filter  # noqa: E402
import catch.utils  # noqa: E402
from catch.filter import probe_designer as ref_probe_designer  # noqa: E402
from catch.filter import set_cover_filter as ref_scf  # noqa: E402
from catch.utils import cluster as ref_cluster  # noqa: E402
from catch import genome as ref_genome  # noqa: E402
from catch_amd import _lib  # noqa: E402
from catch_amd.filter import set_cover_filter as gpu_scf  # noqa: E402
from catch_amd.utils import cluster as gpu_cluster  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402

# the input of the design CLI run: two 1.5-kb genomes of one species, one FASTA = one group
DESIGN_ARGS = ["-pl", "75", "-m", "2", "-e", "50"]


class Recorder:
    """Stands at a reference import path: hands out the catch_amd module's names (or `overrides`), recording which."""

    def __init__(self, target, overrides):
        self._target, self._overrides, self._names = target, overrides, []

    def __getattr__(self, name):
        if not name.startswith("__") and name not in self._names:
            self._names.append(name)
        return self._overrides[name] if name in self._overrides else getattr(self._target, name)


def register(path, parent, attr, rec):
    sys.modules[path] = rec
    setattr(parent, attr, rec)


def seeded():
    random.seed(0)
    np.random.seed(0)


def design_cli():
    seen = {}

    class RecordingSetCoverFilter(gpu_scf.SetCoverFilter):
        def __init__(self, *args, **kw):
            seen["init_args"], seen["init_kwargs"] = list(args), dict(kw)
            super().__init__(*args, **kw)

        def filter(self, input, target_genomes=None, **kw):
            assert kw.get("input_is_grouped")
            seen["filter_kwargs"] = dict(kw)
            seen["objects"] = (input, target_genomes)
            return super().filter(input, target_genomes, **kw)

    rec = Recorder(gpu_scf, {"SetCoverFilter": RecordingSetCoverFilter})
    register("catch.filter.set_cover_filter", catch.filter, "set_cover_filter", rec)
    sys.modules.pop("design", None)
    design = importlib.import_module("design")
    assert design.set_cover_filter is rec
    rng = np.random.Generator(np.random.PCG64(1))
    g = synthetic.make_species(rng, [1500], 2, 1, 0.0, 0.02, with_n=False)
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "t.fasta")
        with open(fa, "w") as f:
            f.write("".join(">g%d\n%s\n" % (i, x[0]) for i, x in enumerate(g)))
        sys.argv = ["design.py", fa] + DESIGN_ARGS + ["-o", os.path.join(tmp, "probes.fasta")]
        args = design.init_and_parse_args("basic")
        try:
            design.main(args)
        except _lib.CatchHipError:
            pass            # no GPU here: the call reached catch_amd's filter and stopped at device creation
    register("catch.filter.set_cover_filter", catch.filter, "set_cover_filter", ref_scf)
    input, targets = seen.pop("objects")
    # the reference's own filter on the same call
    seeded()
    ref_out = ref_scf.SetCoverFilter(*seen["init_args"], **seen["init_kwargs"]).filter(
        input, targets, **seen["filter_kwargs"])
    return dict(design_args=DESIGN_ARGS, names_read=rec._names, init_args=seen["init_args"],
                init_kwargs=seen["init_kwargs"], filter_kwargs=seen["filter_kwargs"],
                filter_input=[[p.seq_str for p in grp] for grp in input],
                target_genomes=[[list(gn.seqs) for gn in grp] for grp in targets],
                reference_selected=[sorted(p.seq_str for p in grp) for grp in ref_out])


def probe_designer_clustering():
    seen = {}

    def recording_cluster(seqs, **kw):
        seen["seqs"], seen["kwargs"] = dict(seqs), dict(kw)
        return gpu_cluster.cluster_with_minhash_signatures(seqs, **kw)

    rec = Recorder(gpu_cluster, {"cluster_with_minhash_signatures": recording_cluster})
    register("catch.utils.cluster", catch.utils, "cluster", rec)
    ref_probe_designer.cluster = rec
    from catch.filter import duplicate_filter
    gs = [[ref_genome.Genome.from_one_seq("ATTA" * 500), ref_genome.Genome.from_one_seq("CGGC" * 500)]]

    def designer():
        df = duplicate_filter.DuplicateFilter()
        return ref_probe_designer.ProbeDesigner(gs, [df], probe_length=100, probe_stride=50, cluster_threshold=0.1,
                                                cluster_merge_after=df, cluster_method="simple",
                                                cluster_fragment_length=500)
    try:
        designer()._cluster_genomes()
    except _lib.CatchHipError:
        pass
    register("catch.utils.cluster", catch.utils, "cluster", ref_cluster)
    ref_probe_designer.cluster = ref_cluster
    seeded()
    ref_clusters = ref_cluster.cluster_with_minhash_signatures(seen["seqs"], **seen["kwargs"])
    seeded()
    genome_clusters = len(designer()._cluster_genomes())
    return dict(names_read=rec._names, seqs=[[k, v] for k, v in seen["seqs"].items()], kwargs=seen["kwargs"],
                reference_clusters=[list(c) for c in ref_clusters], reference_genome_clusters=genome_clusters)


if __name__ == "__main__":
    out = dict(what="calls the reference made across the drop-in boundary, with the reference's own answers "
                    "(tests/golden/make_dropin_golden.py; replayed by tests/test_dropin_reference_cli.py); "
                    "answers were computed after random.seed(0) and np.random.seed(0)",
               design_cli=design_cli(), probe_designer_clustering=probe_designer_clustering())
    with open(os.path.join(HERE, "dropin_calls.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
