"""Grid design: probes for every (dataset, mismatches, cover extension) point.

The reference README's option #3 runs design.py once per taxon over a grid of
--mismatches x --cover-extension values and hands the probe counts to pool.py
(catch/utils/pool_probes_io.py:11-60 reads the table).  Here each dataset is
read, uploaded and run through its front end (candidates, duplicate or near-
duplicate filter) once; its anchor table and cover scan run once per m; the
rows at every cover extension are derived from that one scan on the device
(catchhip_setcover_grid) and solved.  Point (d, m, e) selects exactly what
`python -m catch_amd.design d -m m -e e` selects when np.random and random are
in the state design_grid found them in.
"""
import concurrent.futures
import logging
import os
import random

import numpy as np

from catch_amd import engine
from catch_amd.filter import candidate_probes, duplicate_filter
from catch_amd.filter import near_duplicate_filter, polya_filter, probe_designer
from catch_amd.filter import set_cover_filter

logger = logging.getLogger(__name__)

TABLE_HEADER = ("dataset", "mismatches", "cover_extension", "num_probes")


def dataset_name(path):
    """The FASTA basename without .fasta / .fa / .fna and an optional .gz."""
    name = os.path.basename(path)
    if name.endswith(".gz"):
        name = name[:-3]
    for ext in (".fasta", ".fa", ".fna"):
        if name.endswith(ext):
            return name[:-len(ext)]
    return name


def check_grid_values(name, values):
    values = list(values)
    if len(values) == 0:
        raise ValueError("%s: no values given" % name)
    dup = sorted({v for v in values if values.count(v) > 1})
    if dup:
        raise ValueError("%s: duplicate values %s" % (name, dup))
    if any(v < 0 for v in values):
        raise ValueError("%s: negative values are not allowed" % name)
    return values


def write_probe_count_table(counts, out):
    """counts: [(dataset, m, e, num_probes)] in table order; out: a path or a
    file object.  The table pool.py reads (pool_probes_io.read_table_of_probe_counts)."""
    lines = ["\t".join(TABLE_HEADER)]
    seen = set()
    for d, m, e, n in counts:
        if (d, m, e) in seen:
            raise ValueError("duplicate table row for %s m=%d e=%d" % (d, m, e))
        seen.add((d, m, e))
        lines.append("%s\t%d\t%d\t%d" % (d, m, e, n))
    text = "\n".join(lines) + "\n"
    if hasattr(out, "write"):
        out.write(text)
    else:
        with open(out, "w") as f:
            f.write(text)


def _first_filter(probe_length, filter_with_lsh_hamming, filter_with_lsh_minhash):
    """The filter before the set cover, as catch_amd.design builds it."""
    if filter_with_lsh_hamming is not None and filter_with_lsh_minhash is not None:
        raise Exception("Cannot use both --filter-with-lsh-hamming "
                        "and --filter-with-lsh-minhash")
    if filter_with_lsh_hamming is not None:
        return near_duplicate_filter.NearDuplicateFilterWithHammingDistance(
            filter_with_lsh_hamming, probe_length)
    if filter_with_lsh_minhash is not None:
        return near_duplicate_filter.NearDuplicateFilterWithMinHash(
            filter_with_lsh_minhash)
    return duplicate_filter.DuplicateFilter()


class _Prepared:
    """One dataset after its front end: device targets, the unique candidates
    (on the device, or as host strings) and the anchors of every m."""

    def __init__(self, index, ctx, genomes):
        self.index = index
        self.ctx = ctx
        self.genomes = genomes
        self.targets = None
        self.cands = None        # engine.Candidates (device front end)
        self.uniq = None         # host strings (host front end)
        self.anchors = {}        # m -> what _probes_for(m) needs
        self.universe_p = None

    @property
    def num_sets(self):
        if self.cands is not None:
            return self.cands.n
        return len(self.uniq) if self.uniq is not None else 0

    def probes_for(self, m):
        a = self.anchors[m]
        if self.cands is not None:
            return set_cover_filter._probes_of_candidates(self.cands, a)
        k, uniq, owner, ep, eo = a
        return engine.Probes(self.ctx, uniq, owner, ep, eo, k)

    def strings(self, ids, probe_length):
        if self.cands is not None:
            ids_arr = np.asarray(ids, dtype=np.int64)
            seqs = [s for g in self.genomes for s in g.seqs]
            pos = self.cands.positions(ids_arr)
            which = np.searchsorted(self.targets.seq_off, pos, side="right") - 1
            local = pos - self.targets.seq_off[which]
            return [seqs[q][o:o + probe_length] for q, o in zip(which.tolist(), local.tolist())]
        return [self.uniq[i] for i in ids]

    def close(self):
        for h in (self.cands, self.targets):
            if h is not None:
                h.close()
        self.cands = self.targets = None


def design_grid(datasets, mismatches, cover_extensions, probe_length=100,
                probe_stride=50, lcf_thres=None, island_of_exact_match=0,
                coverage=1.0, filter_with_lsh_hamming=None,
                filter_with_lsh_minhash=None, small_seq_skip=None,
                small_seq_min=None, kmer_probe_map_k=None,
                scan_mode=engine.SCAN_AUTO, stats=None, filter_polya=None,
                filter_composition=None, filter_structure=None, filter_tm=None,
                filter_background=None, candidate_profile=None):
    """Probes for every (dataset, m, e) point.

    datasets: list of datasets, each a list of Genome objects (one FASTA file =
    one dataset).  mismatches, cover_extensions: the grid values.  The other
    options are catch_amd.design's (filter_polya: the (length, mismatches)
    of --filter-polya -- per dataset and a function of the candidate alone,
    so it is part of the front end every grid point shares;
    filter_composition: a composition_filter.CompositionFilter, applied right
    after it in the same way, its `dropped` counts summed over the
    datasets; filter_structure: a structure_filter.StructureFilter, after
    that one, likewise; filter_tm: a tm_filter.TmFilter, after that one,
    likewise -- every dataset passes it once, so its histogram counts a dataset's
    candidates once, not once per grid point; filter_background: a
    background_filter.BackgroundFilter, after that one, likewise;
    candidate_profile: a quality.QualityProfile, which only measures, right
    after the poly(A) filter -- once per dataset, like the Tm histogram).  Returns
    {(dataset index, m, e): probe sequences in the order the set cover picked them}.  stats (a dict, may be
    None) receives the number of grid calls (scans of a (dataset, m)), derived
    row tables and solves."""
    mismatches = check_grid_values("mismatches", mismatches)
    cover_extensions = check_grid_values("cover extensions", cover_extensions)
    lcf = lcf_thres if lcf_thres is not None else probe_length
    if coverage > 1:
        coverage = int(coverage)
    if small_seq_skip is not None and small_seq_min is not None:
        raise Exception("Both --small-seq-skip and --small-seq-min were given: "
                        "one skips short sequences, the other designs on them")
    if kmer_probe_map_k:
        if kmer_probe_map_k > probe_length:
            raise Exception("--kmer-probe-map-k (%d) exceeds the probe length (%d)"
                            % (kmer_probe_map_k, probe_length))
        k_scf = kmer_probe_map_k
    else:
        if probe_length <= 20:
            logger.warning("The probe length (%d) is small: consider a "
                           "--kmer-probe-map-k below it", probe_length)
        k_scf = 20
    # per m, the warnings catch_amd.design gives at that m
    scfs = {}
    for m in mismatches:
        if filter_with_lsh_hamming is not None and filter_with_lsh_minhash is None:
            if filter_with_lsh_hamming > m:
                logger.warning("Nearly duplicate probes are filtered by calling "
                               "near-duplicates probes within a Hamming distance "
                               "that exceeds --mismatches")
        elif filter_with_lsh_minhash is not None and filter_with_lsh_hamming is None:
            if m < 3:
                logger.warning("MISMATCHES is set to %d; at low values using "
                               "--filter-with-lsh-minhash may cause the probes to "
                               "achieve less than the desired coverage", m)
        scfs[m] = set_cover_filter.SetCoverFilter(
            mismatches=m, lcf_thres=lcf, island_of_exact_match=island_of_exact_match,
            coverage=coverage, cover_extension=0, kmer_probe_map_k=k_scf)
        scfs[m].scan_mode = scan_mode
    _first_filter(probe_length, filter_with_lsh_hamming, filter_with_lsh_minhash)   # (argument checks)
    pre_filters = []
    if filter_polya:
        # the warnings catch_amd.design gives
        polya_length, polya_mismatches = filter_polya
        if polya_length > probe_length:
            logger.warning(("Length of poly(A) stretch to filter (%d) is "
                            "greater than PROBE_LENGTH (%d), which is usually "
                            "undesirable"), polya_length, probe_length)
        if polya_length < 10:
            logger.warning(("Length of poly(A) stretch to filter (%d) is "
                            "short, and may lead to many probes being "
                            "filtered"), polya_length)
        if polya_mismatches > 10:
            logger.warning(("Number of mismatches to tolerate when searching "
                            "for poly(A) stretches (%d) is high, and may "
                            "lead to many probes being filtered"),
                           polya_mismatches)
        pre_filters.append(polya_filter.PolyAFilter(polya_length, polya_mismatches))
    if candidate_profile is not None:
        pre_filters.append(candidate_profile)
    if filter_composition is not None:
        pre_filters.append(filter_composition)
    if filter_structure is not None:
        pre_filters.append(filter_structure)
    if filter_tm is not None:
        pre_filters.append(filter_tm)
    if filter_background is not None:
        pre_filters.append(filter_background)

    np_state0, py_state0 = np.random.get_state(), random.getstate()
    out = {}
    counters = dict(grid_calls=0, scans=0, derived=0, solves=0)

    def prepare(di, ctx):
        """The front end of dataset di on ctx and every m's anchors, all random
        draws on this (the calling) thread in the order a single design run
        makes them."""
        genomes = datasets[di]
        np.random.set_state(np_state0)
        random.setstate(py_state0)
        first = _first_filter(probe_length, filter_with_lsh_hamming, filter_with_lsh_minhash)
        scf0 = scfs[mismatches[0]]
        pd = probe_designer.ProbeDesigner(
            [genomes], [first, scf0], probe_length=probe_length, probe_stride=probe_stride,
            allow_small_seqs=small_seq_min, seq_length_to_skip=small_seq_skip)
        P = _Prepared(di, ctx, genomes)
        try:
            mode = pd._device_front_end_mode([genomes], first, scf0)
            P.universe_p = scf0._make_universe_p(genomes)
            ndf = None if type(first) is duplicate_filter.DuplicateFilter else first
            if mode is not None:
                # catch/filter/set_cover_filter.py's _filter_genomes_device, one group
                P.targets = engine.Targets(ctx, [g.seqs for g in genomes])
                P.cands = engine.Candidates(ctx, P.targets, probe_length, probe_stride, small_seq_skip)
                for f in pre_filters:
                    f._apply_to_candidates(P.cands)
                if ndf is not None:
                    ndf._apply_to_candidates(P.cands)
                if P.cands.n == 0:
                    logger.warning("There are no candidate probes for a grouping of genomes")
            elif len(genomes) > 0:
                # ProbeDesigner._design_on_strings's host front end
                cand = []
                for g in genomes:
                    cand += candidate_probes.candidate_strings_from_sequences(
                        list(g.seqs), probe_length, probe_stride, **pd._window_options())
                if len(cand) == 0:
                    logger.warning("There are no candidate probes for a grouping of genomes")
                for f in pre_filters:
                    cand = f._filter_strs(cand)
                if ndf is None:
                    P.uniq = list(dict.fromkeys(cand))
                elif hasattr(ndf, "_filter_strs_many"):
                    P.uniq = ndf._filter_strs_many([cand])[0]
                else:
                    P.uniq = ndf._filter_strs(cand)
                if P.uniq:
                    P.targets = engine.Targets(ctx, [g.seqs for g in genomes])
            if P.targets is None or P.num_sets == 0:
                return P
            np_state1, py_state1 = np.random.get_state(), random.getstate()
            for m in mismatches:
                np.random.set_state(np_state1)
                random.setstate(py_state1)
                if P.cands is not None:
                    P.anchors[m] = set_cover_filter._anchors_for_candidates(
                        P.cands.n, probe_length, m, lcf, k_scf)
                else:
                    from catch_amd import probe
                    P.anchors[m] = probe.anchor_table(P.uniq, m, lcf, min_k=k_scf, k=k_scf,
                                                      assume_unique=True)
        except BaseException:
            P.close()
            raise
        return P

    def run(P):
        """The device work of one dataset on its own context (a worker thread)."""
        res, local = {}, dict(grid_calls=0, scans=0, derived=0, solves=0)
        for m in mismatches:
            if P.targets is None or P.num_sets == 0:
                for e in cover_extensions:
                    res[(P.index, m, e)] = []
                continue
            probes = P.probes_for(m)
            try:
                got = engine.setcover_grid(
                    P.ctx, probes, P.targets, m, lcf, island_of_exact_match,
                    cover_extensions, P.num_sets, None, P.universe_p, scan_mode)
                c = P.ctx.grid_counters()
            finally:
                probes.close()
            local["grid_calls"] += 1
            local["scans"] += c["scans"]
            local["derived"] += c["derived"]
            local["solves"] += c["solves"]
            for e, (ids, _nrows) in zip(cover_extensions, got):
                res[(P.index, m, e)] = P.strings(ids, probe_length)
        return res, local

    width = max(1, int(os.environ.get("CATCHHIP_GROUPS_IN_FLIGHT", "4")))
    width = min(width, max(1, len(datasets)))
    ctxs = set_cover_filter._contexts(width)
    slots = [None] * width       # (prepared, future) per context
    with concurrent.futures.ThreadPoolExecutor(max_workers=width,
                                               thread_name_prefix="catchhip-grid") as pool:
        def collect(slot):
            P, fut = slots[slot]
            slots[slot] = None
            try:
                res, local = fut.result()
            finally:
                P.close()
            out.update(res)
            for k, v in local.items():
                counters[k] += v

        try:
            for di in range(len(datasets)):
                slot = di % width
                if slots[slot] is not None:
                    collect(slot)      # the context is free again
                P = prepare(di, ctxs[slot])
                slots[slot] = (P, pool.submit(run, P))
            for slot in range(width):
                if slots[slot] is not None:
                    collect(slot)
        finally:
            for slot in range(width):
                if slots[slot] is not None:
                    P, fut = slots[slot]
                    try:
                        fut.result()
                    except BaseException:    # noqa: BLE001 -- the first error is the one raised
                        pass
                    P.close()
    if stats is not None:
        stats.update(counters)
    return out
